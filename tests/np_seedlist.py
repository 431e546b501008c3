"""Restatement of the list half of the reference's depth filter, loop for loop (test infrastructure only):

  DepthFilter::initializeSeeds                                  src/depth_filter.cpp:177-191
  DepthFilter::removeKeyframe                                   src/depth_filter.cpp:199-216
  DepthFilter::updatePointSeeds / updateLineSeeds, the lists    src/depth_filter.cpp:270-365, :367-471
      the age test (:289-292), the erasing of converged and NaN seeds, the converged-seed callbacks (:334-360, :439-467)
  PointSeed::PointSeed / LineSeed::LineSeed                     src/depth_filter.cpp:53-74

Written as the reference is: Python lists, one loop per reference loop.  The per-seed body (the epipolar search and the posterior) is NOT
restated here: update() takes it as a function, commit() takes its results as rows.  A stream's seeds are
dict(pt=[..], seg=[..], batch_counter=int); a point seed is dict(ref_kf, batch_id, px, f, level, type, grad, a, b, mu, z_range, sigma2),
a line seed dict(ref_kf, batch_id, px, f, sf, ef, spx, epx, level, a, b, mu_s, mu_e, z_range_s, z_range_e, sigma2_s, sigma2_e), the
float members as numpy.float32.  The map is the stream dict of tests/np_candidates.py that tests/np_newcand.py appends to.

Pins (where this and the device depart from the reference on purpose):
  * Seed::batch_counter is ONE static shared by both kinds and by every filter (src/depth_filter.cpp:44); here it is per stream.
  * removeKeyframe erases only the POINT seeds of the keyframe; its line seeds keep a pointer to a frame that may be gone.  Here the line
    seeds of a removed keyframe are erased too.
  * ref_kf is an index into the stream's keyframe table as it stands: a removal decrements every index above the removed one, as the
    table closes up.
  * No room is all-or-nothing per stream: when the map tables cannot take ALL converged seeds of an update, the stream's update is
    dropped as a whole (nothing changes, the report says so)."""
import copy

import numpy as np

import np_newcand as NC

NOT_VISIBLE, NO_MATCH, UPDATED, CONVERGED, NAN, AGED = 0, 1, 2, 3, 4, 5
PT_PARAMS = ("a", "b", "mu", "sigma2")
SEG_PARAMS = ("a", "b", "mu_s", "mu_e", "sigma2_s", "sigma2_e")
f32 = np.float32


def new_point_seed(ftr, ref_kf, batch_id, depth_mean, depth_min):
    """PointSeed::PointSeed(ftr, float depth_mean, float depth_min) (:53-61)"""
    depth_mean, depth_min = f32(depth_mean), f32(depth_min)
    z_range = f32(1.0 / float(depth_min))
    return dict(ref_kf=ref_kf, batch_id=batch_id, px=list(ftr["px"]), f=list(ftr["f"]), level=int(ftr["level"]), type=int(ftr["type"]), grad=list(ftr["grad"]),
                a=f32(10), b=f32(10), mu=f32(1.0 / float(depth_mean)), z_range=z_range, sigma2=f32(z_range * z_range) / f32(36))


def new_line_seed(ftr, ref_kf, batch_id, depth_mean, depth_min):
    """LineSeed::LineSeed (:63-74)"""
    depth_mean, depth_min = f32(depth_mean), f32(depth_min)
    z_range = f32(1.0 / float(depth_min))
    mu, sigma2 = f32(1.0 / float(depth_mean)), f32(z_range * z_range) / f32(36)
    return dict(ref_kf=ref_kf, batch_id=batch_id, px=list(ftr["px"]), f=list(ftr["f"]), sf=list(ftr["sf"]), ef=list(ftr["ef"]), spx=list(ftr["spx"]), epx=list(ftr["epx"]),
                level=int(ftr["level"]), a=f32(10), b=f32(10), mu_s=mu, mu_e=mu, z_range_s=z_range, z_range_e=z_range, sigma2_s=sigma2, sigma2_e=sigma2)


def keyframe(seeds, removed_kf=-1, new_batch=False, new_kf=0, depth_mean=1.0, depth_min=1.0, new_pt=(), new_seg=()):
    """a keyframe event on one stream's lists (mutated), in the device's order: removeKeyframe, ++batch_counter, initializeSeeds"""
    if removed_kf >= 0:                                               # removeKeyframe (:199-216), line seeds included (pin)
        for kind in ("pt", "seg"):
            it = 0
            while it < len(seeds[kind]):
                if seeds[kind][it]["ref_kf"] == removed_kf:
                    del seeds[kind][it]
                else:
                    it += 1
            for sd in seeds[kind]:                                    # the keyframe table closes up
                if sd["ref_kf"] > removed_kf:
                    sd["ref_kf"] -= 1
    if new_batch:                                                     # ++Seed::batch_counter (:181)
        seeds["batch_counter"] += 1
    for ftr in new_pt:                                                # seeds_.push_back(PointSeed(ftr, new_keyframe_mean_depth_, new_keyframe_min_depth_)) (:184-186)
        seeds["pt"].append(new_point_seed(ftr, new_kf, seeds["batch_counter"], depth_mean, depth_min))
    for ftr in new_seg:
        seeds["seg"].append(new_line_seed(ftr, new_kf, seeds["batch_counter"], depth_mean, depth_min))


def aged(seeds, sd, max_n_kfs):
    """(Seed::batch_counter - it->batch_id) > options_.max_n_kfs (:289)"""
    return seeds["batch_counter"] - sd["batch_id"] > max_n_kfs


def _room_of(st, room):
    return room is None or (len(st["pt_pos"]) <= room["rows_pt"] and len(st["seg_spos"]) <= room["rows_seg"] and len(st["pt_cand"]) <= room["rows_pt_cand"] and
                            len(st["seg_cand"]) <= room["rows_seg_cand"] and sum(len(l) for l in st["pt_obs"]) <= room["cap_pt_obs"] and
                            sum(len(l) for l in st["seg_obs"]) <= room["cap_seg_obs"])


def report_of(seeds, st, counts=None, first=(-1, -1), no_room=0):
    counts = counts or dict(pt=[0] * 6, seg=[0] * 6)
    return dict(pt=list(counts["pt"]), seg=list(counts["seg"]), first_pt=first[0], first_seg=first[1], n_pt_seeds=len(seeds["pt"]), n_seg_seeds=len(seeds["seg"]),
                n_pt=len(st["pt_pos"]), n_seg=len(st["seg_spos"]), n_pt_cand=len(st["pt_cand"]), n_seg_cand=len(st["seg_cand"]),
                n_pt_obs=sum(len(l) for l in st["pt_obs"]), n_seg_obs=sum(len(l) for l in st["seg_obs"]), no_room=no_room, batch_counter=seeds["batch_counter"])


def commit(seeds, st, rows, room=None):
    """what updatePointSeeds / updateLineSeeds do with the lists once the body of every seed has run: rows = dict(pt=[..], seg=[..]) in list
    order, a row dict(status, the new parameters, xyz (points) or xyz_s / xyz_e).  Mutates seeds and st unless the stream lacks room.
    Returns (report, events): the report of plsvo_seeds_update_fetch and the event bytes np_newcand.add reports."""
    seeds2, st2 = copy.deepcopy(seeds), copy.deepcopy(st)
    counts = dict(pt=[0] * 6, seg=[0] * 6)
    new = dict(pt=[], seg=[])
    for kind, params in (("pt", PT_PARAMS), ("seg", SEG_PARAMS)):
        assert len(rows[kind]) == len(seeds2[kind])
        it = 0
        for row in rows[kind]:                                        # the loop over the list (:287, :383): `it` advances or the seed is erased
            sd = seeds2[kind][it]
            counts[kind][row["status"]] += 1
            if row["status"] == AGED:                                 # :289-292
                del seeds2[kind][it]
                continue
            if row["status"] == CONVERGED:                            # :334-355 / :439-462: the landmark, the callback, the erase
                obs = dict(kf=sd["ref_kf"], level=sd["level"])
                if kind == "pt":
                    obs.update(px=sd["px"], f=sd["f"], type=sd["type"], grad=sd["grad"])
                    new["pt"].append(dict(pos=row["xyz"], obs=obs))
                else:
                    obs.update(spx=sd["spx"], epx=sd["epx"], sf=sd["sf"], ef=sd["ef"])
                    new["seg"].append(dict(spos=row["xyz_s"], epos=row["xyz_e"], obs=obs))
                del seeds2[kind][it]
                continue
            if row["status"] == NAN:                                  # :356-360 / :463-467
                del seeds2[kind][it]
                continue
            for p in params:                                          # NOT_VISIBLE, NO_MATCH, UPDATED: the seed stays with what the body left
                sd[p] = f32(row[p])
            it += 1
    rep = NC.add(st2, new)
    if not _room_of(st2, room):
        return report_of(seeds, st, counts, no_room=1), (None, None)
    for k in list(seeds):
        seeds[k] = seeds2[k]
    for k in list(st2):
        st[k] = st2[k]
    return report_of(seeds, st, counts, (rep["first_pt"], rep["first_seg"])), (rep["pt_event"], rep["seg_event"])


def update(seeds, st, body, max_n_kfs, room=None):
    """updatePointSeeds, then updateLineSeeds, with a frame: body(kind, seed) -> the row of a seed that is not aged.  Returns what commit()
    returns, and the rows (the device's shadow rows)."""
    rows = dict(pt=[], seg=[])
    for kind, params in (("pt", PT_PARAMS), ("seg", SEG_PARAMS)):
        for sd in seeds[kind]:
            if aged(seeds, sd, max_n_kfs):
                row = dict({p: sd[p] for p in params}, status=AGED)
                row.update(dict(xyz=[0.0] * 3) if kind == "pt" else dict(xyz_s=[0.0] * 3, xyz_e=[0.0] * 3))
            else:
                row = body(kind, sd)
            rows[kind].append(row)
    rep, ev = commit(seeds, st, rows, room)
    return rep, ev, rows


# ---- the lists as the arrays of plsvo_seed_list / plsvo_seed_rows -------------------------------------------------------------------------
PT_LIST = (("pt_ref_kf", "ref_kf"), ("pt_batch_id", "batch_id"), ("pt_px", "px"), ("pt_f", "f"), ("pt_level", "level"), ("pt_type", "type"), ("pt_grad", "grad"), ("pt_a", "a"),
           ("pt_b", "b"), ("pt_mu", "mu"), ("pt_z_range", "z_range"), ("pt_sigma2", "sigma2"))
SEG_LIST = (("seg_ref_kf", "ref_kf"), ("seg_batch_id", "batch_id"), ("seg_px", "px"), ("seg_f", "f"), ("seg_sf", "sf"), ("seg_ef", "ef"), ("seg_spx", "spx"), ("seg_epx", "epx"),
            ("seg_level", "level"), ("seg_a", "a"), ("seg_b", "b"), ("seg_mu_s", "mu_s"), ("seg_mu_e", "mu_e"), ("seg_z_range_s", "z_range_s"), ("seg_z_range_e", "z_range_e"),
            ("seg_sigma2_s", "sigma2_s"), ("seg_sigma2_e", "sigma2_e"))
PT_ROWS = (("pt_status", "status"), ("pt_a", "a"), ("pt_b", "b"), ("pt_mu", "mu"), ("pt_sigma2", "sigma2"), ("pt_xyz_world", "xyz"))
SEG_ROWS = (("seg_status", "status"), ("seg_a", "a"), ("seg_b", "b"), ("seg_mu_s", "mu_s"), ("seg_mu_e", "mu_e"), ("seg_sigma2_s", "sigma2_s"), ("seg_sigma2_e", "sigma2_e"),
            ("seg_xyz_world_s", "xyz_s"), ("seg_xyz_world_e", "xyz_e"))


def lists_of(seeds):
    """the arrays capi.Context.seeds_stage takes and seeds_fetch_lists returns"""
    d = dict(batch_counter=seeds["batch_counter"])
    for kind, names in (("pt", PT_LIST), ("seg", SEG_LIST)):
        for f, k in names:
            d[f] = [sd[k] for sd in seeds[kind]]
    return d


def rows_of(rows):
    """the arrays capi.Context.seeds_commit_rows takes"""
    d = {}
    for kind, names in (("pt", PT_ROWS), ("seg", SEG_ROWS)):
        for f, k in names:
            d[f] = [r[k] for r in rows[kind]]
    return d
