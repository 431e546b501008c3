"""Cases of the resident seed lists (plsvo_seeds_*), shared by tests/test_seedlist_host.py and tests/test_gpu_seedlist.py.  The maps are the
thirteen streams of tests/newcand_cases.py (the insertion's preconditions hold); on top of a stream a case carries its seed lists in the form
tests/np_seedlist.py reads, and constructed shadow rows -- status, new parameters, xyz_world -- for the commit.  A seed's feature and the
position it converges to come from newcand_cases.make_new: a landmark in view of the stream's frame, observed in one keyframe of the table
as it stands (the first, the last, then in turn), every third point an edgelet with gradients.  Built once (seeded), never changed."""
import copy
import functools

import numpy as np

import insert_cases as Ic
import newcand_cases as Nc
import np_seedlist as SL

CAM_T, CAM, CELL, SEG_CELL, BOUNDARY, PARAMS = Nc.CAM_T, Nc.CAM, Nc.CELL, Nc.SEG_CELL, Nc.BOUNDARY, Nc.PARAMS
LM_RESERVE, RESERVE = Nc.LM_RESERVE, Nc.RESERVE
MAX_N_KFS = 3
COUNTER = 7                                                           # every stream's batch counter
SEED_RESERVE = dict(extra_pt=70, extra_seg=70)
# (point seeds, line seeds) per stream and what their constructed rows say: both sides of the 64-lane round per kind
SEEDS = ((1, 130), (0, 0), (63, 64), (64, 0), (0, 63), (5, 5), (65, 1), (130, 65), (20, 10), (70, 40), (0, 0), (2, 2), (130, 65))
PATTERN = ("converged", "empty", "converged", "converged", "converged", "inactive", "converged", "mixed", "aged", "kept", "empty", "mixed", "converged")
MIXED = (SL.CONVERGED, SL.UPDATED, SL.AGED, SL.CONVERGED, SL.NOT_VISIBLE, SL.NAN, SL.NO_MATCH, SL.CONVERGED, SL.CONVERGED, SL.UPDATED, SL.AGED)
f32 = np.float32


def status_of(pattern, j, k=0):
    if pattern == "converged":
        return SL.CONVERGED
    if pattern == "aged":
        return SL.AGED
    if pattern == "kept":
        return (SL.NOT_VISIBLE, SL.NO_MATCH, SL.UPDATED)[(j + k) % 3]
    return MIXED[(j * 7 + k) % len(MIXED)]                            # 7 and 11 are coprime: every status, interleaved in a round and across rounds


def seeds_of(rng, new, statuses, counter=COUNTER):
    """seed lists whose features are the records' observations; a seed that the rows call aged has a batch id older than MAX_N_KFS"""
    par = lambda: f32(rng.uniform(0.05, 20.0))
    seeds = dict(pt=[], seg=[], batch_counter=counter)
    for j, (p, st) in enumerate(zip(new["pt"], statuses["pt"])):
        o = p["obs"]
        seeds["pt"].append(dict(ref_kf=o["kf"], batch_id=counter - (MAX_N_KFS + 1 + j % 2 if st == SL.AGED else j % (MAX_N_KFS + 1)), px=list(o["px"]), f=list(o["f"]),
                                level=o["level"], type=o["type"], grad=list(o["grad"]), a=par(), b=par(), mu=par(), z_range=par(), sigma2=par()))
    for j, (q, st) in enumerate(zip(new["seg"], statuses["seg"])):
        o = q["obs"]
        mid = [(a + b) / 2 for a, b in zip(o["sf"], o["ef"])]
        nrm = float(np.sqrt(sum(v * v for v in mid)))
        seeds["seg"].append(dict(ref_kf=o["kf"], batch_id=counter - (MAX_N_KFS + 1 + j % 2 if st == SL.AGED else j % (MAX_N_KFS + 1)),
                                 px=[(a + b) / 2 for a, b in zip(o["spx"], o["epx"])], f=[v / nrm for v in mid], sf=list(o["sf"]), ef=list(o["ef"]), spx=list(o["spx"]),
                                 epx=list(o["epx"]), level=o["level"], a=par(), b=par(), mu_s=par(), mu_e=par(), z_range_s=par(), z_range_e=par(), sigma2_s=par(), sigma2_e=par()))
    return seeds


def rows_of(rng, new, statuses, seeds):
    """constructed shadow rows: what the update launch would leave -- the status, the new parameters (the old ones where the body does not
    touch them), the position a converged seed becomes a landmark at"""
    par = lambda: f32(rng.uniform(0.05, 20.0))
    rows = dict(pt=[], seg=[])
    for p, st, sd in zip(new["pt"], statuses["pt"], seeds["pt"]):
        same = st in (SL.AGED, SL.NOT_VISIBLE)
        rows["pt"].append(dict(status=st, xyz=list(p["pos"]) if st == SL.CONVERGED else [0.0] * 3, **{k: sd[k] if same else par() for k in SL.PT_PARAMS}))
    for q, st, sd in zip(new["seg"], statuses["seg"], seeds["seg"]):
        same = st in (SL.AGED, SL.NOT_VISIBLE)
        conv = st == SL.CONVERGED
        rows["seg"].append(dict(status=st, xyz_s=list(q["spos"]) if conv else [0.0] * 3, xyz_e=list(q["epos"]) if conv else [0.0] * 3,
                                **{k: sd[k] if same else par() for k in SL.SEG_PARAMS}))
    return rows


def make_case(rng, s, st, n_pt, n_seg, pattern, k=0):
    """the case of one stream on the tables `st` as they stand: seeds, rows, and the matcher's verdict on the landmarks that will be new"""
    if not st["kf_T"]:
        n_pt = n_seg = 0                                              # a map without keyframes has nothing to refer a seed to
    new, _, _ = Nc.make_new(rng, s, st, n_pt, n_seg)
    statuses = dict(pt=[status_of(pattern, j, k) for j in range(n_pt)], seg=[status_of(pattern, j, k + 3) for j in range(n_seg)])
    seeds = seeds_of(rng, new, statuses)
    rows = rows_of(rng, new, statuses, seeds)
    n_cp, n_cs = statuses["pt"].count(SL.CONVERGED), statuses["seg"].count(SL.CONVERGED)
    found_pt = {len(st["pt_pos"]) + j: int(j % 4 != 3) for j in range(n_cp)}
    found_seg = {len(st["seg_spos"]) + j: (int(j % 5 != 4), int(j % 7 != 6)) for j in range(n_cs)}
    return dict(s, seeds=seeds, rows=rows, active=pattern != "inactive", pattern=pattern, found_pt={**s["found_pt"], **found_pt}, found_seg={**s["found_seg"], **found_seg})


@functools.lru_cache(maxsize=None)
def batch():
    """thirteen unequal streams (four workgroups of four waves, the last one partial) with their seed lists and constructed rows"""
    rng = np.random.default_rng(7201)
    return tuple(make_case(rng, s, s["st"], n_pt, n_seg, pat) for s, (n_pt, n_seg), pat in zip(Nc.batch(), SEEDS, PATTERN))


def room_of(st, lm_reserve=LM_RESERVE, reserve=RESERVE):
    """the room of a stream's map tables as the device checks it: the staged sizes plus the reserves in force at the stage"""
    z = Ic.sizes(st)
    return dict(rows_pt=len(st["pt_pos"]) + lm_reserve.get("extra_pt", 0), rows_seg=len(st["seg_spos"]) + lm_reserve.get("extra_seg", 0),
                rows_pt_cand=z["n_pt_cand"] + lm_reserve.get("extra_pt", 0), rows_seg_cand=z["n_seg_cand"] + lm_reserve.get("extra_seg", 0),
                cap_pt_obs=z["n_pt_obs"] + reserve.get("extra_pt_obs", 0), cap_seg_obs=z["n_seg_obs"] + reserve.get("extra_seg_obs", 0))


def commit(case, seeds, st, room=None):
    """the restatement's commit of the case's rows on (seeds, st), both mutated; an inactive stream reports its sizes and changes nothing"""
    if not case["active"]:
        return SL.report_of(seeds, st), (None, None)
    return SL.commit(seeds, st, case["rows"], room)


def new_features(rng, st, s, n_pt, n_seg):
    """features of a new keyframe (the last of the table as it stands) for initializeSeeds, in np_seedlist's form"""
    if not st["kf_T"]:
        return [], []
    new, _, _ = Nc.make_new(rng, s, st, n_pt, n_seg)
    pt = [dict(p["obs"]) for p in new["pt"]]
    seg = []
    for q in new["seg"]:
        o = q["obs"]
        mid = [(a + b) / 2 for a, b in zip(o["sf"], o["ef"])]
        nrm = float(np.sqrt(sum(v * v for v in mid)))
        seg.append(dict(px=[(a + b) / 2 for a, b in zip(o["spx"], o["epx"])], f=[v / nrm for v in mid], sf=o["sf"], ef=o["ef"], spx=o["spx"], epx=o["epx"], level=o["level"]))
    return pt, seg


def kf_event_of(ev):
    """an event of np_seedlist.keyframe's arguments as capi.Context.seeds_keyframe takes it"""
    if ev is None:
        return None
    d = dict(removed_kf=ev.get("removed_kf", -1), new_batch=ev.get("new_batch", False), new_kf=ev.get("new_kf", 0), depth_mean=ev.get("depth_mean", 1.0), depth_min=ev.get("depth_min", 1.0))
    pt, seg = ev.get("new_pt", ()), ev.get("new_seg", ())
    if pt:
        d.update(pt_px=[f["px"] for f in pt], pt_f=[f["f"] for f in pt], pt_level=[f["level"] for f in pt], pt_type=[f["type"] for f in pt], pt_grad=[f["grad"] for f in pt])
    if seg:
        d.update({"seg_" + k: [f[k] for f in seg] for k in ("px", "f", "sf", "ef", "spx", "epx", "level")})
    return d
