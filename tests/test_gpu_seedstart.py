"""A keyframe's point seeds started on the device from its FAST corners (plsvo_seeds_keyframe_detect / _keyframe_fetch;
pl-svo_amd/csrc/seedlist_device.hpp: seeds_occupancy_kernel, seeds_start_kernel; detect_device.hpp through a slot table) against their
restatement tests/np_seedstart.py.  Everything is compared byte for byte through plsvo_seeds_fetch_lists, the report and
plsvo_seeds_capacity: the detector's scores are integers or uncontracted doubles, the bearing is uncontracted double arithmetic, the rest
is copied.  The pyramids the NumPy side reads are the slot's own levels, downloaded.  Images stay at 160 x 120 (or the 320 x 240
three-image sequence of tests/test_gpu_seedlist.py) so that the emulated run (tests/test_emu_seedstart.py) takes them too; the name of the
one 640 x 480 case contains `full_size`."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest

import candidates_cases as Cc
import np_fast as F
import np_seedlist as SL
import np_seedstart as SS
from test_gpu_detect import _device_buffer, _noise, _scene
from test_gpu_newcand import set_quality
from test_gpu_seedlist import _image_case, check_lists
from test_gpu_select import same_bytes

pytestmark = pytest.mark.gpu

W, H = 160, 120
CAM = (210.0, 190.0, 80.25, 60.5, W, H)                 # fx != fy, fractional principal point
REPORT = ("n_new_pt", "n_new_seg", "n_pt_seeds", "n_seg_seeds", "batch_counter", "no_room", "n_occupied", "reserved0")
f32 = np.float32


@pytest.fixture
def ctx(P):
    c = P.capi.Context(0)
    yield c
    c.close()


def load(ctx, imgs, n_levels=3):
    h, w = imgs[0].shape
    ctx.config_pyramids(len(imgs), w, h, n_levels)
    for i, im in enumerate(imgs):
        ctx.build_pyramid(i, im)
    return [ctx.download_pyramid(i) for i in range(len(imgs))]


def tables(kf_slots):
    """a stream's map tables: keyframes in the given pyramid slots, no landmark"""
    st = Cc.empty_stream([Cc.IDENT] * len(kf_slots))
    st.update(kf_slot=list(kf_slots), pt_nfail=[], pt_nsucc=[], seg_nfail=[], seg_nsucc=[])
    return st


def line_features(rng, n, w=W, h=H):
    out = []
    for _ in range(n):
        v = lambda k: [float(x) for x in rng.uniform(-1, 1, k)]
        out.append(dict(px=[float(rng.uniform(0, w)), float(rng.uniform(0, h))], f=v(3), sf=v(3), ef=v(3), spx=v(2), epx=v(2), level=int(rng.integers(0, 3))))
    return out


def old_seeds(rng, n_pt, n_seg, n_kf, counter=5, w=W, h=H):
    """lists a stream holds beforehand: seeds of every keyframe of its table, of the last batches"""
    sd = dict(pt=[], seg=[], batch_counter=counter)
    for i in range(n_pt):
        ftr = dict(px=[float(rng.uniform(0, w)), float(rng.uniform(0, h))], f=[float(x) for x in rng.uniform(-1, 1, 3)], level=int(rng.integers(0, 3)), type=0, grad=[1.0, 0.0])
        sd["pt"].append(SL.new_point_seed(ftr, i % n_kf, counter - i % 3, 2.0 + i / 16, 0.5 + i / 32))
    for i, ftr in enumerate(line_features(rng, n_seg, w, h)):
        sd["seg"].append(SL.new_line_seed(ftr, (i + 1) % n_kf, counter - i % 2, 3.0 + i / 16, 0.75))
    return sd


def stage(ctx, sts, seeds, cam=CAM, extra_pt=0, extra_seg=0, lm_room=0):
    ctx.candidates_reserve(extra_pt_obs=lm_room, extra_seg_obs=lm_room)
    ctx.candidates_reserve_landmarks(extra_pt=lm_room, extra_seg=lm_room)
    ctx.candidates_stage([Cc.to_job(st) for st in sts], cam, 30, 40, 8)
    set_quality(ctx, sts)
    ctx.seeds_reserve(extra_pt=extra_pt, extra_seg=extra_seg)
    ctx.seeds_stage([SL.lists_of(sd) for sd in seeds], cam, max_n_kfs=3)


def seg_arrays(new_seg):
    return {"seg_" + k: [f[k] for f in new_seg] for k in ("px", "f", "sf", "ef", "spx", "epx", "level")} if new_seg else {}


def dev_event(e, d_occupancy=None, occ_sources=0):
    """an event of np_seedstart.keyframe_detect's arguments as capi.Context.seeds_keyframe_detect takes it"""
    if e is None:
        return None
    return dict(removed_kf=e.get("removed_kf", -1), new_batch=e.get("new_batch", False), new_kf=e.get("new_kf", 0), depth_mean=e.get("depth_mean", 1.0),
                depth_min=e.get("depth_min", 1.0), occ_sources=occ_sources, d_occupancy=d_occupancy, **seg_arrays(e.get("new_seg", ())))


def upload(occ):
    """caller-made occupancy rows [n, cells] in device memory -> (keep-alive, pointer of row 0)"""
    occ = np.ascontiguousarray(occ, np.uint8)
    keep, ptr, _ = _device_buffer(occ.size)
    if isinstance(keep, np.ndarray):
        keep[:] = occ.ravel()
    else:
        import torch
        keep.copy_(torch.from_numpy(occ.ravel()))
        torch.cuda.synchronize()
    return keep, ptr


def check_reports(got, want, tag):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        if w is not None:
            assert {f: g[f] for f in REPORT} == {f: w[f] for f in REPORT}, (tag, k, g, w)


ZERO = dict.fromkeys(REPORT, 0)


def test_rounds_of_64_sources_and_destinations_on_both_sides_of_a_round(ctx):
    """eight streams share one slot; the caller's occupancy cuts their new seeds to 0, 1, 63, 64, 65, 128, 129 and 192 of the 192 cells
    that all hold a corner; their lists hold 0, 1, 63, 64 and 65 seeds beforehand.  A ninth event with cell 8: 298 of 300 cells, five
    rounds, the last partial"""
    lv = load(ctx, [_scene(3), _noise(21)])[1]
    assert len(F.detect(lv, 10, 20, 20.0)) == 192 and len(F.detect(lv, 8, 20, 20.0)) == 298      # conditions on the inputs
    rng = np.random.default_rng(9101)
    new, old = (0, 1, 63, 64, 65, 128, 129, 192), (0, 1, 63, 64, 65, 65, 0, 1)
    occ = np.zeros((8, 192), np.uint8)
    for row, k in zip(occ, new):
        row[rng.permutation(192)[:192 - k]] = 1 + rng.integers(0, 255, 192 - k)                      # (any non-zero byte is "occupied")
    sts = [tables([0, 1]) for _ in new]
    seeds = [old_seeds(rng, n, n // 2, 2) for n in old]
    stage(ctx, sts, seeds, extra_pt=192, extra_seg=4)
    keep, ptr = upload(occ)
    events = [dict(new_batch=bool(k % 2), new_kf=1, depth_mean=2.0 + k, depth_min=0.5 + k / 4, new_seg=line_features(rng, k % 3)) for k in range(8)]
    ctx.seeds_keyframe_detect([dev_event(e, ptr + 192 * k) for k, e in enumerate(events)], cell_size=10)
    want = [SS.keyframe_detect(sd, lv, CAM, 10, caller=o, **e) for sd, o, e in zip(seeds, occ, events)]
    assert [r["n_new_pt"] for r in want] == list(new) and [r["n_occupied"] for r in want] == [192 - k for k in new]
    check_reports(ctx.seeds_keyframe_fetch(), want, "rounds")
    check_lists(ctx, seeds, "rounds")
    # cell 8 on one stream alone: 300 cells
    sts, seeds = [tables([1])], [old_seeds(rng, 63, 2, 1)]
    stage(ctx, sts, seeds, extra_pt=300)
    ctx.seeds_keyframe_detect([dict(new_kf=0, depth_mean=1.5, depth_min=0.25, occ_sources=0)], cell_size=8)
    want = [SS.keyframe_detect(seeds[0], lv, CAM, 8, new_kf=0, depth_mean=1.5, depth_min=0.25)]
    assert want[0]["n_new_pt"] == 298
    check_reports(ctx.seeds_keyframe_fetch(), want, "cell 8")
    check_lists(ctx, seeds, "cell 8")


def test_levels_and_bearing_on_a_size_the_cell_does_not_divide(ctx, P):
    """157 x 93 with cell 25: the last column and row of cells are partial; corners of levels 1 and 2 are among the new seeds; the camera
    has fx != fy and a fractional principal point; the new rows equal sequence.seeds_from_corners' on the device's own corners"""
    seqm = importlib.import_module("pl-svo_amd.sequence")
    cam = (143.5, 151.25, 77.75, 45.125, 157, 93)
    lvs = load(ctx, [_scene(23, 157, 93), _scene(30, 157, 93)])
    sts, seeds = [tables([0]), tables([1, 0])], [dict(pt=[], seg=[], batch_counter=0), dict(pt=[], seg=[], batch_counter=2)]
    stage(ctx, sts, seeds, cam, extra_pt=28)
    ctx.seeds_keyframe_detect([dict(new_kf=0, new_batch=True, depth_mean=2.5, depth_min=0.7, occ_sources=0), dict(new_kf=0, depth_mean=1.25, depth_min=0.3, occ_sources=0)])
    want = [SS.keyframe_detect(seeds[0], lvs[0], cam, 25, new_kf=0, new_batch=True, depth_mean=2.5, depth_min=0.7),
            SS.keyframe_detect(seeds[1], lvs[1], cam, 25, new_kf=0, depth_mean=1.25, depth_min=0.3)]
    levels = [x["level"] for sd in seeds for x in sd["pt"]]
    assert 1 in levels and 2 in levels and 0 in levels
    cells = [F.cell_index(7, 25, *x["px"]) for sd in seeds for x in sd["pt"]]
    assert any(c % 7 == 6 for c in cells) and any(c // 7 == 3 for c in cells)                       # seeds of the partial column and row
    check_reports(ctx.seeds_keyframe_fetch(), want, "levels")
    check_lists(ctx, seeds, "levels")
    got = ctx.seeds_fetch_lists()
    for k, (slot, dm, dmin) in enumerate(((0, 2.5, 0.7), (1, 1.25, 0.3))):
        host = seqm.seeds_from_corners(ctx.detect_fast(slot, 1)[0], cam, dm, dmin)
        for f in ("px", "f", "level", "type", "grad", "a", "b", "mu", "z_range", "sigma2"):
            same_bytes(got[k]["pt_" + f], host[f], ("seeds_from_corners", k, f))


# ---- occupancy sources ------------------------------------------------------------------------------------------------------------------------
CAM_S = (128.0, 128.0, 78.5, 46.5, 157, 93)
# (projected pixel, matched pixel): the matched one is the feature's.  Multiples of the cell exactly, just below one, the last partial
# cell (column 6 and row 3 of 7 x 4), which the pose optimiser culls: its match lies 12 pixels from its projection
SELECTED = (((50.0, 25.0), (50.0, 25.0)), ((74.5, 60.0), (74.99999, 60.0)), ((110.0, 49.5), (110.0, 49.99999)), ((20.0, 70.0), (20.0, 70.0)), ((130.0, 20.0), (130.0, 20.0)),
            ((85.0, 30.0), (85.0, 30.0)), ((140.0, 80.0), (152.0, 88.0)), ((30.0, 45.0), (30.0, 45.0)), ((100.0, 80.0), (100.0, 80.0)))


def selected_stream():
    st = tables([0])
    for i, ((px, py), _) in enumerate(SELECTED):
        z = 2.0 + i / 4
        pos = [(px - CAM_S[2]) / CAM_S[0] * z, (py - CAM_S[3]) / CAM_S[1] * z, z]
        n = float(np.sqrt(sum(v * v for v in pos)))
        Cc.add_pt(st, pos, 3, [dict(kf=0, px=[px, py], f=[v / n for v in pos], level=0, type=0, grad=[1.0, 0.0])])
        st["kf_pt"][0].append(i)
    st.update(pt_nfail=[0] * len(SELECTED), pt_nsucc=[0] * len(SELECTED))
    return st


def run_selection(ctx, P, n):
    """a frame at the keyframe's pose whose matches are SELECTED's -> the features the selection wrote (with the culled one among them)"""
    ctx.candidates_run([P.abi.CandidateFrameJob(Cc.IDENT, (0,), cur_slot=0) for _ in range(n)])
    cand = ctx.candidates_fetch()
    match = []
    for c in cand:
        assert c["n_filed_pt"] == len(SELECTED) and c["n_filed_seg"] == 0
        match.append(dict(found=np.ones(len(SELECTED), np.uint8), px=[SELECTED[lm][1] for lm in c["pt_lm"]], search_level=np.zeros(len(SELECTED), np.int32)))
    ctx.candidates_set_match(match)
    ctx.candidates_select()
    sel = ctx.candidates_select_fetch()
    ctx.candidates_pose_optimize()
    pose = ctx.candidates_pose_fetch([(g["n_matches"], g["n_ls_matches"]) for g in sel])
    for g, p in zip(sel, pose):
        assert g["n_matches"] == len(SELECTED)
        culled = [tuple(px) for px, k in zip(g["pt_px"].tolist(), p.pt_keep) if not k]
        assert (152.0, 88.0) in culled                                 # the reference leaves a culled feature in pt_fts_: it still marks its cell
    return sel


def test_selected_features_mark_their_cells_culled_ones_included(ctx, P):
    lvs = load(ctx, [_scene(23, 157, 93)])
    sts, seeds = [selected_stream(), selected_stream()], [dict(pt=[], seg=[], batch_counter=1), dict(pt=[], seg=[], batch_counter=1)]
    stage(ctx, sts, seeds, CAM_S, extra_pt=28)
    sel = run_selection(ctx, P, 2)
    px = sel[0]["pt_px"]
    cells = {F.cell_index(7, 25, x, y) for x, y in px.tolist()}
    assert {1 * 7 + 2, 2 * 7 + 2, 1 * 7 + 4, 3 * 7 + 6} <= cells   # (50, 25) -> (2, 1); (74.99999, 60) -> column 2, not 3; (110, 49.99999) -> row 1, not 2; the last partial cell
    free = SS.keyframe_detect(copy.deepcopy(seeds[0]), lvs[0], CAM_S, 25, new_kf=0)
    ctx.seeds_keyframe_detect([dict(new_kf=0, depth_mean=2.0, depth_min=1.0, occ_sources=P.abi.SEED_OCC_SELECTED), dict(new_kf=0, depth_mean=2.0, depth_min=1.0, occ_sources=0)])
    want = [SS.keyframe_detect(seeds[0], lvs[0], CAM_S, 25, new_kf=0, depth_mean=2.0, depth_min=1.0, selected_px=px),
            SS.keyframe_detect(seeds[1], lvs[0], CAM_S, 25, new_kf=0, depth_mean=2.0, depth_min=1.0)]
    assert want[0]["n_occupied"] == len(cells) and want[0]["n_new_pt"] < free["n_new_pt"] == want[1]["n_new_pt"]   # the source alone took seeds away
    check_reports(ctx.seeds_keyframe_fetch(), want, "selected")
    check_lists(ctx, seeds, "selected")


def _updated_case(P, ob, ctx, prepare=None):
    """the three-image sequence of tests/test_gpu_seedlist.py, staged, updated with frame 2 and fetched; prepare(seq, sts) may add
    landmarks to the tables before they are staged"""
    seq, sts, seeds, active = _image_case(P, ob)
    cam = tuple(seq["cam"])
    if prepare:
        prepare(seq, sts)
    ctx.config_pyramids(3, 320, 240, 4)
    for k, im in enumerate(seq["images"]):
        ctx.build_pyramid(k, im, 0)
    stage(ctx, sts, seeds, cam, extra_pt=260, extra_seg=4, lm_room=100)
    ctx.seeds_update([dict(cur_slot=2, T_f_w=[float(v) for v in seq["poses_true"][2]]) if a else None for a in active])
    reps = ctx.seeds_update_fetch()
    return seq, cam, sts, active, reps


DET = dict(fast_threshold=7, detection_threshold=2.0)    # the rendered plane of the sequence is soft: the reference's thresholds find no corner in it


def seeds_now(ls):
    """fetched lists as np_seedlist's seeds"""
    return [dict(pt=[dict(ref_kf=int(l["pt_ref_kf"][i]), batch_id=int(l["pt_batch_id"][i]), px=l["pt_px"][i].tolist(), f=l["pt_f"][i].tolist(), level=int(l["pt_level"][i]),
                          type=int(l["pt_type"][i]), grad=l["pt_grad"][i].tolist(), **{k: l["pt_" + k][i] for k in ("a", "b", "mu", "z_range", "sigma2")}) for i in range(len(l["pt_ref_kf"]))],
                 seg=[dict(ref_kf=int(l["seg_ref_kf"][i]), batch_id=int(l["seg_batch_id"][i]), level=int(l["seg_level"][i]),
                           **{k: l["seg_" + k][i].tolist() for k in ("px", "f", "sf", "ef", "spx", "epx")},
                           **{k: l["seg_" + k][i] for k in ("a", "b", "mu_s", "mu_e", "z_range_s", "z_range_e", "sigma2_s", "sigma2_e")}) for i in range(len(l["seg_ref_kf"]))],
                 batch_counter=l["batch_counter"]) for l in ls]


def test_rows_of_the_last_update_mark_their_cells_by_status(ctx, P, ob):
    """shadow rows of a real update on the three-image sequence: UPDATED and CONVERGED rows mark the cell of their px_cur, NOT_VISIBLE,
    NO_MATCH and AGED rows mark nothing.  A NAN row of a POINT seed cannot come out of a real update: z_inv_min is NaN only with a NaN
    variance, whose epipolar segment is NaN, so the search fails first and the row is NO_MATCH (update_point_seed).  The second half
    therefore writes the statuses through plsvo_seeds_commit_rows, which uploads statuses and no px_cur: the rows then hold the px_cur
    the REAL update left -- a NAN row among the marking ones, and NO_MATCH, NOT_VISIBLE and AGED rows whose left-over px_cur lies in a
    cell that otherwise gets a seed (the case the issue asks for can be built, and is)"""
    seq, cam, sts, active, reps = _updated_case(P, ob, ctx)
    assert not any(r["no_room"] for r in reps)
    rows = ctx.seeds_fetch_rows()
    st0 = rows[0]["pt_status"]
    assert all((st0 == s).any() for s in (SL.UPDATED, SL.CONVERGED, SL.NOT_VISIBLE, SL.NO_MATCH, SL.AGED))
    seeds = seeds_now(ctx.seeds_fetch_lists())
    new_kf = [1, 0, 0, 1]                                              # the keyframe in slot 1 where the table has one
    ev = [dict(new_kf=k, depth_mean=2.0, depth_min=1.0) if a else None for k, a in zip(new_kf, active)]
    levels = [ctx.download_pyramid(st["kf_slot"][k])[:3] for st, k in zip(sts, new_kf)]
    ctx.seeds_keyframe_detect([dev_event(e, occ_sources=P.abi.SEED_OCC_UPDATED) for e in ev], **DET)
    want = [SS.keyframe_detect(sd, l, cam, 25, update_rows=(r["pt_status"], r["pt_px_cur"]), **e, **DET) if e else None for sd, l, r, e in zip(seeds, levels, rows, ev)]
    assert want[0]["n_occupied"] >= 10 and want[0]["n_new_pt"] > 20 and want[2]["n_occupied"] == 0   # (stream 2 holds line seeds only)
    check_reports(ctx.seeds_keyframe_fetch(), want, "updated")
    check_lists(ctx, seeds, "updated")
    # -- statuses written over the px_cur that the real update left
    lv = levels[0]
    n0, n_real = len(seeds[0]["pt"]), len(st0)
    px_left = rows[0]["pt_px_cur"]
    free_cells = {F.cell_index(13, 25, float(c["x"]), float(c["y"])) for c in F.detect(lv, 25, 7, 2.0)}
    by_cell = {}
    for j in range(min(n0, n_real)):
        if SS.marks(320, 240, px_left[j]) and px_left[j].any() and F.cell_index(13, 25, *px_left[j]) in free_cells:
            by_cell.setdefault(F.cell_index(13, 25, *px_left[j]), []).append(j)
    assert len(by_cell) >= 6, "too few px_cur of the real update lie in cells that get a seed"
    chosen = dict(zip((SL.NO_MATCH, SL.AGED, SL.NOT_VISIBLE, SL.UPDATED, SL.CONVERGED, SL.NAN), list(by_cell.items())[:6]))
    status = np.full(n0, SL.NO_MATCH, np.int32)
    for stt, (cell, js) in chosen.items():
        status[js] = stt
    ns = len(seeds[0]["seg"])
    commit = [dict(pt_status=status, **{"pt_" + k: [x[k] for x in seeds[0]["pt"]] for k in ("a", "b", "mu", "sigma2")}, pt_xyz_world=np.ones((n0, 3)),
                   seg_status=np.full(ns, SL.NO_MATCH, np.int32), **{"seg_" + k: [x[k] for x in seeds[0]["seg"]] for k in ("a", "b", "mu_s", "mu_e", "sigma2_s", "sigma2_e")},
                   seg_xyz_world_s=np.zeros((ns, 3)), seg_xyz_world_e=np.zeros((ns, 3))), None, None, None]
    ctx.seeds_commit_rows(commit)
    assert ctx.seeds_update_fetch()[0]["no_room"] == 0
    rows2 = ctx.seeds_fetch_rows()[0]
    same_bytes(rows2["pt_px_cur"][:n_real], px_left[:n0], "commit_rows leaves px_cur as the real update wrote it")
    same_bytes(rows2["pt_status"], status, "statuses")
    seeds = seeds_now(ctx.seeds_fetch_lists())                         # (the commit itself is tests/test_gpu_seedlist.py's subject)
    n1 = len(seeds[0]["pt"])
    ctx.seeds_keyframe_detect([dict(new_kf=1, new_batch=True, depth_mean=2.0, depth_min=1.0, occ_sources=P.abi.SEED_OCC_UPDATED), None, None, None], **DET)
    w = SS.keyframe_detect(seeds[0], lv, cam, 25, new_kf=1, new_batch=True, depth_mean=2.0, depth_min=1.0, update_rows=(rows2["pt_status"], rows2["pt_px_cur"]), **DET)
    got_cells = {F.cell_index(13, 25, *x["px"]) for x in seeds[0]["pt"][n1:]}
    assert all(x["batch_id"] == seeds[0]["batch_counter"] for x in seeds[0]["pt"][n1:])
    assert all(chosen[s][0] in got_cells for s in (SL.NO_MATCH, SL.AGED, SL.NOT_VISIBLE)), "a status that must not mark kept a seed out of its cell"
    assert not any(chosen[s][0] in got_cells for s in (SL.UPDATED, SL.CONVERGED, SL.NAN)), "a marking status let a seed into its cell"
    check_reports(ctx.seeds_keyframe_fetch()[:1], [w], "left px_cur")
    check_lists(ctx, seeds, "left px_cur")


LANDMARK_PX = ((60.0, 50.0), (110.0, 70.0), (160.0, 95.0), (215.0, 120.0), (260.0, 150.0), (90.0, 180.0), (190.0, 190.0), (135.0, 140.0))
MATCH_PX = ((62.0, 52.0), (112.5, 74.99999), (150.0, 100.0), (212.0, 118.0), (263.0, 151.0), (88.0, 183.0), (193.0, 188.0), (137.0, 141.0))


def _add_landmarks(seq, sts):
    """eight landmarks on the scene plane's depth, observed in the keyframe that is frame 0, in streams 0 and 1"""
    fx, fy, cx, cy = [float(v) for v in seq["cam"][:4]]
    T0 = [float(v) for v in seq["poses_true"][0]]
    z = float(seq["stream"].plane_d / seq["stream"].plane_n[2])
    for st in sts[:2]:
        kf = [i for i, T in enumerate(st["kf_T"]) if T == T0][0]
        for px, py in LANDMARK_PX:
            c = [(px - cx) / fx * z, (py - cy) / fy * z, z]
            n = float(np.sqrt(sum(v * v for v in c)))
            lm = Cc.add_pt(st, Cc.K.se3_act(Cc.K.se3_inv(T0), c), 3, [dict(kf=kf, px=[px, py], f=[v / n for v in c], level=0, type=0, grad=[1.0, 0.0])])
            st["kf_pt"][kf].append(lm)
        st.update(pt_nfail=[0] * len(LANDMARK_PX), pt_nsucc=[0] * len(LANDMARK_PX))


def test_all_three_sources_together(ctx, P, ob):
    """the caller's bytes, the features of a real selection on the same context (matches placed through plsvo_candidates_set_match) and
    the rows of a real update, in one event: every source marks at least one cell that neither of the other two marks"""
    seq, cam, sts, active, reps = _updated_case(P, ob, ctx, _add_landmarks)
    rows, lists = ctx.seeds_fetch_rows(), ctx.seeds_fetch_lists()
    ctx.candidates_run([P.abi.CandidateFrameJob([float(v) for v in seq["poses_true"][2]], tuple(range(len(st["kf_T"]))), cur_slot=2) for st in sts])
    cand = ctx.candidates_fetch()
    match = []
    for k, c in enumerate(cand):
        lms = [int(v) for v in c["pt_lm"]]                           # (the seeds the update converged are filed as the map's candidates: not matched here)
        mine = [lm < len(MATCH_PX) for lm in lms]
        assert sum(mine) >= 6 if k < 2 else not lms, (k, lms)
        n_e = c["n_filed_pt"] + 2 * c["n_filed_seg"]
        found = np.zeros(n_e, np.uint8)
        found[:len(lms)] = mine
        match.append(dict(found=found, px=[MATCH_PX[lm] if m else (0.0, 0.0) for lm, m in zip(lms, mine)] + [(0.0, 0.0)] * (n_e - len(lms)), search_level=np.zeros(n_e, np.int32)))
    ctx.candidates_set_match(match)
    ctx.candidates_select()
    sel = ctx.candidates_select_fetch()
    assert sel[0]["n_matches"] >= 6 and sel[1]["n_matches"] >= 6
    cell = lambda px: F.cell_index(13, 25, float(px[0]), float(px[1]))
    rng = np.random.default_rng(9103)
    occ = np.zeros((4, 130), np.uint8)
    alone = []
    for k in range(2):
        S = {cell(p) for p in sel[k]["pt_px"]}
        U = {cell(p) for s_, p in zip(rows[k]["pt_status"], rows[k]["pt_px_cur"]) if int(s_) in SS.MARKING and SS.marks(320, 240, p)}
        assert S - U and U - S, (k, S, U)
        mine = [c for c in rng.permutation(130) if c not in S | U][:30]
        occ[k, mine] = 1
        occ[k, sorted(S & U)[:1] + sorted(S - U)[1:2]] = 1            # (overlaps with the other sources as well)
        C_ = set(np.nonzero(occ[k])[0].tolist())
        alone.append((C_ - S - U, S - C_ - U, U - C_ - S))
        assert all(alone[-1]), (k, alone[-1])                          # each source marks a cell the other two do not
    keep, ptr = upload(occ)
    lv = ctx.download_pyramid(1)[:3]
    both = P.abi.SEED_OCC_SELECTED | P.abi.SEED_OCC_UPDATED
    ctx.seeds_keyframe_detect([dict(new_kf=st["kf_slot"].index(1) if 1 in st["kf_slot"] else 0, depth_mean=2.0, depth_min=1.0, occ_sources=both, d_occupancy=ptr + 130 * k) if k < 2 else None
                               for k, st in enumerate(sts)], **DET)
    got = ctx.seeds_fetch_lists()
    rep = ctx.seeds_keyframe_fetch()
    free = {cell((c["x"], c["y"])) for c in F.detect(lv, 25, 7, 2.0)}
    for k in range(2):
        n_old = len(lists[k]["pt_ref_kf"])
        o = SS.occupancy(320, 240, 25, occ[k], sel[k]["pt_px"], (rows[k]["pt_status"], rows[k]["pt_px_cur"]))
        want = SS.corner_features(F.detect(lv, 25, 7, 2.0, o), cam)
        assert len(want) > 10 and rep[k]["n_occupied"] == sum(o)
        got_cells = {cell(p) for p in got[k]["pt_px"][n_old:]}
        assert all((src & free) and not (src & got_cells) for src in alone[k]), (k, "a source alone did not keep seeds out of a cell that holds a corner")
        same_bytes(got[k]["pt_px"][n_old:], [x["px"] for x in want], ("all sources", k, "px"))
        same_bytes(got[k]["pt_f"][n_old:], [x["f"] for x in want], ("all sources", k, "f"))
        same_bytes(got[k]["pt_level"][n_old:], [x["level"] for x in want], ("all sources", k, "level"))
        for f in lists[k]:
            if f != "batch_counter":
                same_bytes(got[k][f][:len(lists[k][f])], lists[k][f], ("all sources", k, f, "old rows"))
    assert rep[2] == ZERO and rep[3] == ZERO


# ---- room ---------------------------------------------------------------------------------------------------------------------------------------
def test_room_is_decided_on_the_device_all_or_nothing(ctx):
    """exact room commits; one row short flags the stream, applies its removal and its counter and appends nothing of either kind; its
    neighbours commit; the detector's keys are left armed; after a restage with room the repeated event gives the restatement's lists"""
    lv = load(ctx, [_noise(21)])[0]
    n_new = len(F.detect(lv, 25, 20, 20.0))
    assert n_new > 20
    rng = np.random.default_rng(9104)
    for short in (0, 1):
        sts = [tables([0, 0, 0]) for _ in range(3)]
        seeds = [old_seeds(rng, 9, 4, 3), old_seeds(rng, 12, 4, 3), old_seeds(rng, 3, 0, 3)]
        gone = sum(x["ref_kf"] == 1 for x in seeds[1]["pt"])
        assert gone == 4
        stage(ctx, sts, seeds, extra_pt=n_new - gone - short, extra_seg=2)     # stream 1: 12 - 4 + n_new rows needed, 12 + extra laid out
        lim = [c["pt"] for c in ctx.seeds_capacity()]
        assert lim == [len(sd["pt"]) + n_new - gone - short for sd in seeds]
        events = [dict(new_kf=2, new_batch=True, depth_mean=2.0, depth_min=1.0, new_seg=line_features(rng, 1)) if k != 1 else
                  dict(removed_kf=1, new_kf=1, new_batch=True, depth_mean=3.0, depth_min=1.5, new_seg=line_features(rng, 2)) for k in range(3)]
        occ = np.zeros((3, 35), np.uint8)
        occ[0, :gone + 1] = 1                                          # the neighbours need fewer rows than stream 1
        occ[2, ::2] = 1
        keep, ptr = upload(occ)
        ctx.seeds_keyframe_detect([dev_event(e, ptr + 35 * k) for k, e in enumerate(events)])
        want = [SS.keyframe_detect(sd, lv, CAM, 25, lim_pt=l, caller=o, **e) for sd, l, o, e in zip(seeds, lim, occ, events)]
        assert [r["no_room"] for r in want] == [0, short, 0]
        got = ctx.detect_fast(0, 1)[0]                                 # directly behind: the keys were left armed, also by the short stream
        assert got.tobytes() == F.detect(lv, 25, 20, 20.0).tobytes()
        check_reports(ctx.seeds_keyframe_fetch(), want, ("room", short))
        check_lists(ctx, seeds, ("room", short))
        if short:
            assert want[1]["n_new_pt"] == 0 and want[1]["n_new_seg"] == 0 and want[1]["n_pt_seeds"] == 12 - gone and want[1]["batch_counter"] == 6
            assert all(x["ref_kf"] != 2 for x in seeds[1]["pt"] + seeds[1]["seg"])                  # the table closed up
            stage(ctx, sts, seeds, extra_pt=n_new, extra_seg=2)
            again = [None, dict(events[1], removed_kf=-1, new_batch=False), None]
            ctx.seeds_keyframe_detect([dev_event(e, ptr + 35 * k) for k, e in enumerate(again)])
            w = SS.keyframe_detect(seeds[1], lv, CAM, 25, caller=occ[1], **again[1])
            assert w["no_room"] == 0 and w["n_new_pt"] == n_new
            check_reports(ctx.seeds_keyframe_fetch(), [ZERO, w, ZERO], "repeated")
            check_lists(ctx, seeds, "repeated")


# ---- the whole event against the host path ---------------------------------------------------------------------------------------------------
def test_the_whole_event_equals_the_host_path_on_a_twin_context(ctx, P):
    """removal of the first, a middle, the last and no keyframe, a new batch, the detection and uploaded line seeds in one call, against
    detect_fast -> seeds_from_corners -> plsvo_seeds_keyframe on a second context with the same tables"""
    seqm = importlib.import_module("pl-svo_amd.sequence")
    twin = P.capi.Context(0)
    try:
        imgs = [_scene(22), _noise(21), _scene(24)]
        lvs = load(ctx, imgs)
        load(twin, imgs)
        rng = np.random.default_rng(9105)
        removed = (0, 2, 4, -1)
        sts = [tables([2, 0, 1, 2, 1]) for _ in removed]
        seeds = [old_seeds(rng, 70, 9, 5) for _ in removed]
        occ = (rng.random((4, 35)) < 0.25).astype(np.uint8)
        stage(ctx, sts, seeds, extra_pt=35, extra_seg=3)
        stage(twin, sts, seeds, extra_pt=35, extra_seg=3)
        events = [dict(removed_kf=r, new_batch=True, new_kf=3 if r >= 0 else 4, depth_mean=2.0 + k, depth_min=0.5 + k, new_seg=line_features(rng, 3)) for k, r in enumerate(removed)]
        slots = [2 if r >= 0 else 1 for r in removed]                  # (tables [2, 0, 1, 2, 1]: row 3 and row 4)
        keep, ptr = upload(occ)
        ctx.seeds_keyframe_detect([dev_event(e, ptr + 35 * k) for k, e in enumerate(events)])
        host = []
        for k, (e, slot) in enumerate(zip(events, slots)):
            sd = seqm.seeds_from_corners(twin.detect_fast(slot, 1, occupancy=occ[k:k + 1])[0], CAM, e["depth_mean"], e["depth_min"])
            host.append(dict(removed_kf=e["removed_kf"], new_batch=True, new_kf=e["new_kf"], depth_mean=e["depth_mean"], depth_min=e["depth_min"],
                             **{"pt_" + f: sd[f] for f in ("px", "f", "level", "type", "grad")}, **seg_arrays(e["new_seg"])))
        twin.seeds_keyframe(host)
        a, b = ctx.seeds_fetch_lists(), twin.seeds_fetch_lists()
        for k in range(4):
            assert a[k]["batch_counter"] == b[k]["batch_counter"] == 6
            for f in a[k]:
                if f != "batch_counter":
                    same_bytes(a[k][f], b[k][f], ("twin", k, f))
        want = [SS.keyframe_detect(sd, lvs[slot], CAM, 25, caller=o, **e) for sd, slot, o, e in zip(seeds, slots, occ, events)]
        assert all(r["n_new_pt"] > 5 for r in want) and any(len(sd["pt"]) - r["n_new_pt"] < 70 for sd, r in zip(seeds, want))
        check_reports(ctx.seeds_keyframe_fetch(), want, "twin")
        check_lists(ctx, seeds, "twin")
    finally:
        twin.close()


# ---- subsets and slots -------------------------------------------------------------------------------------------------------------------------
def test_subsets_slots_and_one_stream_at_a_time(ctx):
    """keyframe slots 2, 0, 2, 1 across the four active streams of six; inactive streams are untouched in rows, counts and report; every
    stream alone equals its place in the batch"""
    lvs = load(ctx, [_scene(22), _noise(21), _scene(24)])
    rng = np.random.default_rng(9106)
    kf_slots = ([1, 2], [0], [0, 1], [0, 2, 1], [2, 1, 1], [1])
    new_kf = (1, 0, None, 1, 2, None)
    assert [s[k] for s, k in zip(kf_slots, new_kf) if k is not None] == [2, 0, 2, 1]
    sts = [tables(s) for s in kf_slots]
    seeds = [old_seeds(rng, 5 + 13 * k, k, len(s)) for k, s in enumerate(kf_slots)]
    first = copy.deepcopy(seeds)
    events = [dict(new_kf=k, new_batch=bool(i % 2), removed_kf=0 if i == 3 else -1, depth_mean=1.5 + i, depth_min=0.5, new_seg=line_features(rng, i % 2)) if k is not None else None
              for i, k in enumerate(new_kf)]
    stage(ctx, sts, seeds, extra_pt=35, extra_seg=2)
    before = ctx.seeds_fetch_lists()
    ctx.seeds_keyframe_detect([dev_event(e) for e in events])
    want = [SS.keyframe_detect(sd, lvs[s[e["new_kf"]]], CAM, 25, **e) if e else ZERO for sd, s, e in zip(seeds, kf_slots, events)]
    reports = ctx.seeds_keyframe_fetch()
    check_reports(reports, want, "subset")
    check_lists(ctx, seeds, "subset")
    whole = ctx.seeds_fetch_lists()
    for k in (2, 5):
        for f in before[k]:
            if f != "batch_counter":
                same_bytes(whole[k][f], before[k][f], ("inactive", k, f))
    assert len({tuple(map(tuple, w["pt_px"][-5:])) for w in (whole[0], whole[1], whole[4])}) == 3   # three different images were read
    for k in (0, 3, 4):
        stage(ctx, [sts[k]], [first[k]], extra_pt=35, extra_seg=2)
        ctx.seeds_keyframe_detect([dev_event(events[k])])
        assert ctx.seeds_keyframe_fetch()[0] == reports[k]
        alone = ctx.seeds_fetch_lists()[0]
        for f in alone:
            if f != "batch_counter":
                same_bytes(alone[f], whole[k][f], ("alone", k, f))


# ---- the rows are live ------------------------------------------------------------------------------------------------------------------------
def test_the_next_update_runs_on_the_new_rows(ctx, P, ob):
    """the next plsvo_seeds_update on the following image leaves, in the new seeds' shadow rows, what plsvo_update_seeds leaves for the
    same seeds (keyframe in slot 1, frame in slot 2)"""
    seq, cam, sts, active, reps = _updated_case(P, ob, ctx)
    before, rows0 = ctx.seeds_fetch_lists(), ctx.seeds_fetch_rows()[0]
    d0 = float(seq["stream"].plane_d / seq["stream"].plane_n[2])
    ctx.seeds_keyframe_detect([dict(new_kf=1, new_batch=True, depth_mean=d0, depth_min=0.5 * d0, occ_sources=P.abi.SEED_OCC_UPDATED), None, None, None], **DET)
    T2 = [float(v) for v in seq["poses_true"][2]]
    ctx.seeds_update([dict(cur_slot=2, T_f_w=T2), None, None, None])   # straight on: neither fetch in between
    rep = ctx.seeds_update_fetch()[0]
    kf = ctx.seeds_keyframe_fetch()[0]                                 # behind the update fetch: a copy, no wait
    rows = ctx.seeds_fetch_rows()[0]
    n_old, n_new = len(before[0]["pt_ref_kf"]), kf["n_new_pt"]
    assert n_new > 20 and sum(rep["pt"]) == n_old + n_new == len(rows["pt_status"])
    lv = ctx.download_pyramid(1)[:3]
    new = SS.corner_features(F.detect(lv, 25, 7, 2.0, SS.occupancy(320, 240, 25, None, None, (rows0["pt_status"], rows0["pt_px_cur"]))), cam)
    assert len(new) == n_new
    z_range = f32(1.0 / float(f32(0.5 * d0)))
    pt = dict(ref_frame=np.full(n_new, 1, np.int32), cur_frame=np.full(n_new, 2, np.int32), px=np.array([x["px"] for x in new]), f=np.array([x["f"] for x in new]),
              level=np.array([x["level"] for x in new], np.int32), type=np.zeros(n_new, np.uint8), grad=np.tile([1.0, 0.0], (n_new, 1)), a=np.full(n_new, 10, f32), b=np.full(n_new, 10, f32),
              mu=np.full(n_new, f32(1.0 / float(f32(d0))), f32), z_range=np.full(n_new, z_range, f32), sigma2=np.full(n_new, f32(z_range * z_range) / f32(36), f32))
    rd = ctx.update_seeds(P.abi.SeedsJob(seq["cam"], seq["poses_true"], np.arange(3), pt, None))
    assert (rd["pt_status"] == SL.UPDATED).sum() + (rd["pt_status"] == SL.CONVERGED).sum() >= 3
    for f in ("pt_status", "pt_a", "pt_b", "pt_mu", "pt_sigma2", "pt_xyz_world", "pt_px_cur", "pt_depth"):
        same_bytes(rows[f][n_old:], rd[f], ("live rows", f))


# ---- protocol --------------------------------------------------------------------------------------------------------------------------------------
def test_protocol_and_error_paths_write_nothing(ctx, P):
    L, h, A = ctx.L, ctx.h, P.abi
    lv = load(ctx, [_noise(21), _scene(22)])[0]
    rng = np.random.default_rng(9108)
    pr = A.detect_params()
    ev = (A.SeedKfDetect * 2)()
    for a in ev:
        a.active, a.removed_kf, a.new_kf, a.depth_mean, a.depth_min = 1, -1, 0, 2.0, 1.0
    call = lambda: L.plsvo_seeds_keyframe_detect(h, 2, C.byref(pr), ev)
    assert call() == A.E_STATE and L.plsvo_seeds_keyframe_fetch(h, 2, (A.SeedKfReport * 2)()) == A.E_STATE          # no staged seed tables
    sts, seeds = [tables([0, 1]), tables([1])], [old_seeds(rng, 7, 3, 2), old_seeds(rng, 4, 2, 1)]
    stage(ctx, sts, seeds, extra_pt=35, extra_seg=1)
    assert L.plsvo_seeds_keyframe_fetch(h, 2, (A.SeedKfReport * 2)()) == A.E_STATE                                  # no event yet
    assert L.plsvo_seeds_keyframe_detect(h, 1, C.byref(pr), ev) == A.E_INVALID and L.plsvo_seeds_keyframe_detect(h, 2, C.byref(pr), None) == A.E_INVALID
    assert L.plsvo_seeds_keyframe_detect(h, 2, None, ev) == A.E_INVALID
    for f, v in (("cell_size", 0), ("n_levels", 0), ("n_levels", 4), ("fast_threshold", 0), ("fast_threshold", 255), ("detection_threshold", -1.0), ("detection_threshold", 0.1),
                 ("detection_threshold", float("nan"))):
        old = getattr(pr, f)
        setattr(pr, f, v)
        assert call() == A.E_INVALID, (f, v)
        setattr(pr, f, old)
    segs = line_features(rng, 2)
    keepalive = {k: np.ascontiguousarray(v, np.int32 if k == "seg_level" else np.float64) for k, v in seg_arrays(segs).items()}

    def with_segs(a, n, drop=None):
        a.n_seg = n
        for k, v in keepalive.items():
            setattr(a, k, None if k == drop else v.ctypes.data_as(A.c_i32_p if k == "seg_level" else A.c_double_p))
    for f, v, code in (("new_kf", 2, A.E_INVALID), ("new_kf", -1, A.E_INVALID), ("occ_sources", 4, A.E_INVALID), ("occ_sources", -1, A.E_INVALID), ("depth_mean", 0.0, A.E_INVALID),
                       ("depth_min", -1.0, A.E_INVALID), ("removed_kf", -2, A.E_INVALID), ("removed_kf", 3, A.E_INVALID), ("n_seg", -1, A.E_INVALID), ("n_seg", 1, A.E_INVALID),
                       ("occ_sources", A.SEED_OCC_SELECTED, A.E_STATE), ("occ_sources", A.SEED_OCC_UPDATED, A.E_STATE)):
        old = getattr(ev[0], f)
        setattr(ev[0], f, v)
        assert call() == code, (f, v)
        setattr(ev[0], f, old)
    for drop in keepalive:                                             # a NULL segment array with a count
        with_segs(ev[1], 1, drop)
        assert call() == A.E_INVALID, drop
    bad = keepalive["seg_level"].copy()
    keepalive["seg_level"][0] = 3
    with_segs(ev[1], 1)
    assert call() == A.E_INVALID                                        # a segment level outside the pyramid
    keepalive["seg_level"][:] = bad
    with_segs(ev[1], 2)
    assert call() == A.E_CAPACITY                                       # two line seeds, one row of room: decided on the host, nothing written
    with_segs(ev[1], 0)
    # a keyframe whose slot lies outside the pyramids
    ctx.config_pyramids(1, W, H, 3)
    ctx.build_pyramid(0, _noise(21))
    ev[0].new_kf = 1
    assert call() == A.E_INVALID
    ev[0].new_kf = 0
    ev[1].active = 0
    load(ctx, [_noise(21), _scene(22)])
    check_lists(ctx, seeds, "refused events")
    got = ctx.detect_fast(0, 1)[0]
    assert got.tobytes() == F.detect(lv, 25, 20, 20.0).tobytes()       # the keys are as they were
    assert call() == A.OK                                               # (stream 0 alone, keyframe 0 in slot 0)
    want = SS.keyframe_detect(seeds[0], lv, CAM, 25, new_kf=0, depth_mean=2.0, depth_min=1.0)
    check_reports(ctx.seeds_keyframe_fetch(), [want, ZERO], "accepted")
    check_lists(ctx, seeds, "accepted")
    # behind an unfetched update the tables are the device's alone
    ctx.seeds_update([dict(cur_slot=0, T_f_w=Cc.IDENT), None])
    assert call() == A.E_STATE and L.plsvo_seeds_keyframe_fetch(h, 2, (A.SeedKfReport * 2)()) == A.E_STATE
    ctx.seeds_update_fetch()
    ev[0].occ_sources = A.SEED_OCC_UPDATED
    assert call() == A.OK                                               # a fetched update: the source is there now
    # a candidate restage drops the seed tables and the reports with them
    ctx.candidates_stage([Cc.to_job(st) for st in sts], CAM, 30, 40, 8)
    assert call() == A.E_STATE and L.plsvo_seeds_keyframe_fetch(h, 2, (A.SeedKfReport * 2)()) == A.E_STATE


# ---- full size -----------------------------------------------------------------------------------------------------------------------------------
def test_full_size_640x480_cell_25_four_streams(ctx):
    cam = (420.0, 415.0, 319.5, 239.5, 640, 480)
    lvs = load(ctx, [_scene(31, 640, 480), _scene(32, 640, 480)])
    rng = np.random.default_rng(9109)
    sts = [tables([0, 1]), tables([1, 0]), tables([1]), tables([0])]
    slots = (1, 1, 1, 0)
    new_kf = (1, 0, 0, 0)
    seeds = [old_seeds(rng, n, 3, len(st["kf_T"]), w=640, h=480) for n, st in zip((0, 200, 63, 130), sts)]
    occ = np.zeros((4, 520), np.uint8)
    occ[1] = rng.random(520) < 0.5
    occ[3, ::3] = 1
    stage(ctx, sts, seeds, cam, extra_pt=520, extra_seg=2)
    keep, ptr = upload(occ)
    events = [dict(new_kf=k, new_batch=True, removed_kf=-1 if i else 0, depth_mean=2.0, depth_min=1.0, new_seg=line_features(rng, 2, 640, 480)) for i, k in enumerate(new_kf)]
    ctx.seeds_keyframe_detect([dev_event(e, ptr + 520 * k) for k, e in enumerate(events)])
    free = {s: F.detect(lvs[s], 25, 20, 20.0) for s in set(slots)}

    def restate(sd, s, o, e):
        """np_seedstart.keyframe_detect with the detection of the unoccupied grid shared between the streams of a slot: a cell's record
        does not depend on the other cells' occupancy (np_fast.detect decides every cell from its own survivors)"""
        SL.keyframe(sd, removed_kf=e["removed_kf"], new_batch=e["new_batch"])
        new = SS.corner_features([c for c in free[s] if not o[F.cell_index(26, 25, float(c["x"]), float(c["y"]))]], cam)
        SL.keyframe(sd, new_kf=e["new_kf"], depth_mean=e["depth_mean"], depth_min=e["depth_min"], new_pt=new, new_seg=e["new_seg"])
        return dict(ZERO, n_new_pt=len(new), n_new_seg=2, n_pt_seeds=len(sd["pt"]), n_seg_seeds=len(sd["seg"]), batch_counter=sd["batch_counter"], n_occupied=int(o.sum()))
    want = [restate(sd, s, o, e) for sd, s, o, e in zip(seeds, slots, occ, events)]
    one = SS.keyframe_detect(old_seeds(np.random.default_rng(1), 0, 0, 1), lvs[0], cam, 25, caller=occ[3], new_kf=0)
    assert one["n_new_pt"] == want[3]["n_new_pt"] > 100                # the shortcut above equals the restatement where it is run in full
    check_reports(ctx.seeds_keyframe_fetch(), want, "full_size")
    check_lists(ctx, seeds, "full_size")
