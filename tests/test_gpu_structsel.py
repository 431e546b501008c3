"""The structure optimisation on the resident map tables on the device (plsvo_candidates_optimize_structure ..;
pl-svo_amd/csrc/structsel_device.hpp) against its restatement tests/np_structsel.py on the cases of tests/structsel_cases.py.  After
every call the positions of plsvo_candidates_fetch_map, the keys and the structure fetch are compared byte for byte, and the NEXT
plsvo_candidates_run must project with the moved positions.  The frames are driven with constructed match results
(plsvo_candidates_set_match) and, but for the resident-mask test, with constructed keep masks; the fixture and the frame driver are those
of tests/test_gpu_insert.py."""
import copy
import ctypes as C

import numpy as np
import pytest

import insert_cases as Ic
import np_structsel as NS
import select_cases as Sc
import structsel_cases as K
from test_gpu_insert import check_tables, frame, insert, stage
from test_gpu_select import same_bytes

FETCH = ("pt_lm", "pt_iters", "pt_pos", "seg_lm", "seg_iters", "seg_spos", "seg_epos")
DEFAULT = dict(max_n_pts=20, n_iter_pts=5, max_n_segs=20, n_iter_segs=5)


@pytest.fixture(scope="module")
def ctx(P):
    c = P.capi.Context(0)
    c.config_pyramids(4, Sc.CAM_T[4], Sc.CAM_T[5], 3)
    for s in range(4):
        c.build_pyramid(s, np.zeros((Sc.CAM_T[5], Sc.CAM_T[4]), np.uint8))
    yield c
    c.close()


def fresh(streams):
    return [NS.keys(copy.deepcopy(s["st"])) for s in streams]


def set_keys(ctx, sts, keys):
    """keys: per stream None or dict(pt_last_optim, seg_last_optim), into the restatement's tables and the device's"""
    for st, k in zip(sts, keys):
        if k:
            st["pt_last_optim"], st["seg_last_optim"] = list(k["pt_last_optim"]), list(k["seg_last_optim"])
    ctx.candidates_set_last_optim(keys)


def ones(sel):
    return np.ones(len(sel["pt_lm"]), np.uint8), np.ones(len(sel["seg_lm"]), np.uint8)


def check_state(ctx, sts, tag):
    check_tables(ctx, sts, tag)
    for k, (g, st) in enumerate(zip(ctx.candidates_fetch_last_optim(), sts)):
        same_bytes(g["pt_last_optim"], np.array(st["pt_last_optim"], np.int32), (tag, "keys", k, "pt"))
        same_bytes(g["seg_last_optim"], np.array(st["seg_last_optim"], np.int32), (tag, "keys", k, "seg"))


def optimize(ctx, sts, sels, masks, frame_ids, caps=DEFAULT, active=None, resident=False, tag=""):
    """the call on the device and in the restatement (which mutates sts), all compared.  masks: per stream (pt_keep, seg_keep); with
    resident = True the device reads its own masks and `masks` (from pose_fetch) go into the restatement.  Returns the restatement's reports."""
    active = [True] * len(sts) if active is None else active
    jobs = [(dict(frame_id=f) if resident else dict(frame_id=f, pt_keep=m[0], seg_keep=m[1])) if a else None for a, f, m in zip(active, frame_ids, masks)]
    ctx.candidates_optimize_structure(jobs, **caps)
    wants = [NS.optimize_structure(st, sel, m[0], m[1], f, **caps) if a else None for st, sel, m, f, a in zip(sts, sels, masks, frame_ids, active)]
    check_state(ctx, sts, tag)
    for k, (g, w) in enumerate(zip(ctx.candidates_structure_fetch(), wants)):
        if w is None:
            assert (g["n_sel_pt"], g["n_sel_seg"]) == (0, 0), (tag, k)
            continue
        assert (g["n_sel_pt"], g["n_sel_seg"]) == (len(w["pt_lm"]), len(w["seg_lm"])), (tag, k, g["n_sel_pt"], g["n_sel_seg"])
        for f in FETCH:
            same_bytes(g[f], w[f], (tag, "fetch", k, f))
    return wants


def positions(sels, chosen):
    return [int(sels["pt_lm"][i]) for i in chosen]


@pytest.mark.gpu
def test_counts_at_the_cap(ctx, P):
    """max_n = 0, fewer entries than the cap, exactly the cap, one more than the cap with distinct keys -- points and segments; every frame
    after a call projects with the moved positions (frame() compares the candidates with the restatement's on the moved tables)"""
    streams = (K.fifty(),)
    sts = fresh(streams)
    stage(ctx, sts)
    for n, (cap_pt, cap_seg) in enumerate(((0, 0), (60, 20), (50, 10), (49, 9))):
        _, _, sels = frame(ctx, P, streams, sts, tag=("caps", n))
        n_pt, n_seg = len(sels[0]["pt_lm"]), len(sels[0]["seg_lm"])
        assert (n_pt, n_seg) == (50, 10)
        set_keys(ctx, sts, [K.keys_by_feature(sts[0], sels[0], [(7 * i) % 50 - 20 for i in range(n_pt)], [(3 * i) % 10 for i in range(n_seg)])])
        w = optimize(ctx, sts, sels, [ones(sels[0])], [100 + n], dict(DEFAULT, max_n_pts=cap_pt, max_n_segs=cap_seg), tag=("caps", n))[0]
        assert (len(w["pt_lm"]), len(w["seg_lm"])) == (min(cap_pt, 50), min(cap_seg, 10))
        if cap_pt == 49:                                               # the one left out holds the largest key
            left = set(int(v) for v in sels[0]["pt_lm"]) - set(int(v) for v in w["pt_lm"])
            assert [sts[0]["pt_last_optim"][lm] for lm in left] == [max((7 * i) % 50 - 20 for i in range(50))]
    frame(ctx, P, streams, sts, tag="caps, after")


@pytest.mark.gpu
def test_ties_go_to_the_earlier_feature_across_rounds_of_64(ctx, P):
    """70 point features, the cap at 20: fifteen keys below the cut, ten at it -- four of them among features 60 .. 63, six among 64 .. 69,
    so the tie count is carried across the round of 64; then the cut inside the first round; then all keys equal (the first frame)"""
    streams = (K.seventy(),)
    sts = fresh(streams)
    stage(ctx, sts)
    cases = ((K.tie_keys(70, range(15), range(60, 70)), list(range(15)) + [60, 61, 62, 63, 64]),
             (K.tie_keys(70, range(15), range(20, 30)), list(range(15)) + [20, 21, 22, 23, 24]),
             ([4] * 70, list(range(20))))
    for n, (keys, chosen) in enumerate(cases):
        _, _, sels = frame(ctx, P, streams, sts, tag=("ties", n))
        assert len(sels[0]["pt_lm"]) == 70 and len(set(int(v) for v in sels[0]["pt_lm"])) == 70
        set_keys(ctx, sts, [K.keys_by_feature(sts[0], sels[0], keys, None)])
        w = optimize(ctx, sts, sels, [ones(sels[0])], [50 + n], tag=("ties", n))[0]
        assert [int(v) for v in w["pt_lm"]] == positions(sels[0], chosen), (n, w["pt_lm"])
    frame(ctx, P, streams, sts, tag="ties, after")


@pytest.mark.gpu
def test_keys_rotate_over_successive_frames(ctx, P):
    """three frames over 50 features with the cap at 20, frame ids negative, small and the largest int32: what frame k refined is not refined
    at k + 1 while older landmarks remain"""
    streams = (K.fifty(),)
    sts = fresh(streams)
    stage(ctx, sts)
    set_keys(ctx, sts, [dict(pt_last_optim=[K.INT_MIN] * 50, seg_last_optim=[K.INT_MIN] * 10)])
    chosen = []
    for n, fid in enumerate((-7, 3, K.INT_MAX)):
        _, _, sels = frame(ctx, P, streams, sts, tag=("rotate", n))
        w = optimize(ctx, sts, sels, [ones(sels[0])], [fid], dict(DEFAULT, max_n_segs=4), tag=("rotate", n))[0]
        chosen.append((set(int(v) for v in w["pt_lm"]), set(int(v) for v in w["seg_lm"])))
        assert all(sts[0]["pt_last_optim"][lm] == fid for lm in chosen[-1][0])
    assert len(chosen[0][0]) == len(chosen[1][0]) == len(chosen[2][0]) == 20 and not chosen[0][0] & chosen[1][0]
    rest = set(range(50)) - chosen[0][0] - chosen[1][0]
    assert len(rest) == 10 and rest <= chosen[2][0] and chosen[2][0] - rest <= chosen[0][0]      # the ten never refined, then the oldest
    assert not chosen[0][1] & chosen[1][1] and len(chosen[0][1] | chosen[1][1] | chosen[2][1]) == 10
    frame(ctx, P, streams, sts, tag="rotate, after")


def doubles(sel):
    """{segment landmark: its two feature positions} of the segments that are a feature twice"""
    at = {}
    for i, lm in enumerate(sel["seg_lm"]):
        at.setdefault(int(lm), []).append(i)
    return {lm: v for lm, v in at.items() if len(v) == 2}


@pytest.mark.gpu
def test_a_doubly_won_segment_runs_twice_or_once_under_the_cap(ctx, P):
    streams = (K.seventy(),)
    sts = fresh(streams)
    stage(ctx, sts)
    _, _, sels = frame(ctx, P, streams, sts, tag="double 1")
    two = doubles(sels[0])
    assert len(two) == 2 and len(sels[0]["seg_lm"]) == 14
    # both instances selected, one iteration per run: the second entry's run starts from the first's result (its report differs from the first's)
    w = optimize(ctx, sts, sels, [ones(sels[0])], [11], dict(DEFAULT, n_iter_segs=1), tag="double, both")[0]
    for lm, (i, j) in two.items():
        assert int(w["seg_lm"][i]) == int(w["seg_lm"][j]) == lm and sts[0]["seg_spos"][lm] == [float(v) for v in w["seg_spos"][j]]
    assert all(not np.array_equal(w["seg_spos"][i], w["seg_spos"][j]) and w["seg_iters"][i] == w["seg_iters"][j] == 1 for i, j in two.values())
    # only one instance fits: the doubled landmark A holds the smallest key and the cap is 1; then A, A and the first instance of B under a cap of 3
    (a, _), (b, _) = sorted(two.items(), key=lambda kv: kv[1][0])
    for n, (cap, want) in enumerate(((1, [a]), (3, [a, a, b]))):
        _, _, sels = frame(ctx, P, streams, sts, tag=("double", cap))
        keys = [1 if int(lm) == a else 2 if int(lm) == b else 9 for lm in sels[0]["seg_lm"]]
        set_keys(ctx, sts, [K.keys_by_feature(sts[0], sels[0], None, keys)])
        w = optimize(ctx, sts, sels, [ones(sels[0])], [12 + n], dict(DEFAULT, max_n_segs=cap), tag=("double", cap))[0]
        assert [int(v) for v in w["seg_lm"]] == want
    frame(ctx, P, streams, sts, tag="double, after")


@pytest.mark.gpu
def test_host_masks_drop_features(ctx, P):
    """every third point feature and the SECOND instance of a doubly won segment are masked out: they are not in the deque"""
    streams = (K.seventy(),)
    sts = fresh(streams)
    stage(ctx, sts)
    _, _, sels = frame(ctx, P, streams, sts, tag="masks")
    pk, sk = ones(sels[0])
    pk[::3] = 0
    (lm, (i, j)), = list(doubles(sels[0]).items())[:1]
    sk[j] = 0
    w = optimize(ctx, sts, sels, [(pk, sk)], [21], dict(DEFAULT, max_n_pts=64), tag="masks")[0]
    assert [int(v) for v in w["pt_lm"]] == [int(v) for k, v in enumerate(sels[0]["pt_lm"]) if k % 3] and list(w["seg_lm"]).count(lm) == 1
    frame(ctx, P, streams, sts, tag="masks, after")


@pytest.mark.gpu
def test_resident_masks_behind_the_pose_optimiser(ctx, P):
    """NULL masks: the call reads the keep masks plsvo_candidates_pose_optimize left on the device (every seventh match is six pixels off
    and is culled); the masks of pose_fetch go into the restatement"""
    streams = K.batch()
    sts = fresh(streams)
    stage(ctx, sts)
    _, got, sels = frame(ctx, P, streams, sts, tag="resident", outliers=True)
    ctx.candidates_pose_optimize()
    po = ctx.candidates_pose_fetch([(g["n_matches"], g["n_ls_matches"]) for g in got])
    masks = [(p.pt_keep, p.seg_keep) for p in po]
    assert sum(int(m[0].sum()) for m in masks) > 30 and any(0 in m[0] for m in masks)                   # kept and rejected features
    optimize(ctx, sts, sels, masks, [5, 6, 7, 8], dict(DEFAULT, max_n_pts=64), resident=True, tag="resident")
    frame(ctx, P, streams, sts, tag="resident, after")


@pytest.mark.gpu
def test_observation_counts_and_a_landmark_at_depth_zero(ctx, P):
    """one observation (a rank-2 system), twelve observations, and a landmark at depth 0 in one keyframe: dp is NaN, the reference rolls
    back, the position is unchanged -- and the key is still written (src/frame_handler_base.cpp:221)"""
    streams = (K.observations(),)
    sts = fresh(streams)
    stage(ctx, sts)
    _, _, sels = frame(ctx, P, streams, sts, tag="observations")
    d0 = streams[0]["depth0"]
    assert [len(sts[0]["pt_obs"][lm]) for lm in (0, 1, d0)] == [1, 12, 3] and set(int(v) for v in sels[0]["pt_lm"]) >= {0, 1, d0}
    before = list(sts[0]["pt_pos"][d0])
    w = optimize(ctx, sts, sels, [ones(sels[0])], [31], dict(DEFAULT, max_n_pts=30, max_n_segs=10), tag="observations")[0]
    at = [int(v) for v in w["pt_lm"]].index(d0)
    assert sts[0]["pt_pos"][d0] == before and int(w["pt_iters"][at]) == 1 and sts[0]["pt_last_optim"][d0] == 31
    assert sum(1 for lm, p in zip(w["pt_lm"], w["pt_pos"]) if list(p) != list(streams[0]["st"]["pt_pos"][int(lm)])) > 15    # the others moved
    frame(ctx, P, streams, sts, tag="observations, after")


@pytest.mark.gpu
def test_a_batch_with_an_inactive_stream_equals_the_gathered_job(ctx, P):
    """four streams with different counts, one inactive (its tables and keys are untouched), one without features; and for the batch the
    in-place result equals plsvo_structure_optimize on the gathered job, bit for bit"""
    streams = K.batch()
    sts = fresh(streams)
    stage(ctx, sts)
    _, _, sels = frame(ctx, P, streams, sts, tag="batch")
    assert len(sels[2]["pt_lm"]) == len(sels[2]["seg_lm"]) == 0
    before = copy.deepcopy(sts)
    active = [True, False, True, True]
    wants = optimize(ctx, sts, sels, [ones(s) for s in sels], [41, 42, 43, 44], active=active, tag="batch")
    assert sts[1]["pt_pos"] == before[1]["pt_pos"] and sts[1]["pt_last_optim"] == before[1]["pt_last_optim"]
    assert (len(wants[2]["pt_lm"]), len(wants[2]["seg_lm"])) == (0, 0) and len(wants[3]["seg_lm"]) == 20 and len(wants[0]["pt_lm"]) == 20
    for k in (0, 3):
        pts, segs = [int(v) for v in wants[k]["pt_lm"]], [int(v) for v in wants[k]["seg_lm"]]
        once = [lm for lm in segs if segs.count(lm) == 1]
        r = ctx.structure_optimize(P.structopt_job_from_batch(NS.gathered_job(before[k], pts, once)))
        same_bytes(r["pt_pos"], np.array([sts[k]["pt_pos"][lm] for lm in pts]).reshape(-1, 3), ("gathered", k, "pt_pos"))
        same_bytes(r["seg_spos"], np.array([sts[k]["seg_spos"][lm] for lm in once]).reshape(-1, 3), ("gathered", k, "seg_spos"))
        same_bytes(r["seg_epos"], np.array([sts[k]["seg_epos"][lm] for lm in once]).reshape(-1, 3), ("gathered", k, "seg_epos"))
        same_bytes(r["pt_iters"], wants[k]["pt_iters"], ("gathered", k, "pt_iters"))
    frame(ctx, P, streams, sts, tag="batch, after")


@pytest.mark.gpu
def test_lifetime_of_the_key_column(ctx, P):
    """a set / fetch round trip returns what was set; an insertion with a removal behind the call on the same run yields the tables of
    np_insert and leaves the keys alone; rows appended by plsvo_candidates_add read 0"""
    streams = (K.fifty(), K.seventy())
    sts = fresh(streams)
    ctx.candidates_reserve_landmarks(extra_pt=3, extra_seg=2)
    try:
        stage(ctx, sts)
    finally:
        ctx.candidates_reserve_landmarks()
    rng = np.random.default_rng(7200)
    set_keys(ctx, sts, [dict(pt_last_optim=rng.integers(K.INT_MIN, K.INT_MAX, len(st["pt_pos"]), endpoint=True), seg_last_optim=rng.integers(-9, 9, len(st["seg_spos"])))
                        for st in sts])
    check_state(ctx, sts, "round trip")
    ctx.candidates_set_last_optim([dict(seg_last_optim=[3] * len(sts[0]["seg_spos"])), None])              # a missing array is left alone
    sts[0]["seg_last_optim"] = [3] * len(sts[0]["seg_spos"])
    check_state(ctx, sts, "one array")
    _, _, sels = frame(ctx, P, streams, sts, tag="lifetime")
    masks = [Ic.keep_masks(s, sel) for s, sel in zip(streams, sels)]
    optimize(ctx, sts, sels, masks, [61, 62], tag="lifetime")
    insert(ctx, streams, sts, sels, [True, True], [1, 0], masks=masks, tag="insertion behind the call")
    check_state(ctx, sts, "keys behind the insertion")
    n_pt = len(sts[0]["pt_pos"])
    new = dict(pt_pos=[[0.1, 0.2, 4.0], [0.3, -0.1, 3.0]], pt_obs_kf=[0, 1], pt_obs_px=[[100.0, 90.0], [120.0, 80.0]], pt_obs_f=[[0.0, 0.0, 1.0], [0.1, 0.0, 0.99]],
               pt_obs_level=[0, 1], pt_obs_type=[0, 0])
    ctx.candidates_add([new, None])
    got = ctx.candidates_fetch_last_optim()
    assert len(got[0]["pt_last_optim"]) == n_pt + 2 and list(got[0]["pt_last_optim"][n_pt:]) == [0, 0]
    same_bytes(got[0]["pt_last_optim"][:n_pt], np.array(sts[0]["pt_last_optim"], np.int32), "keys behind the add")
    same_bytes(got[1]["seg_last_optim"], np.array(sts[1]["seg_last_optim"], np.int32), "keys behind the add, other stream")


@pytest.mark.gpu
def test_structsel_error_paths(ctx, P):
    L, h, A = ctx.L, ctx.h, P.abi
    streams = (K.fifty(), K.seventy())
    sts = fresh(streams)
    stage(ctx, sts)
    pr = A.CandStructOptParams(20, 5, 20, 5)
    jobs = (A.CandStructOpt * 2)()
    for j in jobs:
        j.active, j.frame_id = 1, 9
    outs = (A.CandStructOptOut * 2)()
    assert L.plsvo_candidates_structure_fetch(h, 2, outs) == A.E_STATE                                   # no call since the stage
    assert L.plsvo_candidates_optimize_structure(h, 2, jobs, C.byref(pr)) == A.E_STATE                   # no run
    ctx.candidates_run([A.CandidateFrameJob(s["T"], s["overlap"], cur_slot=0) for s in streams])
    assert L.plsvo_candidates_optimize_structure(h, 2, jobs, C.byref(pr)) == A.E_STATE                   # no selection
    want_c = [Sc.restate_candidates(s, st) for s, st in zip(streams, sts)]
    ctx.candidates_set_match([Sc.match_of(s, r) for s, r in zip(streams, want_c)])
    ctx.candidates_select(**Ic.PARAMS)
    before = (ctx.candidates_fetch_map(), ctx.candidates_fetch_last_optim(), ctx.candidates_fetch_quality())
    assert L.plsvo_candidates_optimize_structure(h, 2, jobs, C.byref(pr)) == A.E_STATE                   # NULL masks, no resident pose optimisation
    keep = np.ones(400, np.uint8)
    jobs[1].pt_keep = jobs[1].seg_keep = keep.ctypes.data_as(A.c_u8_p)
    assert L.plsvo_candidates_optimize_structure(h, 2, jobs, C.byref(pr)) == A.E_STATE                   # ... of stream 0
    jobs[0].pt_keep = jobs[0].seg_keep = keep.ctypes.data_as(A.c_u8_p)
    assert L.plsvo_candidates_optimize_structure(h, 1, jobs, C.byref(pr)) == A.E_INVALID and L.plsvo_candidates_optimize_structure(h, 3, jobs, C.byref(pr)) == A.E_INVALID
    assert L.plsvo_candidates_optimize_structure(h, 2, None, C.byref(pr)) == A.E_INVALID and L.plsvo_candidates_optimize_structure(h, 2, jobs, None) == A.E_INVALID
    for field in ("max_n_pts", "n_iter_pts", "max_n_segs", "n_iter_segs"):
        bad = A.CandStructOptParams(20, 5, 20, 5)
        setattr(bad, field, -1)
        assert L.plsvo_candidates_optimize_structure(h, 2, jobs, C.byref(bad)) == A.E_INVALID, field
    assert L.plsvo_candidates_set_last_optim(h, 1, (A.CandLastOptimIn * 2)()) == A.E_INVALID and L.plsvo_candidates_set_last_optim(h, 2, None) == A.E_INVALID
    assert L.plsvo_candidates_fetch_last_optim(h, 3, (A.CandLastOptimOut * 3)()) == A.E_INVALID and L.plsvo_candidates_fetch_last_optim(h, 2, None) == A.E_INVALID
    assert L.plsvo_candidates_structure_fetch(h, 2, outs) == A.E_STATE                                   # (none of them counted as a call)
    after = (ctx.candidates_fetch_map(), ctx.candidates_fetch_last_optim(), ctx.candidates_fetch_quality())
    for a, b in zip(before[0] + before[1] + before[2], after[0] + after[1] + after[2]):
        for f in a:
            same_bytes(b[f], a[f], ("unchanged", f))
    # the call itself, once; a second one on the same run is refused (the keys have moved on) and changes nothing
    jobs[1].active = 0
    assert L.plsvo_candidates_optimize_structure(h, 2, jobs, C.byref(pr)) == A.OK
    assert L.plsvo_candidates_structure_fetch(h, 1, outs) == A.E_INVALID and L.plsvo_candidates_structure_fetch(h, 2, None) == A.E_INVALID
    # the fetch with the caller's own buffers: one entry short of what a stream selected is refused whole (the counts are reported, no
    # buffer is written); NULL buffers need no capacity; buffers of exactly the selected size are filled and nothing behind them
    lm = [np.full(21, -9, np.int32), np.full(11, -9, np.int32)]
    pos = np.full((21, 3), -9.0)
    outs[0].pt_lm, outs[0].pt_pos, outs[0].seg_lm = lm[0].ctypes.data_as(A.c_i32_p), pos.ctypes.data_as(A.c_double_p), lm[1].ctypes.data_as(A.c_i32_p)
    for cap_pt, cap_seg in ((19, 10), (20, 9), (0, 0), (-1, 10)):
        outs[0].cap_pt, outs[0].cap_seg = cap_pt, cap_seg
        assert L.plsvo_candidates_structure_fetch(h, 2, outs) == A.E_INVALID, (cap_pt, cap_seg)
        assert (outs[0].n_sel_pt, outs[0].n_sel_seg, outs[1].n_sel_pt) == (20, 10, 0) and (lm[0] == -9).all() and (lm[1] == -9).all() and (pos == -9.0).all()
    outs[0].cap_pt, outs[0].cap_seg = 20, 10
    assert L.plsvo_candidates_structure_fetch(h, 2, outs) == A.OK
    assert (lm[0][:20] >= 0).all() and lm[0][20] == -9 and (lm[1][:10] >= 0).all() and lm[1][10] == -9 and (pos[:20] != -9.0).all() and (pos[20] == -9.0).all()
    assert L.plsvo_candidates_structure_fetch(h, 2, (A.CandStructOptOut * 2)()) == A.OK                  # NULL buffers, capacity 0: the counts alone
    rep = ctx.candidates_structure_fetch()
    same_bytes(rep[0]["pt_lm"], lm[0][:20], "the wrapper's fetch"); same_bytes(rep[0]["pt_pos"], pos[:20], "the wrapper's fetch")
    assert (rep[0]["n_sel_pt"], rep[0]["n_sel_seg"], rep[1]["n_sel_pt"], rep[1]["n_sel_seg"]) == (20, 10, 0, 0)
    once = (ctx.candidates_fetch_map(), ctx.candidates_fetch_last_optim())
    assert list(once[1][0]["pt_last_optim"]).count(9) == 20 and not np.array_equal(once[0][0]["pt_pos"], before[0][0]["pt_pos"])
    assert L.plsvo_candidates_optimize_structure(h, 2, jobs, C.byref(pr)) == A.E_STATE
    # behind an insertion the run is closed
    ins = (A.CandInsert * 2)()
    for a in ins:
        a.is_kf, a.remove_kf, a.kf_slot, a.pt_keep, a.seg_keep = 1, -1, 1, keep.ctypes.data_as(A.c_u8_p), keep.ctypes.data_as(A.c_u8_p)
    ctx.candidates_run([A.CandidateFrameJob(s["T"], s["overlap"], cur_slot=0) for s in streams])
    ctx.candidates_set_match([Sc.match_of(s, r) for s, r in zip(streams, ctx.candidates_fetch())])
    ctx.candidates_select(**Ic.PARAMS)
    assert L.plsvo_candidates_insert_keyframe(h, 2, ins) == A.OK
    twice = (ctx.candidates_fetch_map(), ctx.candidates_fetch_last_optim())
    assert L.plsvo_candidates_optimize_structure(h, 2, jobs, C.byref(pr)) == A.E_STATE
    again = (ctx.candidates_fetch_map(), ctx.candidates_fetch_last_optim())
    for a, b in zip(twice[0] + twice[1], again[0] + again[1]):
        for f in a:
            same_bytes(b[f], a[f], ("closed run", f))
    assert ctx.candidates_structure_fetch()[0]["n_sel_pt"] == 20                                         # the last report can still be fetched


@pytest.mark.gpu
def test_an_unfetched_seed_update_refuses_the_call_and_committed_rows_read_zero(P):
    """between plsvo_seeds_update (here: the diagnostic commit of constructed rows) and plsvo_seeds_update_fetch the tables' sizes are the
    device's alone: the call and the key accessors return PLSVO_E_STATE; behind the fetch the landmark rows the commit appended read 0"""
    import np_seedlist as SL
    import seedlist_cases as Sl
    from test_gpu_seedlist import N_SLOTS, fresh as fresh_seeds, stage as stage_seeds
    A = P.abi
    ctx = P.capi.Context(0)
    try:
        ctx.config_pyramids(N_SLOTS, Sc.CAM_T[4], Sc.CAM_T[5], 3)
        for s in range(N_SLOTS):
            ctx.build_pyramid(s, np.zeros((Sc.CAM_T[5], Sc.CAM_T[4]), np.uint8))
        L, h = ctx.L, ctx.h
        cases = Sl.batch()[4:7]
        sts, seeds = fresh_seeds(cases)
        stage_seeds(ctx, sts, seeds)
        n_before = [len(st["pt_pos"]) for st in sts]
        ctx.candidates_set_last_optim([dict(pt_last_optim=[5] * n) for n in n_before])
        ctx.candidates_run([A.CandidateFrameJob(s["T"], s["overlap"], cur_slot=0) for s in cases])
        ctx.candidates_set_match([Ic.frame(s, st)[1] for s, st in zip(cases, sts)])
        ctx.candidates_select(**Ic.PARAMS)
        ctx.seeds_commit_rows([SL.rows_of(c["rows"]) for c in cases])
        keep = np.ones(400, np.uint8)
        jobs = (A.CandStructOpt * 3)()
        for j in jobs:
            j.active, j.frame_id, j.pt_keep, j.seg_keep = 1, 9, keep.ctypes.data_as(A.c_u8_p), keep.ctypes.data_as(A.c_u8_p)
        pr = A.CandStructOptParams(20, 5, 20, 5)
        assert L.plsvo_candidates_optimize_structure(h, 3, jobs, C.byref(pr)) == A.E_STATE
        assert L.plsvo_candidates_set_last_optim(h, 3, (A.CandLastOptimIn * 3)()) == A.E_STATE
        assert L.plsvo_candidates_fetch_last_optim(h, 3, (A.CandLastOptimOut * 3)()) == A.E_STATE
        reps = ctx.seeds_update_fetch()
        assert sum(r["n_pt"] - n for r, n in zip(reps, n_before)) > 0                                    # converged seeds became landmarks
        assert L.plsvo_candidates_optimize_structure(h, 3, jobs, C.byref(pr)) == A.E_STATE               # the update ended the open run, as an add does
        for g, r, n in zip(ctx.candidates_fetch_last_optim(), reps, n_before):
            assert list(g["pt_last_optim"]) == [5] * n + [0] * (r["n_pt"] - n)
            assert not g["seg_last_optim"].any()
    finally:
        ctx.close()
