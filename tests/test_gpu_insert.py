"""The keyframe insertion into the resident map tables on the device (plsvo_candidates_insert_keyframe ..; pl-svo_amd/csrc/insert_device.hpp)
against its restatement tests/np_insert.py on the cases of tests/insert_cases.py.  Everything is compared byte for byte, array by array:
the stage copies what the selection wrote and its only arithmetic is the bearing of a segment's end points.  The frames are driven with
constructed match results (plsvo_candidates_set_match) and, but for the resident-mask test, with constructed keep masks."""
import copy
import ctypes as C

import numpy as np
import pytest

import candidates_cases as Cc
import insert_cases as Ic
import np_candidates as N
import np_select as S
import select_cases as Sc
from test_gpu_select import CAND_FIELDS, SEL_FIELDS, device_A, same_bytes

QUALITY = (("pt_n_failed", "pt_nfail"), ("pt_n_succeeded", "pt_nsucc"), ("pt_type", "pt_type"), ("seg_n_failed", "seg_nfail"), ("seg_n_succeeded", "seg_nsucc"),
           ("seg_type", "seg_type"), ("pt_cand", "pt_cand"), ("seg_cand", "seg_cand"))
OUT_SIZES = ("n_kf", "n_kf_pt", "n_kf_seg", "n_pt_obs", "n_seg_obs", "n_pt_cand", "n_seg_cand")


@pytest.fixture(scope="module")
def ctx(P):
    c = P.capi.Context(0)
    c.config_pyramids(4, Sc.CAM_T[4], Sc.CAM_T[5], 3)
    for s in range(4):
        c.build_pyramid(s, np.zeros((Sc.CAM_T[5], Sc.CAM_T[4]), np.uint8))
    yield c
    c.close()


def stage(ctx, sts, reserve=Ic.RESERVE):
    ctx.candidates_reserve(**reserve)
    ctx.candidates_stage([Cc.to_job(st) for st in sts], Ic.CAM, Ic.CELL, Ic.SEG_CELL, Ic.BOUNDARY)
    ctx.candidates_set_quality([dict(pt_n_failed=st["pt_nfail"], pt_n_succeeded=st["pt_nsucc"], seg_n_failed=st["seg_nfail"], seg_n_succeeded=st["seg_nsucc"]) for st in sts])


def frame(ctx, P, streams, sts, Ts=None, overlaps=None, tag="", outliers=False):
    """one frame on the device and in the restatement (which mutates sts): candidates -> constructed match -> selection, all compared.
    Returns (the device's candidates, its selection, the restatement's selection)."""
    Ts = [s["T"] for s in streams] if Ts is None else Ts
    overlaps = [s["overlap"] for s in streams] if overlaps is None else overlaps
    ctx.candidates_run([P.abi.CandidateFrameJob(T, ov, cur_slot=0) for T, ov in zip(Ts, overlaps)])
    got_c = ctx.candidates_fetch()
    want_c = [N.candidates(st, T, ov, Ic.CAM_T, Ic.CELL, Ic.SEG_CELL, Ic.BOUNDARY) for st, T, ov in zip(sts, Ts, overlaps)]
    for k, (g, w) in enumerate(zip(got_c, want_c)):
        assert (g["n_filed_pt"], g["n_filed_seg"]) == (w["n_filed_pt"], w["n_filed_seg"]), (tag, k)
        for f in CAND_FIELDS:
            same_bytes(g[f], w[f], (tag, "candidates", k, f))
    matches = [Sc.match_of(s, r) for s, r in zip(streams, want_c)]
    if outliers:                                                      # every seventh match lands six pixels off: the pose optimiser rejects it
        for m in matches:
            m["px"][::7] += 6.0
    ctx.candidates_set_match(matches)
    ctx.candidates_select(**Ic.PARAMS)
    got = ctx.candidates_select_fetch()
    want = []
    for k, (s, st, T, r, m) in enumerate(zip(streams, sts, Ts, want_c, matches)):
        w = S.select(st, r, m, Ic.CAM_T, Ic.CELL, Ic.SEG_CELL, Ic.PARAMS["max_fts"], Ic.PARAMS["max_fts_segs"], A=device_A(ctx, P, st, T, r))
        want.append(w)
        assert (got[k]["n_matches"], got[k]["n_ls_matches"], got[k]["n_trials"]) == (w["n_matches"], w["n_ls_matches"], w["n_trials"]), (tag, k)
        for f in SEL_FIELDS:
            same_bytes(got[k][f], w[f], (tag, "select", k, f))
    return got_c, got, want


def check_tables(ctx, sts, tag):
    got = ctx.candidates_fetch_map()
    for k, (g, st) in enumerate(zip(got, sts)):
        want = Ic.tables(st)
        for f in Cc.abi._CAND_MAP_ORDER:
            same_bytes(g[f], want[f], (tag, "map", k, f))


def insert(ctx, streams, sts, sels, active, remove, masks=None, poses=None, tag=""):
    """the insertion on the device and in the restatement (which mutates sts), all compared: tables, quality, events, the report"""
    masks = [Ic.keep_masks(s, sel) for s, sel in zip(streams, sels)] if masks is None else masks
    ins = [dict(remove_kf=r, kf_slot=s["kf_slot"], T_f_w=s["T_new"] if poses is None else None, pt_keep=None if m is None else m[0], seg_keep=None if m is None else m[1])
           if a else None for s, a, r, m in zip(streams, active, remove, masks)]
    ctx.candidates_insert_keyframe(ins)
    outs = []
    for k, (s, st, sel, a, r, m) in enumerate(zip(streams, sts, sels, active, remove, masks)):
        if not a:
            outs.append(None)
            continue
        pk, sk = Ic.keep_masks(s, sel) if m is None else m
        outs.append(Ic.I.insert(st, sel, pk, sk, s["T_new"] if poses is None else poses[k], s["kf_slot"], r, Ic.CAM_T))
    check_tables(ctx, sts, tag)
    quality, report = ctx.candidates_fetch_quality(), ctx.candidates_insert_fetch()
    for k, (st, sel, o, q, rep) in enumerate(zip(sts, sels, outs, quality, report)):
        for f, key in QUALITY:
            same_bytes(q[f], st[key], (tag, "quality", k, f))
        for name in ("pt", "seg"):
            want = [a | (o[name + "_event"][i] if o else 0) for i, a in enumerate(sel[name + "_event"])]
            same_bytes(q[name + "_event"], want, (tag, "event", k, name))
        sz = Ic.sizes(st)
        assert {f: rep[f] for f in OUT_SIZES} == sz, (tag, k, rep, sz)
        if o:
            assert rep["new_kf"] == o["new_kf"] == sz["n_kf"] - 1, (tag, k)
            assert (rep["n_joined_pt"], rep["n_joined_seg"], rep["n_deleted_pt"], rep["n_deleted_seg"]) == (o["n_joined_pt"], o["n_joined_seg"], o["n_deleted_pt"], o["n_deleted_seg"]), (tag, k, rep, o)
        else:
            assert rep["new_kf"] == -1 and rep["n_joined_pt"] == rep["n_deleted_pt"] == 0, (tag, k)
    return outs


def second_frames(streams, sts):
    two = [Ic.second_frame_of(s, st, k) for k, (s, st) in enumerate(zip(streams, sts))]
    return [t for t, _ in two], [o for _, o in two]


@pytest.mark.gpu
def test_insertion_equals_the_restatement_and_later_frames_run_on_its_tables(ctx, P):
    """thirteen unequal streams of which ten insert: the tables after the insertion are the restatement's; a second frame on them equals
    np_candidates / np_select on the restatement's tables (an appended feature changes the visit order) and equals, byte for byte, the
    same frame after a fresh stage of those tables; a second insertion on top of the first is the restatement's again"""
    streams = Ic.batch()
    sts = [copy.deepcopy(s["st"]) for s in streams]
    stage(ctx, sts)
    check_tables(ctx, sts, "staged")
    _, _, sel1 = frame(ctx, P, streams, sts, tag="frame 1")
    outs = insert(ctx, streams, sts, sel1, [s["is_kf"] for s in streams], [s["remove_kf"] for s in streams], tag="insertion 1")
    assert sum(o["n_joined_pt"] for o in outs if o) > 60 and sum(o["n_joined_seg"] for o in outs if o) > 5 and sum(o["n_deleted_seg"] for o in outs if o) > 3
    after1 = copy.deepcopy(sts)
    T2, ov2 = second_frames(streams, sts)
    c2, s2, sel2 = frame(ctx, P, streams, sts, T2, ov2, tag="frame 2")
    assert sum(s["n_matches"] for s in s2) > 100
    # a second insertion: the streams that stood by insert now, every other of the rest again; the oldest row leaves where there are two
    active = [(not s["is_kf"]) or k % 2 == 0 for k, s in enumerate(streams)]
    remove = [0 if len(st["kf_T"]) >= 2 else -1 for st in sts]
    insert(ctx, streams, sts, sel2, active, remove, tag="insertion 2")
    T3, ov3 = second_frames(streams, sts)
    frame(ctx, P, streams, sts, T3, ov3, tag="frame 3")
    # the second frame again, after a fresh stage of the tables the first insertion left
    fresh = copy.deepcopy(after1)
    stage(ctx, fresh)
    c2b, s2b, _ = frame(ctx, P, streams, fresh, T2, ov2, tag="frame 2, restaged")
    for k in range(len(streams)):
        for f in CAND_FIELDS:
            same_bytes(c2b[k][f], c2[k][f], ("restaged", "candidates", k, f))
        for f in ("pt_cand_failed", "seg_cand_failed"):               # (the resident lists have closed up inside their staged room)
            same_bytes(c2[k][f][:len(c2b[k][f])], c2b[k][f], ("restaged", "candidates", k, f))
        for f in s2[k]:
            same_bytes(s2b[k][f], s2[k][f], ("restaged", "select", k, f))


@pytest.mark.gpu
def test_one_stream_at_a_time_equals_its_place_in_the_batch(ctx, P):
    streams = Ic.batch()
    sts = [copy.deepcopy(s["st"]) for s in streams]
    stage(ctx, sts)
    _, _, sel = frame(ctx, P, streams, sts, tag="batch")
    insert(ctx, streams, sts, sel, [s["is_kf"] for s in streams], [s["remove_kf"] for s in streams], tag="batch")
    whole, quality = ctx.candidates_fetch_map(), ctx.candidates_fetch_quality()
    for k in (0, 2, 5, 11, 12):
        one = [copy.deepcopy(streams[k]["st"])]
        stage(ctx, one)
        _, _, sel = frame(ctx, P, streams[k:k + 1], one, tag=("alone", k))
        insert(ctx, streams[k:k + 1], one, sel, [True], [streams[k]["remove_kf"]], tag=("alone", k))
        g, q = ctx.candidates_fetch_map()[0], ctx.candidates_fetch_quality()[0]
        for f in g:
            same_bytes(g[f], whole[k][f], ("alone", k, f))
        for f in q:
            same_bytes(q[f], quality[k][f], ("alone", k, f))


@pytest.mark.gpu
def test_resident_masks_and_pose_behind_the_pose_optimiser(ctx, P):
    """NULL masks and PLSVO_INSERT_POSE_RESIDENT: the insertion reads the keep masks and the pose plsvo_candidates_pose_optimize left on the
    device; the masks and poses of pose_fetch go into the restatement"""
    streams = Ic.batch()
    sts = [copy.deepcopy(s["st"]) for s in streams]
    stage(ctx, sts)
    _, got, sel = frame(ctx, P, streams, sts, tag="frame", outliers=True)
    ctx.candidates_pose_optimize()
    po = ctx.candidates_pose_fetch([(g["n_matches"], g["n_ls_matches"]) for g in got])
    masks = [(p.pt_keep, p.seg_keep) for p in po]
    assert sum(int(m[0].sum()) for m in masks) > 50 and any(0 in m[0] or 0 in m[1] for m in masks)       # kept and rejected features
    ins = [dict(remove_kf=s["remove_kf"], kf_slot=s["kf_slot"]) if s["is_kf"] else None for s in streams]
    ctx.candidates_insert_keyframe(ins)
    for s, st, w, m, p in zip(streams, sts, sel, masks, po):
        if s["is_kf"]:
            Ic.I.insert(st, w, m[0], m[1], [float(v) for v in p.T], s["kf_slot"], s["remove_kf"], Ic.CAM_T)
    check_tables(ctx, sts, "resident")


def needed(s):
    """the room the insertion of stream s needs beyond its staged sizes, from the restatement"""
    st = copy.deepcopy(s["st"])
    before = Ic.sizes(st)
    _, _, sel = Ic.frame(s, st)
    Ic.insert(s, st, sel)
    after = Ic.sizes(st)
    return {r: after[f] - before[f] for r, f in (("extra_kf", "n_kf"), ("extra_kf_pt", "n_kf_pt"), ("extra_kf_seg", "n_kf_seg"), ("extra_pt_obs", "n_pt_obs"), ("extra_seg_obs", "n_seg_obs"))}


@pytest.mark.gpu
def test_capacity_is_decided_before_anything_changes(ctx, P):
    """room exactly sufficient passes; one entry short in each of the five kinds returns PLSVO_E_CAPACITY and leaves EVERY stream's tables,
    quality and candidate lists what they were (the stream beside the short one would have fitted)"""
    rng = np.random.default_rng(6301)
    grow = Ic.random_stream(rng, 3, 50, 30, 12, 10, remove_kf=-1, p_found=0.9)
    small = Ic.first_keyframe_stream()
    streams = (small, grow)
    need = needed(grow)
    assert all(v > 0 for v in need.values()), need
    for short in (None,) + tuple(need):
        reserve = dict(need)
        if short:
            reserve[short] -= 1
        sts = [copy.deepcopy(s["st"]) for s in streams]
        stage(ctx, sts, reserve)
        _, _, sel = frame(ctx, P, streams, sts, tag=("capacity", short))
        if short is None:
            insert(ctx, streams, sts, sel, [True, True], [-1, -1], tag="exact room")
            continue
        before_m, before_q = ctx.candidates_fetch_map(), ctx.candidates_fetch_quality()
        masks = [Ic.keep_masks(s, w) for s, w in zip(streams, sel)]
        with pytest.raises(P.capi.PlsvoError) as e:
            ctx.candidates_insert_keyframe([dict(remove_kf=-1, kf_slot=1, T_f_w=s["T_new"], pt_keep=m[0], seg_keep=m[1]) for s, m in zip(streams, masks)])
        assert e.value.code == P.abi.E_CAPACITY, short
        after_m, after_q = ctx.candidates_fetch_map(), ctx.candidates_fetch_quality()
        for a, b in zip(before_m + before_q, after_m + after_q):
            for f in a:
                same_bytes(b[f], a[f], ("refused", short, f))
        check_tables(ctx, sts, ("refused", short))


@pytest.mark.gpu
def test_fetch_map_follows_the_staged_layout_not_the_last_reserve(ctx, P):
    """the room is the one in force when the tables were staged: a plsvo_candidates_reserve between an insertion and fetch_map (the harness
    gives its room back while the grown tables stay resident) changes neither the reported capacity nor what fetch_map needs and returns"""
    streams = Ic.batch()[4:7]
    sts = [copy.deepcopy(s["st"]) for s in streams]
    stage(ctx, sts)
    staged = [Ic.sizes(st) for st in sts]
    cap = ctx.candidates_capacity()
    for c, z in zip(cap, staged):
        assert c == dict(kf=z["n_kf"] + Ic.RESERVE["extra_kf"], kf_pt=z["n_kf_pt"] + Ic.RESERVE["extra_kf_pt"], kf_seg=z["n_kf_seg"] + Ic.RESERVE["extra_kf_seg"],
                         pt_obs=z["n_pt_obs"] + Ic.RESERVE["extra_pt_obs"], seg_obs=z["n_seg_obs"] + Ic.RESERVE["extra_seg_obs"])
    _, _, sel = frame(ctx, P, streams, sts, tag="frame")
    insert(ctx, streams, sts, sel, [True] * 3, [-1] * 3, tag="insertion")
    assert all(Ic.sizes(st)["n_pt_obs"] > z["n_pt_obs"] and Ic.sizes(st)["n_kf"] > z["n_kf"] for st, z in zip(sts, staged))     # the tables have grown past the tight layout
    for reserve in (dict(), dict(extra_kf=1, extra_pt_obs=3)):
        ctx.candidates_reserve(**reserve)
        assert ctx.candidates_capacity() == cap
        check_tables(ctx, sts, ("after reserve", tuple(reserve)))
    only = ctx.candidates_fetch_map(streams=[1])
    assert only[0] is None and only[2] is None
    for f in only[1]:
        same_bytes(only[1][f], Ic.tables(sts[1])[f], ("one stream", f))
    assert ctx.L.plsvo_candidates_capacity(ctx.h, 2, (P.abi.CandReserve * 3)()) == P.abi.E_INVALID and ctx.L.plsvo_candidates_capacity(ctx.h, 3, None) == P.abi.E_INVALID


@pytest.mark.gpu
def test_insert_error_paths(ctx, P):
    L, h, A = ctx.L, ctx.h, P.abi
    streams = Ic.batch()[4:7]
    sts = [copy.deepcopy(s["st"]) for s in streams]
    stage(ctx, sts)
    ins = (A.CandInsert * 3)()
    for a in ins:
        a.is_kf, a.remove_kf, a.kf_slot = 1, -1, 1
    assert L.plsvo_candidates_insert_fetch(h, 3, (A.CandInsertOut * 3)()) == A.E_STATE                   # no insertion yet
    assert L.plsvo_candidates_insert_keyframe(h, 3, ins) == A.E_STATE                                    # no run
    ctx.candidates_run([A.CandidateFrameJob(s["T"], s["overlap"], cur_slot=0) for s in streams])
    assert L.plsvo_candidates_insert_keyframe(h, 3, ins) == A.E_STATE                                    # no selection
    want_c = [Sc.restate_candidates(s, st) for s, st in zip(streams, sts)]
    ctx.candidates_set_match([Sc.match_of(s, r) for s, r in zip(streams, want_c)])
    ctx.candidates_select(**Ic.PARAMS)
    before_m, before_q = ctx.candidates_fetch_map(), ctx.candidates_fetch_quality()
    assert L.plsvo_candidates_insert_keyframe(h, 3, ins) == A.E_STATE                                    # NULL masks, no resident pose optimisation
    keep = np.ones(400, np.uint8)
    for a in ins:
        a.pt_keep = a.seg_keep = keep.ctypes.data_as(A.c_u8_p)
    ins[1].pose_source = A.INSERT_POSE_RESIDENT
    assert L.plsvo_candidates_insert_keyframe(h, 3, ins) == A.E_STATE                                    # the resident pose, no pose optimisation
    ins[1].pose_source = A.INSERT_POSE_HOST
    assert L.plsvo_candidates_insert_keyframe(h, 2, ins) == A.E_INVALID and L.plsvo_candidates_insert_keyframe(h, 3, None) == A.E_INVALID
    for field, bad in (("remove_kf", len(sts[1]["kf_T"])), ("remove_kf", -2), ("kf_slot", -1), ("pose_source", 3), ("pose_source", A.INSERT_POSE_DEV)):
        old = getattr(ins[1], field)
        setattr(ins[1], field, bad)
        assert L.plsvo_candidates_insert_keyframe(h, 3, ins) == A.E_INVALID, (field, bad)
        setattr(ins[1], field, old)
    assert L.plsvo_candidates_fetch_map(h, 2, (A.CandMapOut * 3)()) == A.E_INVALID and L.plsvo_candidates_fetch_map(h, 3, None) == A.E_INVALID
    bad_idx = np.array([len(sts[0]["pt_pos"])], np.int32)
    pos = (A.CandPositions * 3)()
    pos[0].n_pt, pos[0].pt_idx, pos[0].pt_pos = 1, bad_idx.ctypes.data_as(A.c_i32_p), np.zeros(3).ctypes.data_as(A.c_double_p)
    assert L.plsvo_candidates_set_positions(h, 3, pos) == A.E_INVALID and L.plsvo_candidates_set_positions(h, 2, pos) == A.E_INVALID
    r = A.CandReserve(0, -1, 0, 0, 0, 0)
    assert L.plsvo_candidates_reserve(h, C.byref(r)) == A.E_INVALID
    after_m, after_q = ctx.candidates_fetch_map(), ctx.candidates_fetch_quality()
    for a, b in zip(before_m + before_q, after_m + after_q):
        for f in a:
            same_bytes(b[f], a[f], ("unchanged", f))
    # the insertion itself, once; a second one on the same run is refused
    ins[1].is_kf = 0
    assert L.plsvo_candidates_insert_keyframe(h, 3, ins) == A.OK
    assert L.plsvo_candidates_insert_keyframe(h, 3, ins) == A.E_STATE
    # the run is over: what would read its candidates against the new tables is refused until the next run; its results can still be fetched
    pr = A.CandSelectParams()
    pr.max_fts, pr.max_fts_segs, pr.poseopt_n_iter, pr.reproj_thresh = 120, 100, 10, 2.0
    assert L.plsvo_candidates_match(h) == A.E_STATE and L.plsvo_candidates_select(h, C.byref(pr)) == A.E_STATE and L.plsvo_candidates_pose_optimize(h) == A.E_STATE
    assert L.plsvo_candidates_set_match(h, 3, (A.CandMatchOut * 3)()) == A.E_STATE and L.plsvo_candidates_dev(h, C.byref(A.CandDev())) == A.E_STATE
    assert len(ctx.candidates_select_fetch()) == 3
    ctx.candidates_run([A.CandidateFrameJob(s["T"], s["overlap"], cur_slot=0) for s in streams])
    assert L.plsvo_candidates_dev(h, C.byref(A.CandDev())) == A.OK
    rep = ctx.candidates_insert_fetch()
    assert [r["new_kf"] for r in rep] == [len(sts[0]["kf_T"]), -1, len(sts[2]["kf_T"])]


@pytest.mark.gpu
def test_set_positions_equals_a_restage_with_the_moved_positions(ctx, P):
    streams = Ic.batch()[4:8]
    rng = np.random.default_rng(6302)
    sts = [copy.deepcopy(s["st"]) for s in streams]
    stage(ctx, sts)
    moved = []
    for k, st in enumerate(sts):
        if k == 1:
            moved.append(None)
            continue
        pi, si = rng.permutation(len(st["pt_pos"]))[:25], rng.permutation(len(st["seg_spos"]))[:7]
        m = dict(pt_idx=pi, pt_pos=np.array(st["pt_pos"])[pi] + rng.uniform(-0.05, 0.05, (len(pi), 3)), seg_idx=si,
                 seg_spos=np.array(st["seg_spos"])[si] + rng.uniform(-0.05, 0.05, (len(si), 3)), seg_epos=np.array(st["seg_epos"])[si] + rng.uniform(-0.05, 0.05, (len(si), 3)))
        for i, p in zip(pi, m["pt_pos"]):
            st["pt_pos"][i] = [float(v) for v in p]
        for i, a, b in zip(si, m["seg_spos"], m["seg_epos"]):
            st["seg_spos"][i] = [float(v) for v in a]; st["seg_epos"][i] = [float(v) for v in b]
        moved.append(m)
    ctx.candidates_set_positions(moved)
    check_tables(ctx, sts, "moved")
    ctx.candidates_run([P.abi.CandidateFrameJob(s["T"], s["overlap"], cur_slot=0) for s in streams])
    got = ctx.candidates_fetch()
    stage(ctx, sts)
    ctx.candidates_run([P.abi.CandidateFrameJob(s["T"], s["overlap"], cur_slot=0) for s in streams])
    want = ctx.candidates_fetch()
    for k, (g, w) in enumerate(zip(got, want)):
        for f in g:
            same_bytes(g[f], w[f], ("moved", k, f))


@pytest.mark.gpu
def test_a_reserve_of_zeros_is_the_tight_layout_and_room_changes_no_result(P):
    streams = Ic.batch()[:6]
    jobs = [Cc.to_job(s["st"]) for s in streams]
    frames = [P.abi.CandidateFrameJob(s["T"], s["overlap"], cur_slot=0) for s in streams]
    res = []
    for reserve in (None, dict(), Ic.RESERVE):
        ctx = P.capi.Context(0)
        try:
            if reserve is not None:
                ctx.candidates_reserve(**reserve)
            ctx.candidates_stage(jobs, Ic.CAM, Ic.CELL, Ic.SEG_CELL, Ic.BOUNDARY)
            ctx.candidates_run(frames)
            out = ctx.candidates_fetch()
            d = ctx.candidates_dev()
            res.append((out, [int(d.m_off[k]) for k in range(len(jobs))], [int(d.f_off[k]) for k in range(len(jobs))], int(d.n_frames), ctx.candidates_fetch_map()))
        finally:
            ctx.close()
    assert res[0][1:4] == res[1][1:4] and res[2][2] != res[0][2] and res[2][1] == res[0][1]
    for other in res[1:]:
        for k in range(len(jobs)):
            for f in res[0][0][k]:
                same_bytes(other[0][k][f], res[0][0][k][f], ("reserve", k, f))
            for f in res[0][4][k]:
                same_bytes(other[4][k][f], res[0][4][k][f], ("reserve", "map", k, f))


@pytest.mark.gpu
def test_insert_full_size_replicas(ctx, P):
    """1024 streams: 16 distinct tables (10 keyframes of about 200 + 80 features) x 64 replicas, every other stream inserts.  Every replica
    equals its first instance with the same choice, and the first thirty-two equal the restatement"""
    rng = np.random.default_rng(6303)
    base = [Ic.random_stream(rng, 10, 700, 260, 12, 6, remove_kf=int(rng.integers(-1, 10))) for _ in range(16)]
    reps = 64
    streams = base * reps
    active = [(k + k // 16) % 2 == 0 for k in range(16 * reps)]
    sts = [copy.deepcopy(s["st"]) for s in base]
    assert np.mean([Ic.sizes(st)["n_kf_pt"] for st in sts]) / 10 > 180 and np.mean([Ic.sizes(st)["n_kf_seg"] for st in sts]) / 10 > 70
    jobs = [Cc.to_job(st) for st in sts]
    ctx.candidates_reserve(extra_kf=1, extra_kf_pt=200, extra_kf_seg=200, extra_pt_obs=200, extra_seg_obs=200)
    ctx.candidates_stage(jobs * reps, Ic.CAM, Ic.CELL, Ic.SEG_CELL, Ic.BOUNDARY)
    ctx.candidates_set_quality([dict(pt_n_failed=st["pt_nfail"], pt_n_succeeded=st["pt_nsucc"], seg_n_failed=st["seg_nfail"], seg_n_succeeded=st["seg_nsucc"]) for st in sts] * reps)
    ctx.candidates_run([P.abi.CandidateFrameJob(s["T"], s["overlap"], cur_slot=0) for s in streams])
    want_c = [Sc.restate_candidates(s, st) for s, st in zip(base, sts)]
    matches = [Sc.match_of(s, r) for s, r in zip(base, want_c)]
    ctx.candidates_set_match(matches * reps)
    ctx.candidates_select(**Ic.PARAMS)
    sel = [S.select(st, r, m, Ic.CAM_T, Ic.CELL, Ic.SEG_CELL, Ic.PARAMS["max_fts"], Ic.PARAMS["max_fts_segs"], A={}) for st, r, m in zip(sts, want_c, matches)]
    masks = [Ic.keep_masks(s, w) for s, w in zip(base, sel)]
    ctx.candidates_insert_keyframe([dict(remove_kf=streams[k]["remove_kf"], kf_slot=1, T_f_w=Ic.T_NEW, pt_keep=masks[k % 16][0], seg_keep=masks[k % 16][1]) if active[k] else None
                                    for k in range(16 * reps)])
    got, quality = ctx.candidates_fetch_map(), ctx.candidates_fetch_quality()
    for k in range(32):
        st = copy.deepcopy(sts[k % 16])
        if active[k]:
            Ic.insert(base[k % 16], st, sel[k % 16])
        want = Ic.tables(st)
        for f in want:
            same_bytes(got[k][f], want[f], ("full_size", k, f))
        for f, key in QUALITY:
            same_bytes(quality[k][f], st[key], ("full_size", k, f))
    for k in range(32, 16 * reps):
        first = k % 16 + (0 if active[k] == active[k % 16] else 16)
        for f in got[k]:
            same_bytes(got[k][f], got[first][f], (k, f))
        for f in quality[k]:
            same_bytes(quality[k][f], quality[first][f], (k, f))
