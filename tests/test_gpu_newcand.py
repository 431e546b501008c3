"""New map candidates appended to the resident map tables on the device (plsvo_candidates_add ..; pl-svo_amd/csrc/newcand_device.hpp)
against their restatement tests/np_newcand.py on the cases of tests/newcand_cases.py.  Everything is compared byte for byte, array by
array: the kernel copies and computes nothing.  The frames behind an add are driven with constructed match results
(plsvo_candidates_set_match) and constructed keep masks, like those of tests/test_gpu_insert.py, whose helpers run them."""
import copy
import ctypes as C

import numpy as np
import pytest

import candidates_cases as Cc
import insert_cases as Ic
import newcand_cases as Nc
import np_select as S
import select_cases as Sc
from test_gpu_insert import QUALITY, check_tables, frame, insert
from test_gpu_select import same_bytes

REPORT = ("first_pt", "first_seg", "n_added_pt", "n_added_seg")


@pytest.fixture(scope="module")
def ctx(P):
    c = P.capi.Context(0)
    c.config_pyramids(4, Sc.CAM_T[4], Sc.CAM_T[5], 3)
    for s in range(4):
        c.build_pyramid(s, np.zeros((Sc.CAM_T[5], Sc.CAM_T[4]), np.uint8))
    yield c
    c.close()


def set_quality(ctx, sts):
    ctx.candidates_set_quality([dict(pt_n_failed=st["pt_nfail"], pt_n_succeeded=st["pt_nsucc"], seg_n_failed=st["seg_nfail"], seg_n_succeeded=st["seg_nsucc"]) for st in sts])


def stage(ctx, sts, reserve=Nc.RESERVE, lm_reserve=Nc.LM_RESERVE):
    ctx.candidates_reserve(**reserve)
    ctx.candidates_reserve_landmarks(**lm_reserve)
    ctx.candidates_stage([Cc.to_job(st) for st in sts], Nc.CAM, Nc.CELL, Nc.SEG_CELL, Nc.BOUNDARY)
    set_quality(ctx, sts)


def check_quality(ctx, sts, events, tag):
    for k, (q, st, ev) in enumerate(zip(ctx.candidates_fetch_quality(), sts, events)):
        for f, key in QUALITY:
            same_bytes(q[f], st[key], (tag, "quality", k, f))
        same_bytes(q["pt_event"], ev[0], (tag, "event", k, "pt")); same_bytes(q["seg_event"], ev[1], (tag, "event", k, "seg"))


def add(ctx, cases, sts, tag=""):
    """the add on the device and in the restatement (which mutates sts), all compared: tables, quality, events, the report"""
    before = [(q["pt_event"], q["seg_event"]) for q in ctx.candidates_fetch_quality()]
    ctx.candidates_add([Nc.records(s["new"]) for s in cases])
    reps = [Nc.add(s, st) for s, st in zip(cases, sts)]
    check_tables(ctx, sts, tag)
    events = [(list(b[0]) + r["pt_event"][len(b[0]):], list(b[1]) + r["seg_event"][len(b[1]):]) for b, r in zip(before, reps)]
    check_quality(ctx, sts, events, tag)
    for k, (got, want, st) in enumerate(zip(ctx.candidates_add_fetch(), reps, sts)):
        z = Ic.sizes(st)
        assert {f: got[f] for f in REPORT} == {f: want[f] for f in REPORT}, (tag, k, got)
        assert (got["n_pt"], got["n_seg"], got["n_pt_cand"], got["n_seg_cand"], got["n_pt_obs"], got["n_seg_obs"]) == \
               (len(st["pt_pos"]), len(st["seg_spos"]), z["n_pt_cand"], z["n_seg_cand"], z["n_pt_obs"], z["n_seg_obs"]), (tag, k, got)
    return reps


def posed(ctx, sel):
    ctx.candidates_pose_optimize()
    return ctx.candidates_pose_fetch([(g["n_matches"], g["n_ls_matches"]) for g in sel])


def staged_and_added(ctx):
    cases = Nc.batch()
    sts = [copy.deepcopy(s["st"]) for s in cases]
    stage(ctx, sts)
    check_tables(ctx, sts, "staged")
    add(ctx, cases, sts, "add")
    return cases, sts


@pytest.mark.gpu
def test_add_equals_the_restatement_and_the_next_frame_runs_on_the_grown_tables(ctx, P):
    """thirteen unequal streams of which nine add: tables, quality, events and the report are the restatement's; the next frame
    (run -> set_match -> select -> pose_optimize) equals np_candidates / np_select on the restatement's tables and equals, byte for byte,
    the same frame after a fresh stage of those tables plus set_quality"""
    cases, sts = staged_and_added(ctx)
    after = copy.deepcopy(sts)
    c1, s1, sel = frame(ctx, P, cases, sts, tag="frame on the grown tables")
    p1 = posed(ctx, s1)
    new_matched = sum(1 for s, w in zip(cases, sel) for lm in w["pt_lm"] if lm >= len(s["st"]["pt_pos"]))
    assert new_matched > 40 and sum(1 for s, w in zip(cases, sel) for lm in w["seg_lm"] if lm >= len(s["st"]["seg_spos"])) > 20   # the new candidates are features
    fresh = copy.deepcopy(after)
    stage(ctx, fresh)
    c2, s2, _ = frame(ctx, P, cases, fresh, tag="the same frame, restaged")
    p2 = posed(ctx, s2)
    for k in range(len(cases)):
        for f in c1[k]:
            same_bytes(c2[k][f], c1[k][f], ("restaged", "candidates", k, f))
        for f in s1[k]:
            same_bytes(s2[k][f], s1[k][f], ("restaged", "select", k, f))
        same_bytes(p2[k].T, p1[k].T, ("restaged", "pose", k)); same_bytes(p2[k].cov, p1[k].cov, ("restaged", "cov", k))
        same_bytes(p2[k].pt_keep, p1[k].pt_keep, ("restaged", "pt_keep", k)); same_bytes(p2[k].seg_keep, p1[k].seg_keep, ("restaged", "seg_keep", k))


@pytest.mark.gpu
@pytest.mark.parametrize("removal", (False, True))
def test_insertion_behind_an_add_equals_the_restatement(ctx, P, removal):
    """without a removal: the new candidates that were matched and kept join their keyframe (TYPE_UNKNOWN, the original feature appended
    to it).  With the removal of a keyframe that holds other new candidates' observation: those are deleted and erased.  Both against
    np_insert on np_newcand's tables; a frame on the result follows"""
    cases, sts = staged_and_added(ctx)
    n_old = [len(s["st"]["pt_pos"]) for s in cases]
    _, _, sel = frame(ctx, P, cases, sts, tag="frame")
    remove = [Nc.removal_of(s, st) if removal else -1 for s, st in zip(cases, sts)]
    doomed = [[lm for lm in st["pt_cand"] if lm >= n and st["pt_obs"][lm][-1]["kf"] == r] for st, n, r in zip(sts, n_old, remove)]
    outs = insert(ctx, cases, sts, sel, [True] * len(cases), remove, tag=("insertion", removal))
    joined = [lm for st, n, o in zip(sts, n_old, outs) for lm in range(n, len(st["pt_pos"])) if o["pt_event"][lm] & 4]
    assert len(joined) > 40
    if removal:
        gone = [(st, lm) for st, o, lms in zip(sts, outs, doomed) for lm in lms if not o["pt_event"][lm] & 4]
        assert len(gone) > 10 and all(st["pt_type"][lm] == Ic.D and lm not in st["pt_cand"] for st, lm in gone)
    two = [Ic.second_frame_of(s, st, k) for k, (s, st) in enumerate(zip(cases, sts))]
    frame(ctx, P, cases, sts, [t for t, _ in two], [o for _, o in two], tag=("frame behind the insertion", removal))


@pytest.mark.gpu
def test_adds_in_a_row_and_an_add_directly_behind_an_insertion(ctx, P):
    """a second add continues the indices behind the first; an add directly after an insertion on the same run works on the inserted tables
    (its observations name keyframes of the table as it stands now) and ORs nothing into the old landmarks' event bytes"""
    cases, sts = staged_and_added(ctx)
    more = Nc.second_new(cases, sts)
    reps = add(ctx, more, sts, "second add")
    assert all(r["first_pt"] == len(s["st"]["pt_pos"]) + len(s["new"]["pt"]) for r, s in zip(reps, cases) if r["n_added_pt"])
    _, _, sel = frame(ctx, P, more, sts, tag="frame")
    insert(ctx, more, sts, sel, [s["is_kf"] for s in more], [s["remove_kf"] if s["is_kf"] else -1 for s in more], tag="insertion")
    third = Nc.second_new(more, sts)                                  # (generated on the inserted tables: rows have moved, a new last keyframe)
    add(ctx, third, sts, "add behind the insertion")
    two = [Ic.second_frame_of(s, st, k) for k, (s, st) in enumerate(zip(third, sts))]
    frame(ctx, P, third, sts, [t for t, _ in two], [o for _, o in two], tag="frame behind the third add")


@pytest.mark.gpu
def test_one_stream_at_a_time_equals_its_place_in_the_batch(ctx, P):
    cases, sts = staged_and_added(ctx)
    whole, quality, report = ctx.candidates_fetch_map(), ctx.candidates_fetch_quality(), ctx.candidates_add_fetch()
    for k in (0, 2, 6, 7, 10, 12):
        one = [copy.deepcopy(cases[k]["st"])]
        stage(ctx, one)
        add(ctx, cases[k:k + 1], one, ("alone", k))
        g, q = ctx.candidates_fetch_map()[0], ctx.candidates_fetch_quality()[0]
        for f in g:
            same_bytes(g[f], whole[k][f], ("alone", k, f))
        for f in q:
            same_bytes(q[f], quality[k][f], ("alone", k, f))
        assert ctx.candidates_add_fetch()[0] == report[k]


def snapshot(ctx):
    return ctx.candidates_fetch_map() + ctx.candidates_fetch_quality()


def same_snapshot(ctx, before, tag):
    for a, b in zip(before, snapshot(ctx)):
        for f in a:
            same_bytes(b[f], a[f], (tag, f))


@pytest.mark.gpu
def test_capacity_is_decided_before_anything_changes(ctx, P):
    """room exactly sufficient passes; one short in each of the four kinds returns PLSVO_E_CAPACITY and leaves EVERY stream's tables,
    quality and lists what they were (the streams beside the short one would have fitted)"""
    cases = (Nc.batch()[11], Nc.batch()[7], Nc.batch()[9])            # stream 7 adds the most: 130 points, 65 segments
    need = dict(extra_pt=130, extra_seg=65, extra_pt_obs=130, extra_seg_obs=65)
    assert (len(cases[1]["new"]["pt"]), len(cases[1]["new"]["seg"])) == (130, 65)
    for short in (None,) + tuple(need):
        room = dict(need)
        if short:
            room[short] -= 1
        sts = [copy.deepcopy(s["st"]) for s in cases]
        stage(ctx, sts, dict(extra_pt_obs=room["extra_pt_obs"], extra_seg_obs=room["extra_seg_obs"]), dict(extra_pt=room["extra_pt"], extra_seg=room["extra_seg"]))
        assert ctx.candidates_lm_capacity() == [dict(pt=len(st["pt_pos"]) + room["extra_pt"], seg=len(st["seg_spos"]) + room["extra_seg"]) for st in sts]
        if short is None:
            add(ctx, cases, sts, "exact room")
            continue
        before = snapshot(ctx)
        with pytest.raises(P.capi.PlsvoError) as e:
            ctx.candidates_add([Nc.records(s["new"]) for s in cases])
        assert e.value.code == P.abi.E_CAPACITY, short
        same_snapshot(ctx, before, ("refused", short))
        check_tables(ctx, sts, ("refused", short))


@pytest.mark.gpu
def test_add_error_paths(P):
    L_ctx = P.capi.Context(0)
    try:
        _error_paths(L_ctx, P)
    finally:
        L_ctx.close()


def _error_paths(ctx, P):
    L, h, A = ctx.L, ctx.h, P.abi
    cases = Nc.batch()[6:9]                                           # stream 6 adds 65 points and a segment, 7 adds 130 / 65, 8 stands by
    sts = [copy.deepcopy(s["st"]) for s in cases]
    none = (A.CandNew * 3)()
    assert L.plsvo_candidates_add(h, 3, none) == A.E_STATE and L.plsvo_candidates_add_fetch(h, 3, (A.CandAddOut * 3)()) == A.E_STATE   # before a stage
    assert L.plsvo_candidates_lm_capacity(h, 3, (A.CandLmReserve * 3)()) == A.E_STATE
    assert L.plsvo_candidates_reserve_landmarks(h, C.byref(A.CandLmReserve(-1, 0))) == A.E_INVALID and L.plsvo_candidates_reserve_landmarks(h, C.byref(A.CandLmReserve(0, -1))) == A.E_INVALID
    stage(ctx, sts)
    assert L.plsvo_candidates_add_fetch(h, 3, (A.CandAddOut * 3)()) == A.E_STATE                         # no add since the stage
    assert L.plsvo_candidates_lm_capacity(h, 2, (A.CandLmReserve * 3)()) == A.E_INVALID and L.plsvo_candidates_lm_capacity(h, 3, None) == A.E_INVALID
    before = snapshot(ctx)
    assert L.plsvo_candidates_add(h, 2, none) == A.E_INVALID and L.plsvo_candidates_add(h, 3, None) == A.E_INVALID

    def build(mutate):
        """the records of the three streams as ctypes, stream 1's arrays changed by `mutate(dict of arrays)`; -> (array, keep-alive)"""
        arr, keep = (A.CandNew * 3)(), []
        for k, (a, s) in enumerate(zip(arr, cases)):
            d = Nc.records(s["new"])
            if d is None:
                continue
            d = {f: np.ascontiguousarray(v, dtype=np.int32 if f in A._CAND_NEW_I32 else np.uint8 if f in A._CAND_NEW_U8 else np.float64) for f, v in d.items()}
            a.n_pt, a.n_seg = len(d.get("pt_pos", ())), len(d.get("seg_spos", ()))
            if k == 1:
                mutate(d, a)
            for f, v in d.items():
                if v is not None:
                    keep.append(v)
                    setattr(a, f, ctx._ptr(v))
        return arr, keep

    n_kf = len(sts[1]["kf_T"])

    def set_at(f, i, v):
        def m(d, a):
            d[f] = d[f].copy(); d[f][i] = v
        return m

    def drop(f):
        def m(d, a):
            d[f] = None
        return m

    def count(f, v):
        def m(d, a):
            setattr(a, f, v)
        return m
    invalid = [("negative point count", count("n_pt", -1)), ("negative segment count", count("n_seg", -3)), ("keyframe == n_kf", set_at("pt_obs_kf", 129, n_kf)),
               ("negative keyframe", set_at("seg_obs_kf", 0, -1)), ("level == PLSVO_MAX_LEVELS", set_at("pt_obs_level", 5, 8)), ("negative level", set_at("seg_obs_level", 64, -1)),
               ("unknown feature type", set_at("pt_obs_type", 77, 2)), ("edgelets without gradients", drop("pt_obs_grad"))]
    invalid += [("null " + f, drop(f)) for f in A._CAND_NEW_ORDER if f != "pt_obs_grad"]
    assert any(t == 1 for t in Nc.records(cases[1]["new"])["pt_obs_type"])
    for name, mutate in invalid:
        arr, keep = build(mutate)
        assert L.plsvo_candidates_add(h, 3, arr) == A.E_INVALID, name
    same_snapshot(ctx, before, "invalid")
    assert L.plsvo_candidates_add_fetch(h, 3, (A.CandAddOut * 3)()) == A.E_STATE                         # (none of them counted as an add)
    # corners without gradients are accepted: zeros are stored
    corners = copy.deepcopy(sts)
    plain = [dict(s, new=dict(pt=[dict(p, obs=dict(p["obs"], type=0, grad=[0.0, 0.0])) for p in s["new"]["pt"]], seg=s["new"]["seg"])) for s in cases]
    recs = [Nc.records(s["new"]) for s in plain]
    for r in recs:
        if r and "pt_obs_grad" in r:
            del r["pt_obs_grad"]
    ctx.candidates_add(recs)
    for s, st in zip(plain, corners):
        Nc.add(s, st)
    check_tables(ctx, corners, "corners without gradients")
    # an add ends the open run: what reads the run's candidates against the new tables is refused until the next run; its fetches still work
    stage(ctx, sts)
    ctx.candidates_run([A.CandidateFrameJob(s["T"], s["overlap"], cur_slot=0) for s in cases])
    want_c = [Sc.restate_candidates(s, st) for s, st in zip(cases, sts)]
    ctx.candidates_set_match([Sc.match_of(s, r) for s, r in zip(cases, want_c)])
    ctx.candidates_select(**Nc.PARAMS)
    sel_before, cand_before = ctx.candidates_select_fetch(), ctx.candidates_fetch()
    ctx.candidates_add([Nc.records(s["new"]) for s in cases])
    pr = A.CandSelectParams()
    pr.max_fts, pr.max_fts_segs, pr.poseopt_n_iter, pr.reproj_thresh = 120, 100, 10, 2.0
    ins = (A.CandInsert * 3)()
    keepm = np.ones(400, np.uint8)
    for a in ins:
        a.is_kf, a.remove_kf, a.kf_slot, a.pt_keep, a.seg_keep = 1, -1, 1, keepm.ctypes.data_as(A.c_u8_p), keepm.ctypes.data_as(A.c_u8_p)
    after_add = snapshot(ctx)
    assert L.plsvo_candidates_match(h) == A.E_STATE and L.plsvo_candidates_select(h, C.byref(pr)) == A.E_STATE and L.plsvo_candidates_pose_optimize(h) == A.E_STATE
    assert L.plsvo_candidates_set_match(h, 3, (A.CandMatchOut * 3)()) == A.E_STATE and L.plsvo_candidates_dev(h, C.byref(A.CandDev())) == A.E_STATE
    assert L.plsvo_candidates_insert_keyframe(h, 3, ins) == A.E_STATE
    same_snapshot(ctx, after_add, "closed run")
    for a, b in zip(sel_before + cand_before, ctx.candidates_select_fetch() + ctx.candidates_fetch()):   # the run's results, as they were
        for f in a:
            same_bytes(b[f], a[f], ("the run's fetches", f))
    # the same refusals when the add comes before the selection of its run
    ctx.candidates_run([A.CandidateFrameJob(s["T"], s["overlap"], cur_slot=0) for s in cases])
    ctx.candidates_add([None, None, None])                            # an add of nothing ends the run all the same
    assert L.plsvo_candidates_match(h) == A.E_STATE and L.plsvo_candidates_select(h, C.byref(pr)) == A.E_STATE
    ctx.candidates_run([A.CandidateFrameJob(s["T"], s["overlap"], cur_slot=0) for s in cases])
    assert L.plsvo_candidates_dev(h, C.byref(A.CandDev())) == A.OK
    # the maximum observation level follows the new observations: level 3 lies outside the three-level pyramid of the matcher
    ctx.config_pyramids(4, Sc.CAM_T[4], Sc.CAM_T[5], 3)
    for slot in range(4):
        ctx.build_pyramid(slot, np.zeros((Sc.CAM_T[5], Sc.CAM_T[4]), np.uint8))
    ctx.candidates_match()
    high = Nc.make_new(np.random.default_rng(1), cases[0], sts[0], 1, 0)[0]
    high["pt"][0]["obs"]["level"] = 3
    ctx.candidates_add([Nc.records(high), None, None])
    ctx.candidates_run([A.CandidateFrameJob(s["T"], s["overlap"], cur_slot=0) for s in cases])
    assert L.plsvo_candidates_match(h) == A.E_CAPACITY


@pytest.mark.gpu
def test_a_landmark_reserve_of_zeros_is_todays_layout_and_room_changes_no_result(P):
    streams = Ic.batch()[:6]
    jobs = [Cc.to_job(s["st"]) for s in streams]
    frames = [P.abi.CandidateFrameJob(s["T"], s["overlap"], cur_slot=0) for s in streams]
    res = []
    for lm_reserve in (None, dict(), Nc.LM_RESERVE):
        ctx = P.capi.Context(0)
        try:
            if lm_reserve is not None:
                ctx.candidates_reserve_landmarks(**lm_reserve)
            ctx.candidates_stage(jobs, Ic.CAM, Ic.CELL, Ic.SEG_CELL, Ic.BOUNDARY)
            ctx.candidates_run(frames)
            out = ctx.candidates_fetch()
            d = ctx.candidates_dev()
            offs = ([int(d.m_off[k]) for k in range(len(jobs))], [int(d.f_off[k]) for k in range(len(jobs))], int(d.n_frames), int(d.n_entries))
            want_c = [Sc.restate_candidates(s) for s in streams]
            ctx.candidates_set_match([Sc.match_of(s, r) for s, r in zip(streams, want_c)])
            ctx.candidates_select(**Ic.PARAMS)
            res.append((out, offs, ctx.candidates_select_fetch(), ctx.candidates_fetch_map(), ctx.candidates_fetch_quality(), ctx.candidates_lm_capacity()))
        finally:
            ctx.close()
    assert res[0][1] == res[1][1] and res[2][1][0] != res[0][1][0] and res[2][1][1] == res[0][1][1]      # room moves the matcher rows, not the frame table
    assert res[0][5] == res[1][5] == [dict(pt=j.n_pt, seg=j.n_seg) for j in jobs]
    for other in res[1:]:
        for part in (0, 2, 3, 4):
            for k in range(len(jobs)):
                for f in res[0][part][k]:
                    same_bytes(other[part][k][f], res[0][part][k][f], ("reserve", part, k, f))


@pytest.mark.gpu
def test_add_full_size_replicas(ctx, P):
    """1024 streams: 16 distinct tables x 64 replicas, every other stream adds.  Every replica equals its first instance with the same
    choice, and the first thirty-two equal the restatement"""
    rng = np.random.default_rng(7103)
    base = [Ic.random_stream(rng, 10, 700, 260, 12, 6, remove_kf=-1) for _ in range(16)]
    news = [Nc.make_new(rng, s, s["st"], int(rng.integers(1, 140)), int(rng.integers(1, 140)))[0] for s in base]
    reps = 64
    active = [(k + k // 16) % 2 == 0 for k in range(16 * reps)]
    jobs = [Cc.to_job(s["st"]) for s in base]
    ctx.candidates_reserve(extra_pt_obs=140, extra_seg_obs=140)
    ctx.candidates_reserve_landmarks(extra_pt=140, extra_seg=140)
    ctx.candidates_stage(jobs * reps, Nc.CAM, Nc.CELL, Nc.SEG_CELL, Nc.BOUNDARY)
    set_quality(ctx, [s["st"] for s in base] * reps)
    recs = [Nc.records(n) for n in news]
    ctx.candidates_add([recs[k % 16] if active[k] else None for k in range(16 * reps)])
    got, quality = ctx.candidates_fetch_map(), ctx.candidates_fetch_quality()
    for k in range(32):
        st = copy.deepcopy(base[k % 16]["st"])
        ev = ([0] * len(st["pt_pos"]), [0] * len(st["seg_spos"]))
        if active[k]:
            r = Nc.NC.add(st, news[k % 16])
            ev = (r["pt_event"], r["seg_event"])
        want = Ic.tables(st)
        for f in want:
            same_bytes(got[k][f], want[f], ("full_size", k, f))
        for f, key in QUALITY:
            same_bytes(quality[k][f], st[key], ("full_size", k, f))
        same_bytes(quality[k]["pt_event"], ev[0], ("full_size", k)); same_bytes(quality[k]["seg_event"], ev[1], ("full_size", k))
    for k in range(32, 16 * reps):
        first = k % 16 + (0 if active[k] == active[k % 16] else 16)
        for f in got[k]:
            same_bytes(got[k][f], got[first][f], (k, f))
        for f in quality[k]:
            same_bytes(quality[k][f], quality[first][f], (k, f))
