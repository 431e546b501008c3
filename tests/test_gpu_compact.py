"""The compaction of the resident map tables on the device (plsvo_candidates_compact ..; pl-svo_amd/csrc/compact_device.hpp) against its
restatement tests/np_compact.py: on the directed cases of tests/compact_cases.py, and on tables whose deleted rows arose the real way
(an add, a frame's selection, an insertion with a removal; the cases of tests/newcand_cases.py).  Everything is compared byte for byte,
array by array: the kernel moves rows and computes nothing."""
import copy
import ctypes as C

import numpy as np
import pytest

import candidates_cases as Cc
import compact_cases as K
import insert_cases as Ic
import newcand_cases as Nc
import np_candidates as N
import np_compact as NK
import select_cases as Sc
from test_gpu_insert import QUALITY, check_tables, frame, insert
from test_gpu_select import same_bytes


@pytest.fixture(scope="module")
def ctx(P):
    c = P.capi.Context(0)
    c.config_pyramids(4, Sc.CAM_T[4], Sc.CAM_T[5], 3)
    for s in range(4):
        c.build_pyramid(s, np.zeros((Sc.CAM_T[5], Sc.CAM_T[4]), np.uint8))
    yield c
    c.close()


def stage(ctx, sts, keys=None, reserve=K.RESERVE, lm_reserve=K.LM_RESERVE):
    ctx.candidates_reserve(**reserve)
    ctx.candidates_reserve_landmarks(**lm_reserve)
    ctx.candidates_stage([Cc.to_job(st) for st in sts], K.CAM, K.CELL, K.SEG_CELL, K.BOUNDARY)
    ctx.candidates_set_quality([dict(pt_n_failed=st["pt_nfail"], pt_n_succeeded=st["pt_nsucc"], seg_n_failed=st["seg_nfail"], seg_n_succeeded=st["seg_nsucc"]) for st in sts])
    if keys is not None:
        ctx.candidates_set_last_optim([dict(pt_last_optim=k["pt"], seg_last_optim=k["seg"]) for k in keys])
    return [(c["pt"], c["seg"]) for c in ctx.candidates_lm_capacity()]


def check_all(ctx, sts, events, keys, tag):
    check_tables(ctx, sts, tag)
    for k, (q, o, st, ev, ky) in enumerate(zip(ctx.candidates_fetch_quality(), ctx.candidates_fetch_last_optim(), sts, events, keys)):
        for f, key in QUALITY:
            same_bytes(q[f], st[key], (tag, "quality", k, f))
        same_bytes(q["pt_event"], ev["pt"], (tag, "event", k, "pt")); same_bytes(q["seg_event"], ev["seg"], (tag, "event", k, "seg"))
        same_bytes(o["pt_last_optim"], ky["pt"], (tag, "key", k, "pt")); same_bytes(o["seg_last_optim"], ky["seg"], (tag, "key", k, "seg"))


def device_state(ctx):
    """the event bytes and keys as the device holds them, as the lists the restatement moves"""
    ev = [dict(pt=[int(v) for v in q["pt_event"]], seg=[int(v) for v in q["seg_event"]]) for q in ctx.candidates_fetch_quality()]
    ky = [dict(pt=[int(v) for v in o["pt_last_optim"]], seg=[int(v) for v in o["seg_last_optim"]]) for o in ctx.candidates_fetch_last_optim()]
    return ev, ky


def compact(ctx, cases, sts, rows, tag=""):
    """the compaction on the device and in the restatement (which mutates sts), all compared: tables, quality, events, keys, the report"""
    events, keys = device_state(ctx)
    ctx.candidates_compact([s["mode"] for s in cases])
    reps = [K.compact(s, st, r, events=ev, keys=ky) for s, st, r, ev, ky in zip(cases, sts, rows, events, keys)]
    check_all(ctx, sts, events, keys, tag)
    for k, (got, want) in enumerate(zip(ctx.candidates_compact_fetch(), reps)):
        assert {f: got[f] for f in NK.REPORT} == {f: want[f] for f in NK.REPORT}, (tag, k, got, want)
        same_bytes(got["pt_remap"], want["pt_remap"], (tag, "remap", k, "pt")); same_bytes(got["seg_remap"], want["seg_remap"], (tag, "remap", k, "seg"))
    return reps, events, keys


@pytest.mark.gpu
def test_compaction_equals_the_restatement_on_the_directed_cases(ctx, P):
    """twenty-six unequal streams: every size on both sides of the 64-lane round, every pattern of deleted rows, leftover and emptied
    lists, a list of 70 entries, candidate lists of 0 and 70, broken preconditions (pin 7), streams standing by, mode 2 on both sides of
    its threshold per kind.  A second compaction finds nothing to do and changes nothing"""
    cases = K.batch()
    sts = [copy.deepcopy(s["st"]) for s in cases]
    rows = stage(ctx, sts, [s["keys"] for s in cases])
    assert rows == [K.rows_of(st) for st in sts]
    reps, _, _ = compact(ctx, cases, sts, rows, "directed")
    assert sum(r["n_pt_before"] - r["n_pt_after"] for r in reps) > 500 and sum(r["n_seg_before"] - r["n_seg_after"] for r in reps) > 400
    assert sum(r["n_repointed_pt"] + r["n_repointed_seg"] for r in reps) >= 4 and sum(r["n_erased_pt_cand"] + r["n_erased_seg_cand"] for r in reps) == 6
    again = [dict(s, mode=(NK.ALWAYS, 0, 0)) if s["mode"][0] == NK.ALWAYS else dict(s, mode=(NK.STANDBY, 0, 0)) for s in cases]
    reps2, _, _ = compact(ctx, again, sts, rows, "a second compaction")
    assert all(r["n_pt_before"] == r["n_pt_after"] and r["n_seg_obs_before"] == r["n_seg_obs_after"] for r in reps2)


def grown_and_thinned(ctx, P):
    """the cases of the add, staged with room, then: add -> frame -> insertion with a removal.  Deleted rows arise the real way: the
    selection's safeDelete*, the insertion's safeDeleteFrame / removeFrameCandidates"""
    cases = Nc.batch()
    sts = [copy.deepcopy(s["st"]) for s in cases]
    rng = np.random.default_rng(8301)
    keys = [dict(pt=[int(v) for v in rng.integers(1, 500, len(st["pt_pos"]))], seg=[int(v) for v in rng.integers(1, 500, len(st["seg_spos"]))]) for st in sts]
    rows = stage(ctx, sts, keys, Nc.RESERVE, Nc.LM_RESERVE)
    ctx.candidates_add([Nc.records(s["new"]) for s in cases])
    for s, st in zip(cases, sts):
        Nc.add(s, st)
    _, _, sel = frame(ctx, P, cases, sts, tag="frame")
    remove = [Nc.removal_of(s, st) for s, st in zip(cases, sts)]
    insert(ctx, cases, sts, sel, [True] * len(cases), remove, tag="insertion")
    return cases, sts, rows


@pytest.mark.gpu
def test_compaction_behind_an_insertion_and_the_calls_behind_it_equal_a_fresh_stage(ctx, P):
    """deleted rows that arose the real way leave; then a frame, an add and an insertion on the compacted tables equal the restatement
    and equal, byte for byte, the same calls behind a fresh stage of the restatement's tables plus set_quality / set_last_optim"""
    cases, sts, rows = grown_and_thinned(ctx, P)
    n_dead = sum(st["pt_type"].count(N.TYPE_DELETED) + st["seg_type"].count(N.TYPE_DELETED) for st in sts)
    assert n_dead > 60
    cases = [dict(s, mode=(NK.ALWAYS, 0, 0)) for s in cases]
    reps, events, keys = compact(ctx, cases, sts, rows, "behind the insertion")
    assert sum(r["n_pt_before"] - r["n_pt_after"] + r["n_seg_before"] - r["n_seg_after"] for r in reps) == n_dead
    assert all(r["n_repointed_pt"] + r["n_repointed_seg"] + r["n_erased_pt_cand"] + r["n_erased_seg_cand"] == 0 for r in reps)   # the preconditions held
    cases = [K.remapped(s, r) for s, r in zip(cases, reps)]
    after = copy.deepcopy(sts)

    def follow(tables, tag):
        two = [Ic.second_frame_of(s, st, k) for k, (s, st) in enumerate(zip(cases, tables))]
        c1, s1, sel = frame(ctx, P, cases, tables, [t for t, _ in two], [o for _, o in two], tag=(tag, "frame"))
        more = Nc.second_new(cases, tables)
        ctx.candidates_add([Nc.records(s["new"]) for s in more])
        for s, st in zip(more, tables):
            Nc.add(s, st)
        added = ctx.candidates_add_fetch()
        check_tables(ctx, tables, (tag, "add"))
        ctx.candidates_run([P.abi.CandidateFrameJob(t, o, cur_slot=0) for t, o in two])
        return c1, s1, added, ctx.candidates_fetch(), ctx.candidates_fetch_map(), ctx.candidates_fetch_quality(), ctx.candidates_fetch_last_optim()

    a = follow(sts, "compacted")
    assert sum(g["n_matches"] for g in a[1]) > 100
    fresh = copy.deepcopy(after)
    stage(ctx, fresh, keys, Nc.RESERVE, Nc.LM_RESERVE)
    b = follow(fresh, "restaged")
    assert a[2] == b[2]
    for part in (0, 1, 3, 4, 5, 6):
        for k in range(len(cases)):
            for f in a[part][k]:
                if part == 5 and f.endswith("_event"):
                    continue                                          # (the restage starts without the events of the frames before it)
                same_bytes(b[part][k][f], a[part][k][f], ("restaged", part, k, f))


@pytest.mark.gpu
def test_an_insertion_behind_the_compaction_equals_the_restatement(ctx, P):
    cases, sts, rows = grown_and_thinned(ctx, P)
    cases = [dict(s, mode=(NK.ALWAYS, 0, 0)) for s in cases]
    reps, _, _ = compact(ctx, cases, sts, rows, "compaction")
    cases = [K.remapped(s, r) for s, r in zip(cases, reps)]
    two = [Ic.second_frame_of(s, st, k) for k, (s, st) in enumerate(zip(cases, sts))]
    _, _, sel = frame(ctx, P, cases, sts, [t for t, _ in two], [o for _, o in two], tag="frame behind the compaction")
    remove = [0 if len(st["kf_T"]) >= 2 else -1 for st in sts]
    insert(ctx, cases, sts, sel, [True] * len(cases), remove, tag="insertion behind the compaction")


@pytest.mark.gpu
def test_one_stream_at_a_time_equals_its_place_in_the_batch(ctx, P):
    cases = K.batch()
    sts = [copy.deepcopy(s["st"]) for s in cases]
    rows = stage(ctx, sts, [s["keys"] for s in cases])
    ctx.candidates_compact([s["mode"] for s in cases])
    whole = (ctx.candidates_fetch_map(), ctx.candidates_fetch_quality(), ctx.candidates_fetch_last_optim(), ctx.candidates_compact_fetch())
    for k in (0, 2, 3, 8, 10, 11, 15, 22):
        one = [copy.deepcopy(cases[k]["st"])]
        stage(ctx, one, [cases[k]["keys"]])
        ctx.candidates_compact([cases[k]["mode"]])
        alone = (ctx.candidates_fetch_map(), ctx.candidates_fetch_quality(), ctx.candidates_fetch_last_optim(), ctx.candidates_compact_fetch())
        for a, w in zip(alone, whole):
            for f in a[0]:
                same_bytes(a[0][f], w[k][f], ("alone", k, f))


@pytest.mark.gpu
def test_an_add_refused_for_capacity_passes_after_the_compaction_and_reuses_the_freed_rows(ctx, P):
    """behind an add, a frame and an insertion a stream has free landmark rows and deleted ones; one point more than the free rows
    converges: PLSVO_E_CAPACITY, nothing changed.  Mode 2 with that need as its threshold compacts the points of that stream only, the same
    add passes, and the rows it reuses read key 0 and counters 0 whatever the landmarks that left them held"""
    cases, sts, rows = grown_and_thinned(ctx, P)
    caps = ctx.candidates_capacity()
    pick = None
    for k, (st, r, cap) in enumerate(zip(sts, rows, caps)):
        free, n_dead = r[0] - len(st["pt_pos"]), st["pt_type"].count(N.TYPE_DELETED)
        cand_rows = len(cases[k]["st"]["pt_cand"]) + Nc.LM_RESERVE["extra_pt"]
        if st["kf_T"] and n_dead >= 3 and len(st["pt_cand"]) + free + 1 <= cand_rows and Ic.sizes(st)["n_pt_obs"] + free + 1 <= cap["pt_obs"]:
            pick = k
            break
    assert pick is not None
    st, free = sts[pick], rows[pick][0] - len(sts[pick]["pt_pos"])
    _, keys = device_state(ctx)
    new, fp, fs = Nc.make_new(np.random.default_rng(8402), cases[pick], st, free + 1, 0)
    recs = [Nc.records(new) if k == pick else None for k in range(len(cases))]
    before = ctx.candidates_fetch_map() + ctx.candidates_fetch_quality() + ctx.candidates_fetch_last_optim()
    with pytest.raises(P.capi.PlsvoError) as e:
        ctx.candidates_add(recs)
    assert e.value.code == P.abi.E_CAPACITY
    for a, b in zip(before, ctx.candidates_fetch_map() + ctx.candidates_fetch_quality() + ctx.candidates_fetch_last_optim()):
        for f in a:
            same_bytes(b[f], a[f], ("refused", f))
    modes = [dict(s, mode=(NK.ROOM, free + 1, 0) if k == pick else (NK.ROOM, 0, 0)) for k, s in enumerate(cases)]
    reps, events, keys2 = compact(ctx, modes, sts, rows, "room")
    assert [r["ran_pt"] for r in reps] == [int(k == pick) for k in range(len(cases))] and not any(r["ran_seg"] for r in reps)
    n_after, n_before = reps[pick]["n_pt_after"], reps[pick]["n_pt_before"]
    assert n_before - n_after >= 3 and any(v > 0 for v in keys[pick]["pt"][n_after:n_before])        # the rows that came free held keys
    ctx.candidates_add(recs)                                          # the same records: their keyframes have not moved
    r = Nc.NC.add(st, new)
    events[pick]["pt"] += r["pt_event"][n_after:]
    keys2[pick]["pt"] += [0] * (free + 1)
    assert st["pt_nfail"][n_after:] == [0] * (free + 1) and len(st["pt_pos"]) == n_after + free + 1
    check_all(ctx, sts, events, keys2, "add into the freed rows")
    got = ctx.candidates_add_fetch()[pick]
    assert (got["first_pt"], got["n_added_pt"], got["n_pt"]) == (n_after, free + 1, n_after + free + 1)


@pytest.mark.gpu
def test_a_seed_update_without_room_commits_when_repeated_after_the_compaction(ctx, P):
    """one observation entry short for the converged point seeds of the middle stream: its report says no_room and nothing of it changed.
    The compaction drops the observation lists its deleted landmarks left over; the repeated commit of the same rows finds the room on
    the device (seeds_commit_kernel reads the counts and the list ends there) and equals np_seedlist on the compacted tables.  The seed
    lists reference keyframes, not landmarks: the compaction leaves them byte for byte"""
    import np_seedlist as SL
    import seedlist_cases as Sl
    import test_gpu_seedlist as Ts
    cases = (Sl.batch()[11], Sl.batch()[7], Sl.batch()[9])
    left_over = sum(len(o) for o, t in zip(cases[1]["st"]["pt_obs"], cases[1]["st"]["pt_type"]) if t == N.TYPE_DELETED)
    assert left_over >= 1
    need = dict(extra_pt=sum(r["status"] == SL.CONVERGED for r in cases[1]["rows"]["pt"]), extra_seg=sum(r["status"] == SL.CONVERGED for r in cases[1]["rows"]["seg"]))
    reserve, lm_reserve = dict(extra_pt_obs=need["extra_pt"] - 1, extra_seg_obs=need["extra_seg"]), need
    sts, seeds = Ts.fresh(cases)
    Ts.stage(ctx, sts, seeds, reserve, lm_reserve)
    rooms = [Sl.room_of(c["st"], lm_reserve, reserve) for c in cases]
    reps = Ts.commit(ctx, cases, sts, seeds, rooms, "one entry short")
    assert [r["no_room"] for r in reps] == [0, 1, 0]
    lists = ctx.seeds_fetch_lists()
    modes = [dict(c, mode=(NK.ALWAYS, 0, 0) if k == 1 else (NK.STANDBY, 0, 0)) for k, c in enumerate(cases)]
    out, _, _ = compact(ctx, modes, sts, [(c["pt"], c["seg"]) for c in ctx.candidates_lm_capacity()], "compaction")
    assert out[1]["n_pt_obs_before"] - out[1]["n_pt_obs_after"] == left_over
    for a, b in zip(lists, ctx.seeds_fetch_lists()):
        for f in a:
            same_bytes(b[f], a[f], ("seed lists", f))
    again = (dict(cases[0], active=False), cases[1], dict(cases[2], active=False))
    reps = Ts.commit(ctx, again, sts, seeds, rooms, "repeated")
    assert [r["no_room"] for r in reps] == [0, 0, 0] and reps[1]["pt"][SL.CONVERGED] == need["extra_pt"] and reps[1]["first_pt"] == out[1]["n_pt_after"]


@pytest.mark.gpu
def test_compact_error_paths(P):
    c = P.capi.Context(0)
    try:
        _error_paths(c, P)
    finally:
        c.close()


def _error_paths(ctx, P):
    L, h, A = ctx.L, ctx.h, P.abi
    cases = Nc.batch()[6:9]
    sts = [copy.deepcopy(s["st"]) for s in cases]
    modes = lambda *m: (A.CandCompact * 3)(*[A.CandCompact(*v) for v in m])
    ok = modes((1, 0, 0, 0), (2, 3, 3, 0), (0, 0, 0, 0))
    assert L.plsvo_candidates_compact(h, 3, ok) == A.E_STATE and L.plsvo_candidates_compact_fetch(h, 3, (A.CandCompactOut * 3)()) == A.E_STATE   # before a stage
    ctx.config_pyramids(4, Sc.CAM_T[4], Sc.CAM_T[5], 3)
    for slot in range(4):
        ctx.build_pyramid(slot, np.zeros((Sc.CAM_T[5], Sc.CAM_T[4]), np.uint8))
    stage(ctx, sts, None, Nc.RESERVE, Nc.LM_RESERVE)
    snapshot = lambda: ctx.candidates_fetch_map() + ctx.candidates_fetch_quality() + ctx.candidates_fetch_last_optim()

    def same(before, tag):
        for a, b in zip(before, snapshot()):
            for f in a:
                same_bytes(b[f], a[f], (tag, f))
    assert L.plsvo_candidates_compact_fetch(h, 3, (A.CandCompactOut * 3)()) == A.E_STATE                 # no compaction since the stage
    ctx.candidates_run([A.CandidateFrameJob(s["T"], s["overlap"], cur_slot=0) for s in cases])
    want_c = [Sc.restate_candidates(s, st) for s, st in zip(cases, sts)]
    ctx.candidates_set_match([Sc.match_of(s, r) for s, r in zip(cases, want_c)])
    ctx.candidates_select(**Nc.PARAMS)
    before = snapshot()
    for name, bad in (("another n", None), ("NULL", None), ("unknown mode", modes((1, 0, 0, 0), (3, 0, 0, 0), (0, 0, 0, 0))), ("negative mode", modes((-1, 0, 0, 0), (1, 0, 0, 0), (0, 0, 0, 0))),
                      ("negative point threshold", modes((1, 0, 0, 0), (2, -1, 0, 0), (0, 0, 0, 0))), ("negative segment threshold", modes((1, 0, 0, 0), (0, 0, 0, 0), (2, 0, -4, 0)))):
        rc = L.plsvo_candidates_compact(h, 2, ok) if name == "another n" else L.plsvo_candidates_compact(h, 3, None) if name == "NULL" else L.plsvo_candidates_compact(h, 3, bad)
        assert rc == A.E_INVALID, name
    same(before, "invalid")
    assert L.plsvo_candidates_compact_fetch(h, 3, (A.CandCompactOut * 3)()) == A.E_STATE                 # (none of them counted as a compaction)
    assert L.plsvo_candidates_dev(h, C.byref(A.CandDev())) == A.OK                                       # ... nor ended the run
    # a compaction ends the open run; the run's fetches keep returning its results, in the old row numbers
    sel_before, cand_before = ctx.candidates_select_fetch(), ctx.candidates_fetch()
    ctx.candidates_compact([1, ("room", 3, 3), None])
    pr = A.CandSelectParams()
    pr.max_fts, pr.max_fts_segs, pr.poseopt_n_iter, pr.reproj_thresh = 120, 100, 10, 2.0
    ins = (A.CandInsert * 3)()
    keepm = np.ones(400, np.uint8)
    for a in ins:
        a.is_kf, a.remove_kf, a.kf_slot, a.pt_keep, a.seg_keep = 1, -1, 1, keepm.ctypes.data_as(A.c_u8_p), keepm.ctypes.data_as(A.c_u8_p)
    after = snapshot()
    assert L.plsvo_candidates_match(h) == A.E_STATE and L.plsvo_candidates_select(h, C.byref(pr)) == A.E_STATE and L.plsvo_candidates_pose_optimize(h) == A.E_STATE
    assert L.plsvo_candidates_set_match(h, 3, (A.CandMatchOut * 3)()) == A.E_STATE and L.plsvo_candidates_dev(h, C.byref(A.CandDev())) == A.E_STATE
    assert L.plsvo_candidates_insert_keyframe(h, 3, ins) == A.E_STATE
    same(after, "closed run")
    for a, b in zip(sel_before + cand_before, ctx.candidates_select_fetch() + ctx.candidates_fetch()):
        for f in a:
            same_bytes(b[f], a[f], ("the run's fetches", f))
    assert L.plsvo_candidates_compact_fetch(h, 2, (A.CandCompactOut * 3)()) == A.E_INVALID and L.plsvo_candidates_compact_fetch(h, 3, None) == A.E_INVALID
    assert len(ctx.candidates_compact_fetch()) == 3
    # the report is valid until the tables move again: an add, an insertion, a stage
    ctx.candidates_add([None, None, None])
    assert L.plsvo_candidates_compact_fetch(h, 3, (A.CandCompactOut * 3)()) == A.E_STATE
    ctx.candidates_compact([None, None, None])                        # legal behind an add; a compaction of nothing reports and ends the run all the same
    assert [r["ran_pt"] + r["ran_seg"] for r in ctx.candidates_compact_fetch()] == [0, 0, 0]
    ctx.candidates_run([A.CandidateFrameJob(s["T"], s["overlap"], cur_slot=0) for s in cases])
    ctx.candidates_compact([None, None, None])
    assert L.plsvo_candidates_match(h) == A.E_STATE
    stage(ctx, sts, None, Nc.RESERVE, Nc.LM_RESERVE)
    assert L.plsvo_candidates_compact_fetch(h, 3, (A.CandCompactOut * 3)()) == A.E_STATE


@pytest.mark.gpu
def test_compact_full_size_replicas(ctx, P):
    """1024 streams: 16 distinct tables x 64 replicas, every other stream compacts.  Every replica equals its first instance with the
    same choice, and the first thirty-two equal the restatement"""
    rng = np.random.default_rng(8501)
    base = [Ic.random_stream(rng, 8, 300, 120, 12, 6, remove_kf=-1) for _ in range(16)]
    for s in base:                                                    # a quarter of the rows deleted, beyond the few the builder made
        st = s["st"]
        for name in ("pt", "seg"):
            held = {lm for fts in st["kf_" + name] for lm in fts if lm >= 0}
            for lm in sorted(held)[::4]:
                st[name + "_type"][lm] = N.TYPE_DELETED
                for fts in st["kf_" + name]:
                    fts[:] = [-1 if v == lm else v for v in fts]
    reps = 64
    active = [(k + k // 16) % 2 == 0 for k in range(16 * reps)]
    ctx.candidates_reserve()
    ctx.candidates_reserve_landmarks()
    ctx.candidates_stage([Cc.to_job(s["st"]) for s in base] * reps, K.CAM, K.CELL, K.SEG_CELL, K.BOUNDARY)
    ctx.candidates_set_quality([dict(pt_n_failed=s["st"]["pt_nfail"], pt_n_succeeded=s["st"]["pt_nsucc"], seg_n_failed=s["st"]["seg_nfail"], seg_n_succeeded=s["st"]["seg_nsucc"])
                                for s in base] * reps)
    ctx.candidates_compact([1 if a else 0 for a in active])
    got, quality, report = ctx.candidates_fetch_map(), ctx.candidates_fetch_quality(), ctx.candidates_compact_fetch()
    assert sum(r["n_pt_before"] - r["n_pt_after"] for r in report[:16]) > 500
    for k in range(32):
        st = copy.deepcopy(base[k % 16]["st"])
        rep = NK.compact(st, NK.ALWAYS if active[k] else NK.STANDBY)
        want = Ic.tables(st)
        for f in want:
            same_bytes(got[k][f], want[f], ("full_size", k, f))
        for f, key in QUALITY:
            same_bytes(quality[k][f], st[key], ("full_size", k, f))
        assert {f: report[k][f] for f in NK.REPORT} == {f: rep[f] for f in NK.REPORT}, k
    for k in range(32, 16 * reps):
        first = k % 16 + (0 if active[k] == active[k % 16] else 16)
        for f in got[k]:
            same_bytes(got[k][f], got[first][f], (k, f))
        for f in quality[k]:
            same_bytes(quality[k][f], quality[first][f], (k, f))
        assert all(np.array_equal(report[k][f], report[first][f]) for f in report[k]), k
