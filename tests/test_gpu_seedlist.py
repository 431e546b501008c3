"""The depth filter's seed lists resident on the device (plsvo_seeds_*; pl-svo_amd/csrc/seedlist_device.hpp, update_seeds_resident_kernel)
against their restatement tests/np_seedlist.py on the cases of tests/seedlist_cases.py.  Everything is compared byte for byte, array by
array: the commit and the keyframe event copy and compute nothing, and the per-seed body is plsvo_update_seeds'.  The frames behind a
commit are driven with constructed match results, like those of tests/test_gpu_newcand.py, whose helpers run them."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest

import candidates_cases as Cc
import insert_cases as Ic
import newcand_cases as Nc
import np_seedlist as SL
import seedlist_cases as Sl
import select_cases as Sc
from test_gpu_insert import QUALITY, check_tables, frame, insert
from test_gpu_newcand import check_quality, set_quality, snapshot
from test_gpu_select import same_bytes

N_SLOTS = 12
REPORT = ("pt", "seg", "first_pt", "first_seg", "n_pt_seeds", "n_seg_seeds", "n_pt", "n_seg", "n_pt_cand", "n_seg_cand", "n_pt_obs", "n_seg_obs", "no_room", "batch_counter")


@pytest.fixture(scope="module")
def ctx(P):
    c = P.capi.Context(0)
    c.config_pyramids(N_SLOTS, Sc.CAM_T[4], Sc.CAM_T[5], 3)         # a keyframe's slot is its row in the cases' tables
    for s in range(N_SLOTS):
        c.build_pyramid(s, np.zeros((Sc.CAM_T[5], Sc.CAM_T[4]), np.uint8))
    yield c
    c.close()


def stage_maps(ctx, sts, reserve=Sl.RESERVE, lm_reserve=Sl.LM_RESERVE):
    ctx.candidates_reserve(**reserve)
    ctx.candidates_reserve_landmarks(**lm_reserve)
    ctx.candidates_stage([Cc.to_job(st) for st in sts], Sl.CAM, Sl.CELL, Sl.SEG_CELL, Sl.BOUNDARY)
    set_quality(ctx, sts)


def stage(ctx, sts, seeds, reserve=Sl.RESERVE, lm_reserve=Sl.LM_RESERVE, seed_reserve=Sl.SEED_RESERVE):
    stage_maps(ctx, sts, reserve, lm_reserve)
    ctx.seeds_reserve(**seed_reserve)
    ctx.seeds_stage([SL.lists_of(sd) for sd in seeds], Sl.CAM, max_n_kfs=Sl.MAX_N_KFS)


def check_lists(ctx, seeds, tag):
    got = ctx.seeds_fetch_lists()
    assert len(got) == len(seeds)
    for k, (g, sd) in enumerate(zip(got, seeds)):
        want = SL.lists_of(sd)
        assert g["batch_counter"] == want["batch_counter"], (tag, k)
        for f in want:
            if f != "batch_counter":
                same_bytes(g[f], want[f], (tag, "seeds", k, f))


def check_reports(got, want, tag):
    for k, (g, w) in enumerate(zip(got, want)):
        assert {f: g[f] for f in REPORT} == {f: w[f] for f in REPORT}, (tag, k, g, w)


def events_before(ctx):
    return [(list(q["pt_event"]), list(q["seg_event"])) for q in ctx.candidates_fetch_quality()]


def events_of(before, evs):
    """the event bytes behind a commit: the old landmarks' as they were, PLSVO_LM_EVENT_NEW for the new ones"""
    return [(b[0] + list(ev[0][len(b[0]):]) if ev[0] is not None else b[0], b[1] + list(ev[1][len(b[1]):]) if ev[1] is not None else b[1]) for b, ev in zip(before, evs)]


def commit(ctx, cases, sts, seeds, rooms, tag=""):
    """the commit of the cases' constructed rows on the device and in the restatement (which mutates sts and seeds), all compared: seed
    lists, map tables, quality, events, the report.  Returns the restatement's reports"""
    before = events_before(ctx)
    ctx.seeds_commit_rows([SL.rows_of(c["rows"]) if c["active"] else None for c in cases])
    got = ctx.seeds_update_fetch()
    res = [Sl.commit(c, sd, st, room) for c, sd, st, room in zip(cases, seeds, sts, rooms)]
    check_reports(got, [r for r, _ in res], tag)
    check_lists(ctx, seeds, tag)
    check_tables(ctx, sts, tag)
    check_quality(ctx, sts, events_of(before, [ev for _, ev in res]), tag)
    return [r for r, _ in res]


def converged_records(case):
    """the converged rows of a case as the records plsvo_candidates_add takes: what a caller of the host path packs"""
    new = dict(pt=[], seg=[])
    if case["active"]:
        for sd, row in zip(case["seeds"]["pt"], case["rows"]["pt"]):
            if row["status"] == SL.CONVERGED:
                new["pt"].append(dict(pos=row["xyz"], obs=dict(kf=sd["ref_kf"], px=sd["px"], f=sd["f"], level=sd["level"], type=sd["type"], grad=sd["grad"])))
        for sd, row in zip(case["seeds"]["seg"], case["rows"]["seg"]):
            if row["status"] == SL.CONVERGED:
                new["seg"].append(dict(spos=row["xyz_s"], epos=row["xyz_e"], obs=dict(kf=sd["ref_kf"], spx=sd["spx"], epx=sd["epx"], sf=sd["sf"], ef=sd["ef"], level=sd["level"])))
    return Nc.records(new)


def fresh(cases):
    return [copy.deepcopy(c["st"]) for c in cases], [copy.deepcopy(c["seeds"]) for c in cases]


@pytest.mark.gpu
def test_commit_of_constructed_rows_equals_the_restatement_and_the_host_path(ctx, P):
    """thirteen unequal streams: 0, 1, 63, 64, 65 and 130 converged rows per kind, converged rows between aged, NaN and kept ones in a round
    and across rounds, every row converged, every row aged, empty lists, an inactive stream, one without keyframes.  Lists, tables, quality,
    events and reports are the restatement's; the tables are, byte for byte, those the host path of the same tree builds from the same
    rows (plsvo_candidates_add); the next frame runs on them"""
    cases = Sl.batch()
    conv = [(sum(r["status"] == SL.CONVERGED for r in c["rows"]["pt"]), sum(r["status"] == SL.CONVERGED for r in c["rows"]["seg"])) if c["active"] else (0, 0) for c in cases]
    assert {0, 1, 63, 64, 65, 130} <= {a for a, _ in conv} and {0, 1, 63, 64, 65, 130} <= {b for _, b in conv}
    sts, seeds = fresh(cases)
    stage(ctx, sts, seeds)
    check_lists(ctx, seeds, "staged")
    reps = commit(ctx, cases, sts, seeds, [Sl.room_of(c["st"]) for c in cases], "commit")
    assert not any(r["no_room"] for r in reps) and [(r["pt"][SL.CONVERGED], r["seg"][SL.CONVERGED]) for r in reps] == conv
    assert reps[5]["n_pt_seeds"] == 5 and sum(reps[5]["pt"]) == 0                                          # the inactive stream kept its lists
    resident = snapshot(ctx)
    frame(ctx, P, cases, sts, tag="frame on the grown tables")
    host, _ = fresh(cases)
    stage_maps(ctx, host)
    ctx.candidates_add([converged_records(c) for c in cases])
    for a, b in zip(resident, snapshot(ctx)):
        for f in a:
            same_bytes(b[f], a[f], ("host path", f))


def run_update(ctx, cases, sts, seeds, rooms, active=None, tag=""):
    """plsvo_seeds_update with every stream's own frame on the (all-zero) pyramids: the body's rows are the device's own
    (plsvo_seeds_fetch_rows; tests on images compare them with plsvo_update_seeds), everything around the body is the restatement's -- the
    age test, the erasing, the hand-over, the report"""
    active = [True] * len(cases) if active is None else active
    before = events_before(ctx)
    ctx.seeds_update([dict(cur_slot=1, T_f_w=c["T"]) if a else None for c, a in zip(cases, active)])
    got = ctx.seeds_update_fetch()
    rows = ctx.seeds_fetch_rows()
    reps, evs = [], []
    for k, (c, sd, st, room, a, r) in enumerate(zip(cases, seeds, sts, rooms, active, rows)):
        if not a:
            reps.append(SL.report_of(sd, st)); evs.append((None, None))
            continue
        it = dict(pt=iter(range(len(sd["pt"]))), seg=iter(range(len(sd["seg"]))))
        assert len(r["pt_status"]) == len(sd["pt"]) and len(r["seg_status"]) == len(sd["seg"]), (tag, k)

        def body(kind, seed, r=r, sd=sd, it=it):
            j = next(i for i in it[kind] if not SL.aged(sd, sd[kind][i], Sl.MAX_N_KFS))
            assert r[kind + "_status"][j] != SL.AGED, (tag, kind, j)
            names = SL.PT_ROWS if kind == "pt" else SL.SEG_ROWS
            return {key: (int(r[f][j]) if key == "status" else r[f][j].tolist() if key.startswith("xyz") else r[f][j]) for f, key in names}
        n_aged = [sum(SL.aged(sd, x, Sl.MAX_N_KFS) for x in sd[kind]) for kind in ("pt", "seg")]
        rep, ev, _ = SL.update(sd, st, body, Sl.MAX_N_KFS, room)
        assert [rep["pt"][SL.AGED], rep["seg"][SL.AGED]] == n_aged and [int((r["pt_status"] == SL.AGED).sum()), int((r["seg_status"] == SL.AGED).sum())] == n_aged, (tag, k)
        reps.append(rep); evs.append(ev)
    check_reports(got, reps, tag)
    check_lists(ctx, seeds, tag)
    check_tables(ctx, sts, tag)
    check_quality(ctx, sts, events_of(before, evs), tag)
    return reps


@pytest.mark.gpu
def test_capacity_short_streams_are_dropped_whole_and_their_neighbours_commit(ctx, P):
    """room exactly sufficient commits; one short in each of the four kinds flags the short stream, leaves its seed lists and its map tables
    byte for byte what they were and commits its neighbours; after a restage with room the repeated commit equals the restatement"""
    cases = (Sl.batch()[11], Sl.batch()[7], Sl.batch()[9])            # stream 7: converged rows between the others across rounds
    need = dict(extra_pt=sum(r["status"] == SL.CONVERGED for r in cases[1]["rows"]["pt"]), extra_seg=sum(r["status"] == SL.CONVERGED for r in cases[1]["rows"]["seg"]))
    assert need["extra_pt"] > 40 and need["extra_seg"] > 20 and need["extra_pt"] > sum(r["status"] == SL.CONVERGED for r in cases[0]["rows"]["pt"])
    need.update(extra_pt_obs=need["extra_pt"], extra_seg_obs=need["extra_seg"])
    for short in (None,) + tuple(need):
        room = dict(need)
        if short:
            room[short] -= 1
        sts, seeds = fresh(cases)
        reserve, lm_reserve = dict(extra_pt_obs=room["extra_pt_obs"], extra_seg_obs=room["extra_seg_obs"]), dict(extra_pt=room["extra_pt"], extra_seg=room["extra_seg"])
        stage(ctx, sts, seeds, reserve, lm_reserve)
        before = (ctx.candidates_fetch_map()[1], ctx.candidates_fetch_quality()[1], ctx.seeds_fetch_lists()[1])
        reps = commit(ctx, cases, sts, seeds, [Sl.room_of(c["st"], lm_reserve, reserve) for c in cases], ("room", short))
        assert [r["no_room"] for r in reps] == [0, 1 if short else 0, 0], short
        assert reps[0]["pt"][SL.CONVERGED] + reps[0]["seg"][SL.CONVERGED] > 0                                 # a neighbour that hands seeds over
        if short is None:
            continue
        after = (ctx.candidates_fetch_map()[1], ctx.candidates_fetch_quality()[1], ctx.seeds_fetch_lists()[1])
        for a, b in zip(before, after):
            for f in a:
                same_bytes(b[f], a[f], ("short stream", short, f))
        # the caller restages with room and repeats: the tables and lists as they stand, the same rows for the stream that was dropped
        again = (dict(cases[0], active=False), cases[1], dict(cases[2], active=False))
        stage(ctx, sts, seeds)
        reps = commit(ctx, again, sts, seeds, [Sl.room_of(st) for st in sts], ("repeated", short))
        assert [r["no_room"] for r in reps] == [0, 0, 0] and reps[1]["pt"][SL.CONVERGED] == need["extra_pt"]


@pytest.mark.gpu
def test_keyframe_events_equal_the_restatement_and_a_new_batch_ages_seeds_out(ctx, P):
    """removal of the first, a middle and the last keyframe and none; new batches; appends of 0, 1, 64 and 65 seeds per kind; then an
    update: the seeds the new batch made too old are erased unsearched, the others take the body's result"""
    cases = Sl.batch()
    sts, seeds = fresh(cases)
    stage(ctx, sts, seeds)
    rng = np.random.default_rng(7202)
    n_kf = [len(st["kf_T"]) for st in sts]
    assert n_kf[3] == 5 and n_kf[4] == 6 and n_kf[0] == 4
    plan = {0: dict(removed_kf=0, new_batch=True, n=(1, 64)), 2: dict(removed_kf=-1, new_batch=True, n=(64, 1)), 3: dict(removed_kf=2, new_batch=True, n=(65, 0)),
            4: dict(removed_kf=5, new_batch=False, n=(0, 65)), 7: dict(removed_kf=1, new_batch=True, n=(0, 0)), 9: dict(removed_kf=-1, new_batch=False, n=(3, 2)),
            11: dict(removed_kf=-1, new_batch=True, n=(0, 0)), 12: dict(removed_kf=2, new_batch=False, n=(0, 0))}
    events = []
    for k, (c, st) in enumerate(zip(cases, sts)):
        if k not in plan:
            events.append(None)
            continue
        p = plan[k]
        pt, seg = Sl.new_features(rng, st, c, *p["n"])
        # (the map tables themselves do not change here: the removed index only has to lie in the table; the seeds of a removed last
        #  keyframe go, a new seed refers to the last row that is left)
        events.append(dict(removed_kf=p["removed_kf"], new_batch=p["new_batch"], new_kf=n_kf[k] - 1, depth_mean=2.5 + k / 8, depth_min=0.75 + k / 16, new_pt=pt, new_seg=seg))
    before = [(len(sd["pt"]), len(sd["seg"])) for sd in seeds]
    ctx.seeds_keyframe([Sl.kf_event_of(e) for e in events])
    for sd, e in zip(seeds, events):
        if e:
            SL.keyframe(sd, **e)
    check_lists(ctx, seeds, "keyframe event")
    assert any(len(sd["pt"]) < b[0] for sd, b in zip(seeds, before)) and any(len(sd["seg"]) < b[1] + len(e["new_seg"]) for sd, b, e in zip(seeds, before, events) if e)
    aged = sum(SL.aged(sd, x, Sl.MAX_N_KFS) for sd in seeds for kind in ("pt", "seg") for x in sd[kind])
    assert aged > 40                                                  # batch ids that were at the limit before the new batch
    reps = run_update(ctx, cases, sts, seeds, [Sl.room_of(c["st"]) for c in cases], tag="update behind the events")
    assert sum(r["pt"][SL.AGED] + r["seg"][SL.AGED] for r in reps) == aged
    # a second event on the lists as they stand (the mirrors are exact again), and an update on them
    ctx.seeds_keyframe([dict(new_batch=True) if st["kf_T"] else None for st in sts])
    for sd, st in zip(seeds, sts):
        if st["kf_T"]:
            SL.keyframe(sd, new_batch=True)
    check_lists(ctx, seeds, "second event")
    run_update(ctx, cases, sts, seeds, [Sl.room_of(c["st"]) for c in cases], active=[k % 3 != 1 for k in range(len(cases))], tag="second update")


@pytest.mark.gpu
def test_keyframe_capacity_is_decided_before_anything_changes(ctx, P):
    cases = Sl.batch()[6:9]
    rng = np.random.default_rng(7203)
    for extra, ok in ((dict(extra_pt=64, extra_seg=65), True), (dict(extra_pt=63, extra_seg=65), False), (dict(extra_pt=64, extra_seg=64), False)):
        sts, seeds = fresh(cases)
        stage(ctx, sts, seeds, seed_reserve=extra)
        assert ctx.seeds_capacity() == [dict(pt=len(sd["pt"]) + extra["extra_pt"], seg=len(sd["seg"]) + extra["extra_seg"]) for sd in seeds]
        pt, seg = Sl.new_features(rng, sts[1], cases[1], 64, 65)
        events = [dict(new_batch=True, new_kf=0, depth_mean=2.0, depth_min=1.0, new_pt=pt[:3], new_seg=[]), dict(new_batch=True, new_kf=1, depth_mean=3.0, depth_min=0.5, new_pt=pt, new_seg=seg), None]
        if ok:
            ctx.seeds_keyframe([Sl.kf_event_of(e) for e in events])
            for sd, e in zip(seeds, events):
                if e:
                    SL.keyframe(sd, **e)
        else:
            with pytest.raises(P.capi.PlsvoError) as e:
                ctx.seeds_keyframe([Sl.kf_event_of(e) for e in events])
            assert e.value.code == P.abi.E_CAPACITY
        check_lists(ctx, seeds, ("keyframe capacity", ok))


@pytest.mark.gpu
def test_update_directly_behind_an_insertion_with_removal_then_the_keyframe_event(ctx, P):
    """the order of a keyframe in the pipeline: frame -> selection -> insertion (a keyframe leaves, the table closes up) -> seed update on
    the same run -> keyframe event (the removed keyframe's seeds go, the others are renumbered, the new keyframe's seeds start)"""
    cases = [c for c in Sl.batch() if c["st"]["kf_T"] and c["is_kf"]]
    sts, seeds = fresh(cases)
    stage(ctx, sts, seeds)
    _, _, sel = frame(ctx, P, cases, sts, tag="frame")
    remove = [Nc.removal_of(c, st) for c, st in zip(cases, sts)]
    insert(ctx, cases, sts, sel, [True] * len(cases), remove, tag="insertion")
    rooms = [Sl.room_of(c["st"]) for c in cases]
    run_update(ctx, cases, sts, seeds, rooms, tag="update behind the insertion")
    rng = np.random.default_rng(7204)
    events = []
    for c, st, r in zip(cases, sts, remove):
        pt, seg = Sl.new_features(rng, st, c, 5, 3)
        for f in pt + seg:
            f.pop("kf", None)
        events.append(dict(removed_kf=r, new_batch=True, new_kf=len(st["kf_T"]) - 1, depth_mean=3.0, depth_min=1.5, new_pt=pt, new_seg=seg))
    ctx.seeds_keyframe([Sl.kf_event_of(e) for e in events])
    for sd, e in zip(seeds, events):
        SL.keyframe(sd, **e)
    check_lists(ctx, seeds, "event behind the insertion")
    assert all(x["ref_kf"] < len(st["kf_T"]) for sd, st in zip(seeds, sts) for kind in ("pt", "seg") for x in sd[kind])
    two = [Ic.second_frame_of(c, st, k) for k, (c, st) in enumerate(zip(cases, sts))]
    frame(ctx, P, cases, sts, [t for t, _ in two], [o for _, o in two], tag="frame behind the event")
    run_update(ctx, cases, sts, seeds, rooms, tag="update on the new table")


@pytest.mark.gpu
def test_one_stream_at_a_time_equals_its_place_in_the_batch(ctx, P):
    cases = Sl.batch()
    sts, seeds = fresh(cases)
    stage(ctx, sts, seeds)
    ctx.seeds_commit_rows([SL.rows_of(c["rows"]) if c["active"] else None for c in cases])
    report = ctx.seeds_update_fetch()
    whole, quality, lists = ctx.candidates_fetch_map(), ctx.candidates_fetch_quality(), ctx.seeds_fetch_lists()
    for k in (0, 2, 5, 7, 10, 12):
        one, sd = fresh(cases[k:k + 1])
        stage(ctx, one, sd)
        ctx.seeds_commit_rows([SL.rows_of(cases[k]["rows"]) if cases[k]["active"] else None])
        assert ctx.seeds_update_fetch()[0] == report[k]
        for got, want in ((ctx.candidates_fetch_map()[0], whole[k]), (ctx.candidates_fetch_quality()[0], quality[k]), (ctx.seeds_fetch_lists()[0], lists[k])):
            for f in want:
                same_bytes(got[f], want[f], ("alone", k, f))


@pytest.mark.gpu
def test_seed_protocol_and_error_paths(P):
    L_ctx = P.capi.Context(0)
    try:
        _protocol(L_ctx, P)
    finally:
        L_ctx.close()


def _protocol(ctx, P):
    L, h, A = ctx.L, ctx.h, P.abi
    cases = Sl.batch()[6:9]
    sts, seeds = fresh(cases)
    pr = A.SeedParams()
    pr.cam = A.Pinhole(*Sl.CAM) if not isinstance(Sl.CAM, A.Pinhole) else Sl.CAM
    pr.n_pyr_levels, pr.align_max_iter, pr.max_epi_search_steps, pr.edgelet_filtering, pr.edgelet_max_angle, pr.px_noise, pr.convergence_sigma2_thresh, pr.max_n_kfs = 3, 10, 1000, 1, 0.7, 1.0, 200.0, 3
    none = (A.SeedList * 3)()
    assert L.plsvo_seeds_stage(h, 3, C.byref(pr), none) == A.E_STATE                                       # no candidate tables
    stage_maps(ctx, sts)
    assert L.plsvo_seeds_stage(h, 3, C.byref(pr), none) == A.E_STATE                                       # no pyramids
    ctx.config_pyramids(N_SLOTS, Sc.CAM_T[4], Sc.CAM_T[5], 3)
    for slot in range(N_SLOTS):
        ctx.build_pyramid(slot, np.zeros((Sc.CAM_T[5], Sc.CAM_T[4]), np.uint8))
    assert L.plsvo_seeds_stage(h, 2, C.byref(pr), none) == A.E_STATE                                       # another n than the candidate tables
    assert L.plsvo_seeds_update(h, 3, (A.SeedFrame * 3)()) == A.E_STATE and L.plsvo_seeds_fetch_lists(h, 3, (A.SeedList * 3)()) == A.E_STATE   # before a stage
    assert L.plsvo_seeds_reserve(h, C.byref(A.SeedReserve(-1, 0))) == A.E_INVALID and L.plsvo_seeds_reserve(h, C.byref(A.SeedReserve(0, -1))) == A.E_INVALID
    assert L.plsvo_seeds_stage(h, 3, None, none) == A.E_INVALID and L.plsvo_seeds_stage(h, 3, C.byref(pr), None) == A.E_INVALID

    def build(mutate):
        """the lists of the three streams as ctypes, stream 1's changed by `mutate(dict of arrays, struct)`"""
        arr, keep = (A.SeedList * 3)(), []
        for k, (a, sd) in enumerate(zip(arr, seeds)):
            d = SL.lists_of(sd)
            a.batch_counter = d.pop("batch_counter")
            d = {f: np.ascontiguousarray(d[f], dtype=A._SEED_CT[t][1]) for f, t, _ in A._SEED_LIST_FIELDS}
            a.n_pt, a.n_seg = len(d["pt_ref_kf"]), len(d["seg_ref_kf"])
            if k == 1:
                mutate(d, a)
            for f, t, _ in A._SEED_LIST_FIELDS:
                if d[f] is not None and d[f].size:
                    keep.append(d[f])
                    setattr(a, f, d[f].ctypes.data_as(A._SEED_CT[t][0]))
        return arr, keep

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
    n_kf = len(sts[1]["kf_T"])
    assert any(x["type"] == 1 for x in seeds[1]["pt"])
    invalid = [("negative point count", count("n_pt", -1)), ("negative segment count", count("n_seg", -2)), ("ref_kf == n_kf", set_at("pt_ref_kf", 129, n_kf)),
               ("negative ref_kf", set_at("seg_ref_kf", 0, -1)), ("level outside the pyramid", set_at("pt_level", 5, 3)), ("negative level", set_at("seg_level", 64, -1)),
               ("unknown feature type", set_at("pt_type", 77, 2)), ("edgelets without gradients under edgelet filtering", drop("pt_grad"))]
    invalid += [("null " + f, drop(f)) for f, _, _ in A._SEED_LIST_FIELDS if f != "pt_grad"]
    for name, mutate in invalid:
        arr, keep = build(mutate)
        assert L.plsvo_seeds_stage(h, 3, C.byref(pr), arr) == A.E_INVALID, name
    assert L.plsvo_seeds_fetch_lists(h, 3, (A.SeedList * 3)()) == A.E_STATE                                 # (none of them staged anything)
    arr, keep = build(lambda d, a: None)
    assert L.plsvo_seeds_stage(h, 3, C.byref(pr), arr) == A.OK
    ctx._seed_n = 3
    check_lists(ctx, seeds, "staged through ctypes")
    # -- update: every argument check
    fr = (A.SeedFrame * 3)()
    for a in fr:
        a.active, a.cur_slot, a.pose_source = 1, 1, A.INSERT_POSE_HOST
        a.T_f_w = (C.c_double * 7)(0, 0, 0, 1, 0, 0, 0)
    assert L.plsvo_seeds_update(h, 2, fr) == A.E_INVALID and L.plsvo_seeds_update(h, 3, None) == A.E_INVALID
    for f, v, code in (("cur_slot", -1, A.E_INVALID), ("cur_slot", N_SLOTS, A.E_INVALID), ("pose_source", 3, A.E_INVALID), ("pose_source", A.INSERT_POSE_DEV, A.E_INVALID),
                       ("pose_source", A.INSERT_POSE_RESIDENT, A.E_STATE)):
        old = getattr(fr[1], f)
        setattr(fr[1], f, v)
        assert L.plsvo_seeds_update(h, 3, fr) == code, (f, v)
        setattr(fr[1], f, old)
    assert L.plsvo_seeds_update_fetch(h, 3, (A.SeedReport * 3)()) == A.E_STATE and L.plsvo_seeds_fetch_rows(h, 3, (A.SeedRows * 3)()) == A.E_STATE   # no update yet
    # -- keyframe: every argument check, nothing written
    ev = (A.SeedKf * 3)()
    for a in ev:
        a.removed_kf = -1
    for f, v in (("removed_kf", -2), ("removed_kf", n_kf + 1), ("n_pt", -1), ("n_seg", -1)):
        old = getattr(ev[1], f)
        setattr(ev[1], f, v)
        assert L.plsvo_seeds_keyframe(h, 3, ev) == A.E_INVALID, (f, v)
        setattr(ev[1], f, old)
    pt, seg = Sl.new_features(np.random.default_rng(1), sts[1], cases[1], 3, 2)
    good = dict(new_kf=0, depth_mean=2.0, depth_min=1.0, new_pt=pt, new_seg=seg)
    for name, bad in (("new_kf == n_kf", dict(good, new_kf=n_kf)), ("negative new_kf", dict(good, new_kf=-1)), ("depth_min 0", dict(good, depth_min=0.0)),
                      ("negative depth_mean", dict(good, depth_mean=-1.0)), ("level outside the pyramid", dict(good, new_pt=[dict(pt[0], level=3)] + pt[1:])),
                      ("unknown type", dict(good, new_pt=[dict(pt[0], type=2)] + pt[1:]))):
        with pytest.raises(P.capi.PlsvoError) as e:
            ctx.seeds_keyframe([None, Sl.kf_event_of(bad), None])
        assert e.value.code == A.E_INVALID, name
    check_lists(ctx, seeds, "refused events")
    # -- between an update and its fetch the candidate tables are the device's alone; the closed run's fetches keep working
    ctx.candidates_run([A.CandidateFrameJob(s["T"], s["overlap"], cur_slot=0) for s in cases])
    ctx.candidates_set_match([Ic.frame(s, st)[1] for s, st in zip(cases, sts)])                           # (the restatement's frame: its selection shortens the lists)
    ctx.candidates_select(**Nc.PARAMS)
    sel_before, cand_before = ctx.candidates_select_fetch(), ctx.candidates_fetch()
    tables_before = snapshot(ctx)
    ctx.seeds_commit_rows([SL.rows_of(c["rows"]) for c in cases])
    sp = A.CandSelectParams()
    sp.max_fts, sp.max_fts_segs, sp.poseopt_n_iter, sp.reproj_thresh = 120, 100, 10, 2.0
    ins = (A.CandInsert * 3)()
    keepm = np.ones(400, np.uint8)
    for a in ins:
        a.is_kf, a.remove_kf, a.kf_slot, a.pt_keep, a.seg_keep = 1, -1, 1, keepm.ctypes.data_as(A.c_u8_p), keepm.ctypes.data_as(A.c_u8_p)
    frames = (A.CandFrame * 3)(*[A.CandidateFrameJob(s["T"], s["overlap"], cur_slot=0).c for s in cases])
    refused = dict(run=L.plsvo_candidates_run(h, 3, frames), match=L.plsvo_candidates_match(h), set_match=L.plsvo_candidates_set_match(h, 3, (A.CandMatchOut * 3)()),
                   select=L.plsvo_candidates_select(h, C.byref(sp)), pose_optimize=L.plsvo_candidates_pose_optimize(h), dev=L.plsvo_candidates_dev(h, C.byref(A.CandDev())),
                   insert=L.plsvo_candidates_insert_keyframe(h, 3, ins), add=L.plsvo_candidates_add(h, 3, (A.CandNew * 3)()), add_fetch=L.plsvo_candidates_add_fetch(h, 3, (A.CandAddOut * 3)()),
                   set_quality=L.plsvo_candidates_set_quality(h, 3, (A.CandQualityIn * 3)()), fetch_quality=L.plsvo_candidates_fetch_quality(h, 3, (A.CandQualityOut * 3)()),
                   fetch_map=L.plsvo_candidates_fetch_map(h, 3, (A.CandMapOut * 3)()), set_positions=L.plsvo_candidates_set_positions(h, 3, (A.CandPositions * 3)()),
                   seeds_keyframe=L.plsvo_seeds_keyframe(h, 3, ev), seeds_fetch_lists=L.plsvo_seeds_fetch_lists(h, 3, (A.SeedList * 3)()),
                   seeds_update=L.plsvo_seeds_update(h, 3, fr), seeds_stage=L.plsvo_seeds_stage(h, 3, C.byref(pr), arr))
    assert all(rc == A.E_STATE for rc in refused.values()), refused
    for a, b in zip(sel_before + cand_before, ctx.candidates_select_fetch() + ctx.candidates_fetch()):      # the run's results, as they were
        for f in a:
            same_bytes(b[f], a[f], ("the run's fetches", f))
    reps = ctx.seeds_update_fetch()
    assert reps == ctx.seeds_update_fetch()                                                                 # a second fetch returns the same report
    want = [Sl.commit(c, sd, st, Sl.room_of(c["st"])) for c, sd, st in zip(cases, seeds, sts)]
    check_reports(reps, [r for r, _ in want], "fetched")
    check_tables(ctx, sts, "fetched"); check_lists(ctx, seeds, "fetched")
    assert any(not np.array_equal(a[f], b[f]) for a, b in zip(tables_before, snapshot(ctx)) for f in a)   # (the refused calls wrote nothing; the commit did)
    # the update ended the open run, as an add does
    assert L.plsvo_candidates_match(h) == A.E_STATE and L.plsvo_candidates_select(h, C.byref(sp)) == A.E_STATE
    ctx.candidates_run([A.CandidateFrameJob(s["T"], s["overlap"], cur_slot=0) for s in cases])
    assert L.plsvo_candidates_dev(h, C.byref(A.CandDev())) == A.OK
    # a candidate restage drops the seed tables: the caller restages both
    stage_maps(ctx, sts)
    for rc in (L.plsvo_seeds_update(h, 3, fr), L.plsvo_seeds_keyframe(h, 3, ev), L.plsvo_seeds_fetch_lists(h, 3, (A.SeedList * 3)()), L.plsvo_seeds_update_fetch(h, 3, (A.SeedReport * 3)()),
               L.plsvo_seeds_commit_rows(h, 3, (A.SeedRows * 3)()), L.plsvo_seeds_capacity(h, 3, (A.SeedReserve * 3)())):
        assert rc == A.E_STATE
    ctx.seeds_stage([SL.lists_of(sd) for sd in seeds], Sl.CAM, max_n_kfs=Sl.MAX_N_KFS)
    check_lists(ctx, seeds, "restaged")


@pytest.mark.gpu
def test_commit_full_size_replicas(ctx, P):
    """1024 streams: 16 distinct streams x 64 replicas, every other one active.  Every replica equals its first instance with the same
    choice, and the first thirty-two equal the restatement"""
    rng = np.random.default_rng(7205)
    base = [Ic.random_stream(rng, 10, 300, 120, 12, 6, remove_kf=-1) for _ in range(16)]
    cases = [Sl.make_case(rng, s, s["st"], int(rng.integers(1, 140)), int(rng.integers(1, 140)), "mixed", k) for k, s in enumerate(base)]
    reps = 64
    active = [(k + k // 16) % 2 == 0 for k in range(16 * reps)]
    ctx.candidates_reserve(extra_pt_obs=140, extra_seg_obs=140)
    ctx.candidates_reserve_landmarks(extra_pt=140, extra_seg=140)
    ctx.candidates_stage([Cc.to_job(s["st"]) for s in base] * reps, Sl.CAM, Sl.CELL, Sl.SEG_CELL, Sl.BOUNDARY)
    set_quality(ctx, [s["st"] for s in base] * reps)
    ctx.seeds_reserve()
    ctx.seeds_stage([SL.lists_of(c["seeds"]) for c in cases] * reps, Sl.CAM, max_n_kfs=Sl.MAX_N_KFS)
    rows = [SL.rows_of(c["rows"]) for c in cases]
    ctx.seeds_commit_rows([rows[k % 16] if active[k] else None for k in range(16 * reps)])
    report = ctx.seeds_update_fetch()
    got, quality, lists = ctx.candidates_fetch_map(), ctx.candidates_fetch_quality(), ctx.seeds_fetch_lists()
    for k in range(32):
        st, sd = copy.deepcopy(base[k % 16]["st"]), copy.deepcopy(cases[k % 16]["seeds"])
        rep, ev = Sl.commit(dict(cases[k % 16], active=active[k]), sd, st)
        assert {f: report[k][f] for f in REPORT} == {f: rep[f] for f in REPORT}, k
        want = Ic.tables(st)
        for f in want:
            same_bytes(got[k][f], want[f], ("full_size", k, f))
        for f, key in QUALITY:
            same_bytes(quality[k][f], st[key], ("full_size", k, f))
        ev = events_of([([0] * len(base[k % 16]["st"]["pt_pos"]), [0] * len(base[k % 16]["st"]["seg_spos"]))], [ev])[0]
        same_bytes(quality[k]["pt_event"], ev[0], ("full_size", k)); same_bytes(quality[k]["seg_event"], ev[1], ("full_size", k))
        for f, v in SL.lists_of(sd).items():
            if f != "batch_counter":
                same_bytes(lists[k][f], v, ("full_size", k, f))
    for k in range(32, 16 * reps):
        first = k % 16 + (0 if active[k] == active[k % 16] else 16)
        assert report[k] == report[first], k
        for a, b in ((got[k], got[first]), (quality[k], quality[first]), (lists[k], lists[first])):
            for f in a:
                same_bytes(a[f], b[f], (k, f))


# ---- the update on images: plsvo_update_seeds' body on the resident rows ---------------------------------------------------------------------
def _image_case(P, ob):
    """seeds over a 320 x 240 sequence (sequence.make_sequence, synth.make_seeds) with the inputs of tests/test_depth_filter.py's edge cases,
    where the oracle makes point and line seeds converge: tight seeds at the true depth, a bearing behind the camera, NaN variances, a seed a
    kilometre away.  Four streams share the three images: both kinds with frame 0 as the FIRST keyframe, points only with frame 0 as the
    LAST keyframe, segments only with one keyframe, and one that is not active"""
    seqm = importlib.import_module("pl-svo_amd.sequence")
    seq = seqm.make_sequence(26, n_frames=3, W=320, H=240, n_pts=70, n_seg=10, step_scale=1.0)
    frames = [ob.build_pyramid(im, 4) for im in seq["images"]]
    pt, seg, truth = P.synth.make_seeds(seq, cur_frame=2)
    n, ns = len(pt["px"]), len(seg["px"])
    pt["f"] = pt["f"].copy()
    pt["f"][0] = [0.0, 0.0, -1.0]
    for i in [1] + list(range(8, n, 5)):
        pt["sigma2"][i], pt["mu"][i] = 1e-8, 1.0 / truth["pt_depth"][i]
    pt["sigma2"][2] = np.nan
    pt["mu"][3], pt["sigma2"][3] = 1e-3, 1e-10
    for i in range(0, ns, 2):
        seg["sigma2_s"][i] = seg["sigma2_e"][i] = 1e-8
        seg["mu_s"][i], seg["mu_e"][i] = 1.0 / truth["seg_sdepth"][i], 1.0 / truth["seg_edepth"][i]
    seg["sigma2_s"][1] = np.nan
    ro = ob.update_seeds(P.abi.SeedsJob(seq["cam"], seq["poses_true"], np.arange(3), pt, seg), frames)
    assert (ro["pt_status"] == SL.CONVERGED).sum() >= 3 and (ro["seg_status"] == SL.CONVERGED).sum() >= 2   # a condition on the inputs: the oracle's verdict
    f32 = np.float32

    def seeds_of(ref_kf, points, segments, counter=7):
        sd = dict(pt=[], seg=[], batch_counter=counter)
        for i in (range(n) if points else ()):
            sd["pt"].append(dict(ref_kf=ref_kf, batch_id=counter - i % 6, px=pt["px"][i].tolist(), f=pt["f"][i].tolist(), level=int(pt["level"][i]), type=int(pt["type"][i]),
                                 grad=pt["grad"][i].tolist(), **{k: f32(pt[k][i]) for k in ("a", "b", "mu", "z_range", "sigma2")}))
        for i in (range(ns) if segments else ()):
            sd["seg"].append(dict(ref_kf=ref_kf, batch_id=counter - (5 if i == 3 else i % 3), px=seg["px"][i].tolist(), f=seg["f"][i].tolist(), sf=seg["sf"][i].tolist(),
                                  ef=seg["ef"][i].tolist(), spx=seq["seg_spx0"][i].tolist(), epx=seq["seg_epx0"][i].tolist(), level=int(seg["level"][i]),
                                  **{k: f32(seg[k][i]) for k in ("a", "b", "mu_s", "mu_e", "z_range_s", "z_range_e", "sigma2_s", "sigma2_e")}))
        return sd
    T = [list(map(float, t)) for t in seq["poses_true"]]
    tables = [dict(kf_T=[T[0], T[1]], kf_slot=[0, 1]), dict(kf_T=[T[1], T[0]], kf_slot=[1, 0]), dict(kf_T=[T[0]], kf_slot=[0]), dict(kf_T=[T[0], T[1]], kf_slot=[0, 1])]
    sts = []
    for t in tables:
        st = Cc.empty_stream(t["kf_T"])
        st.update(kf_slot=t["kf_slot"], pt_nfail=[], pt_nsucc=[], seg_nfail=[], seg_nsucc=[])
        sts.append(st)
    seeds = [seeds_of(0, True, True), seeds_of(1, True, False), seeds_of(0, False, True), seeds_of(0, True, True)]
    return seq, sts, seeds, [True, True, True, False]


def _host_rows(P, ctx, seq, sd):
    """the host path's half of an update: the caller's age test, then plsvo_update_seeds on the seeds that are left -> body(kind, seed)"""
    live = {kind: [x for x in sd[kind] if not SL.aged(sd, x, Sl.MAX_N_KFS)] for kind in ("pt", "seg")}
    col = lambda kind, k: np.array([x[k] for x in live[kind]])
    pt = dict(ref_frame=np.zeros(len(live["pt"]), np.int32), cur_frame=np.full(len(live["pt"]), 2, np.int32), **{k: col("pt", k) for k in ("px", "f", "level", "type", "grad", "a", "b", "mu", "z_range", "sigma2")}) if live["pt"] else None
    seg = dict(ref_frame=np.zeros(len(live["seg"]), np.int32), cur_frame=np.full(len(live["seg"]), 2, np.int32),
               **{k: col("seg", k) for k in ("px", "f", "sf", "ef", "level", "a", "b", "mu_s", "mu_e", "z_range_s", "z_range_e", "sigma2_s", "sigma2_e")}) if live["seg"] else None
    rd = ctx.update_seeds(P.abi.SeedsJob(seq["cam"], seq["poses_true"], np.arange(3), pt, seg))
    at = dict(pt={id(x): j for j, x in enumerate(live["pt"])}, seg={id(x): j for j, x in enumerate(live["seg"])})

    def body(kind, seed):
        j = at[kind][id(seed)]
        names = SL.PT_ROWS if kind == "pt" else SL.SEG_ROWS
        return {key: (int(rd[f][j]) if key == "status" else rd[f][j].tolist() if key.startswith("xyz") else rd[f][j]) for f, key in names}
    return body, rd, live


@pytest.mark.gpu
def test_update_on_images_equals_update_seeds_plus_the_restatement_plus_add(P, ob):
    """the resident update equals plsvo_update_seeds (the body, on the seeds the caller's age test leaves) plus the restatement's list
    handling plus plsvo_candidates_add, in every shadow row, every seed row and every map table; the next frame's run / match / select /
    pose_optimize on the grown tables equal those on a fresh stage of the same tables"""
    seq, sts, seeds, active = _image_case(P, ob)
    cam = tuple(seq["cam"])
    ctx = P.capi.Context(0)
    try:
        ctx.config_pyramids(3, 320, 240, 4)
        for k, im in enumerate(seq["images"]):
            ctx.build_pyramid(k, im, 0)
        T2 = [float(v) for v in seq["poses_true"][2]]
        bodies = [_host_rows(P, ctx, seq, sd) if a else None for sd, a in zip(seeds, active)]

        def stage_tables(tabs):
            ctx.candidates_reserve(extra_pt_obs=100, extra_seg_obs=20)
            ctx.candidates_reserve_landmarks(extra_pt=100, extra_seg=20)
            ctx.candidates_stage([Cc.to_job(st) for st in tabs], cam, Sl.CELL, Sl.SEG_CELL, Sl.BOUNDARY)
            set_quality(ctx, tabs)
        stage_tables(sts)
        ctx.seeds_reserve()
        ctx.seeds_stage([SL.lists_of(sd) for sd in seeds], cam, max_n_kfs=Sl.MAX_N_KFS)
        staged = copy.deepcopy(seeds)
        ctx.seeds_update([dict(cur_slot=2, T_f_w=T2) if a else None for a in active])
        got = ctx.seeds_update_fetch()
        rows = ctx.seeds_fetch_rows()
        reps, news = [], []
        for k, (sd, st, a, b, r) in enumerate(zip(seeds, sts, active, bodies, rows)):
            if not a:
                reps.append(SL.report_of(sd, st)); news.append(None)
                assert len(r["pt_status"]) == 0 and len(r["seg_status"]) == 0
                continue
            body, rd, live = b
            n_old = (len(st["pt_pos"]), len(st["seg_spos"]))
            rep, _, want_rows = SL.update(sd, st, body, Sl.MAX_N_KFS)
            reps.append(rep)
            # every shadow row: the aged ones by the restatement, the others plsvo_update_seeds' bytes (px_cur and depth included)
            for kind, names in (("pt", SL.PT_ROWS), ("seg", SL.SEG_ROWS)):
                for f, key in names:
                    same_bytes(r[f], [w[key] for w in want_rows[kind]], ("rows", k, f))
                keep = [j for j, x in enumerate(staged[k][kind]) if not SL.aged(staged[k], x, Sl.MAX_N_KFS)]
                for f in (("pt_px_cur", "pt_depth") if kind == "pt" else ("seg_depth_s", "seg_depth_e")):
                    same_bytes(r[f][keep], rd[f], ("rows", k, f))
            news.append(dict(pt=[dict(pos=p, obs=o[0]) for p, o in zip(st["pt_pos"][n_old[0]:], st["pt_obs"][n_old[0]:])],
                             seg=[dict(spos=a_, epos=b_, obs=o[0]) for a_, b_, o in zip(st["seg_spos"][n_old[1]:], st["seg_epos"][n_old[1]:], st["seg_obs"][n_old[1]:])]))
        check_reports(got, reps, "update on images")
        assert sum(r["pt"][SL.CONVERGED] for r in reps) >= 6 and sum(r["seg"][SL.CONVERGED] for r in reps) >= 4 and sum(r["pt"][SL.AGED] + r["seg"][SL.AGED] for r in reps) > 20
        assert sum(r["pt"][SL.NAN] + r["pt"][SL.NO_MATCH] for r in reps) > 0 and sum(r["pt"][SL.NOT_VISIBLE] for r in reps) >= 2
        check_lists(ctx, seeds, "update on images")
        check_tables(ctx, sts, "update on images")
        resident = snapshot(ctx)

        def next_frame():
            ctx.candidates_run([P.abi.CandidateFrameJob(T2, tuple(range(len(st["kf_T"]))), cur_slot=2) for st in sts])
            ctx.candidates_match()
            cand = ctx.candidates_fetch()
            ctx.candidates_select(**Sl.PARAMS)
            sel = ctx.candidates_select_fetch()
            ctx.candidates_pose_optimize()
            return cand, sel, ctx.candidates_pose_fetch([(g["n_matches"], g["n_ls_matches"]) for g in sel])
        c1, s1, p1 = next_frame()
        assert sum(g["n_matches"] for g in s1) > 3                    # the new candidates are matched in the frame they converged in
        # the host path of the same tree: the tables as they were, plsvo_candidates_add of the converged seeds' records
        old = [dict(st, pt_pos=[], pt_type=[], pt_obs=[], seg_spos=[], seg_epos=[], seg_type=[], seg_obs=[], pt_cand=[], seg_cand=[], pt_nfail=[], pt_nsucc=[], seg_nfail=[], seg_nsucc=[])
               for st in sts]
        stage_tables(old)
        ctx.candidates_add([Nc.records(nw) if nw else None for nw in news])
        for a, b in zip(resident, snapshot(ctx)):
            for f in a:
                same_bytes(b[f], a[f], ("host path", f))
        # a fresh stage of the grown tables
        stage_tables(sts)
        c2, s2, p2 = next_frame()
        for k in range(len(sts)):
            for f in c1[k]:
                same_bytes(c2[k][f], c1[k][f], ("restaged", "candidates", k, f))
            for f in s1[k]:
                same_bytes(s2[k][f], s1[k][f], ("restaged", "select", k, f))
            same_bytes(p2[k].T, p1[k].T, ("restaged", "pose", k)); same_bytes(p2[k].cov, p1[k].cov, ("restaged", "cov", k))
            same_bytes(p2[k].pt_keep, p1[k].pt_keep, ("restaged", "pt_keep", k)); same_bytes(p2[k].seg_keep, p1[k].seg_keep, ("restaged", "seg_keep", k))
    finally:
        ctx.close()
