"""The keyframe stage on the resident map tables (plsvo_candidates_set_keypts / _fetch_keypts / _run_close / _close_fetch and the upkeep of
the key-point table behind the selection and the insertion; pl-svo_amd/csrc/keystage_device.hpp) against its restatement
tests/np_keystage.py.  Every comparison is byte for byte; on gathered inputs the close list is also compared with the synchronous
plsvo_close_keyframes, which runs the same device functions.  The frames of the upkeep tests are driven as in tests/test_gpu_insert.py:
constructed match results and keep masks."""
import copy

import numpy as np
import pytest

import candidates_cases as Cc
import insert_cases as Ic
import np_candidates as N
import np_keyframe as K
import np_keystage as NK
import select_cases as Sc
from test_gpu_insert import ctx, frame, insert, stage      # (ctx: a module fixture with pyramids of the small camera's size)
from test_gpu_select import CAND_FIELDS, same_bytes

CAM_T = Cc.CAM_T                                           # 320 x 240, fx a power of two: constructed pixels are exact
U, G = Sc.U, Sc.G


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def check_close(got, want, tag):
    assert (got["n_close"], got["n_overlap"]) == (want["n_close"], want["n_overlap"]), (tag, got, want)
    assert np.array_equal(got["close_idx"], want["close_idx"]), (tag, got["close_idx"], want["close_idx"])
    assert np.array_equal(bits(got["close_dist"]), bits(want["close_dist"])), tag


def stage_plain(ctx, sts):
    ctx.candidates_reserve()
    ctx.candidates_reserve_landmarks()
    ctx.candidates_stage([Cc.to_job(st) for st in sts], Cc.CAM, Cc.CELL, Cc.SEG_CELL, Cc.BOUNDARY)


def run_close_and_check(ctx, P, sts, tables, Ts, max_n_kfs, tag):
    """run_close against the restatement, against the synchronous call on gathered inputs, and its candidates against a plain run with
    the same list from the host"""
    frames = lambda ovs: [P.abi.CandidateFrameJob(T, ov, cur_slot=0) for T, ov in zip(Ts, ovs)]
    ctx.candidates_run_close(frames([()] * len(sts)), max_n_kfs)
    got = ctx.candidates_close_fetch()
    cand = ctx.candidates_fetch()
    want = [NK.close(st, tab, T, CAM_T, max_n_kfs) for st, tab, T in zip(sts, tables, Ts)]
    jobs = []
    for st, tab, T in zip(sts, tables, Ts):
        n_kf = len(st["kf_T"])
        kp, kv = np.zeros((n_kf, 5, 3)), np.zeros((n_kf, 5), np.uint8)
        for k in range(n_kf):
            for s in range(5):
                h = int(tab[k][s])
                if h >= 0 and st["kf_pt"][k][h] >= 0:
                    kp[k, s], kv[k, s] = st["pt_pos"][st["kf_pt"][k][h]], 1
        jobs.append(P.abi.CloseKeyframesJob(Cc.CAM, T, np.array(st["kf_T"]).reshape(-1, 7), kp, kv, max_n_kfs))
    sync = ctx.close_keyframes(jobs)
    for k, (g, w, s) in enumerate(zip(got, want, sync)):
        check_close(g, w, (tag, "restatement", k))
        check_close(g, s, (tag, "plsvo_close_keyframes", k))
    ctx.candidates_run(frames([w["close_idx"][:w["n_overlap"]] for w in want]))
    plain = ctx.candidates_fetch()
    for k, (a, b) in enumerate(zip(cand, plain)):
        assert (a["n_filed_pt"], a["n_filed_seg"]) == (b["n_filed_pt"], b["n_filed_seg"]), (tag, k)
        for f in CAND_FIELDS + ("pt_cand_failed", "seg_cand_failed"):
            same_bytes(a[f], b[f], (tag, "candidates", k, f))
    return want


# ---- close keyframes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_kfs", [(64,), (1, 5, 64, 65), (65, 5, 1, 64, 5)], ids=["1 stream", "4 streams", "5 streams"])
def test_close_keyframes_on_the_resident_tables(ctx, P, n_kfs):
    """a full and a partial workgroup, streams of unequal size, tables of 1, 5, 64 and 65 keyframes (the rounds of 64 of both passes);
    every other stream's key points computed on the device, the others given (rows of five NULLs among them); max_n_kfs below, at and
    above n_close"""
    rng = np.random.default_rng(9100 + len(n_kfs))
    sts = [Cc.rand_stream(rng, [(int(rng.integers(0, 9)), 2) for _ in range(n)], 40, 6, 3, 2, max_obs=4) for n in n_kfs]
    given = []
    for s, st in enumerate(sts):
        if s % 2 == 0 and len(n_kfs) > 1:
            given.append(None)
            continue
        tab = np.full((len(st["kf_T"]), 5), -1, np.int32)
        for k, l in enumerate(st["kf_pt"]):
            if l and rng.random() < 0.8:
                tab[k] = [int(rng.integers(-1, len(l))) for _ in range(5)]
        given.append(tab)
    stage_plain(ctx, sts)
    ctx.candidates_set_keypts(given)
    tables = ctx.candidates_fetch_keypts()
    for k, (st, g, t) in enumerate(zip(sts, given, tables)):
        same_bytes(t[:len(st["kf_T"])], NK.fresh(st, CAM_T) if g is None else g, ("table", k))
    Ts = [Cc.rand_pose(rng, 0.5, 0.8) for _ in sts]
    first = run_close_and_check(ctx, P, sts, tables, Ts, 10, "max 10")
    big = max(range(len(sts)), key=lambda k: first[k]["n_close"])
    n_close = first[big]["n_close"]
    assert 2 <= n_close and (len(n_kfs) == 1 or any(0 < w["n_close"] < len(st["kf_T"]) for w, st in zip(first, sts)))   # (one stream: every keyframe may be close)
    for m in sorted({max(n_close - 1, 0), n_close, n_close + 1, 0}):
        want = run_close_and_check(ctx, P, sts, tables, Ts, m, "max %d" % m)
        assert want[big]["n_overlap"] == min(m, n_close)


def directed_close_stream():
    """the new frame at the origin without rotation; keyframe k has one feature, its only key point, at a pixel chosen exactly"""
    centres = [(0.3, 0, 0), (0.5, 0, 0), (0.7, 0, 0), (0.9, 0, 0), (0.2, 0.1, 0), (0.05, 0, 0), (0.1, 0, 0), (-0.1, 0, 0), (0, 0.1, 0)]
    st = Cc.empty_stream([Cc.kf_at(c) for c in centres])
    at = [Cc.pos_at(0.0, 100.0, 4.0), Cc.pos_at(320.0, 100.0, 4.0), Cc.pos_at(100.0, 240.0, 4.0), Cc.pos_at(100.0, 0.0, 4.0), [0.1, 0.05, -2.0], None,
          Cc.pos_at(50.0, 50.0, 4.0), Cc.pos_at(60.0, 60.0, 4.0), Cc.pos_at(70.0, 70.0, 4.0)]
    for k, p in enumerate(at):
        if p is not None:
            st["kf_pt"][k].append(Cc.add_pt(st, p, N.TYPE_GOOD, [Cc.observe(k, st["kf_T"][k], p)]))
    names = dict(x0=0, x_width=1, y_height=2, y0=3, behind=4, all_null=5, equal_a=6, equal_b=7, equal_c=8)
    return st, names


@pytest.mark.gpu
def test_close_keyframes_edges_and_live_positions(ctx, P):
    """projections at exactly 0 (visible) and exactly width / height (not), a key point behind the camera, a keyframe of five NULLs, three
    keyframes at the same distance (table order); then two key landmarks are moved (plsvo_candidates_set_positions) so that their
    visibility flips: the position is read where it lies NOW"""
    st, nm = directed_close_stream()
    other = Cc.rand_stream(np.random.default_rng(9150), [(5, 1)] * 3, 20, 4, max_obs=3)
    sts = [other, st]
    stage_plain(ctx, sts)
    ctx.candidates_set_keypts()
    tables = ctx.candidates_fetch_keypts()
    assert list(tables[1][nm["all_null"]]) == [-1] * 5 and all(t[0] == 0 for k, t in enumerate(tables[1][:9]) if k != nm["all_null"])
    Ts = [Cc.rand_pose(np.random.default_rng(9151)), list(Cc.IDENT)]
    want = run_close_and_check(ctx, P, sts, tables, Ts, 10, "edges")[1]
    assert list(want["close_idx"]) == [nm["equal_a"], nm["equal_b"], nm["equal_c"], nm["x0"], nm["y0"]], want
    assert want["close_dist"][0] == want["close_dist"][1] == want["close_dist"][2]
    # the landmark at x = width moves half a pixel inside, the one at x = 0 behind the camera
    moved = {st["kf_pt"][nm["x_width"]][0]: Cc.pos_at(319.5, 100.0, 4.0), st["kf_pt"][nm["x0"]][0]: [0.0, 0.0, -1.0]}
    ctx.candidates_set_positions([None, dict(pt_idx=list(moved), pt_pos=list(moved.values()))])
    st2 = copy.deepcopy(st)
    for lm, p in moved.items():
        st2["pt_pos"][lm] = [float(v) for v in p]
    want2 = run_close_and_check(ctx, P, [other, st2], tables, Ts, 10, "moved")[1]
    assert nm["x_width"] in want2["close_idx"] and nm["x0"] not in want2["close_idx"]
    snapshot = NK.close(st, tables[1], Ts[1], CAM_T, 10)                 # what positions snapshot at set_keypts time would give
    assert list(snapshot["close_idx"]) != list(want2["close_idx"])


# ---- upkeep of the key-point table --------------------------------------------------------------------------------------------------------
def fetch_tables(ctx, sts):
    return [t[:len(st["kf_T"])].copy() for t, st in zip(ctx.candidates_fetch_keypts(), sts)]


def selection_upkeep(before, after, tables, tag):
    """the table behind a selection, event by event (the landmarks in ascending order) and all at once: the same.  Returns the tables and
    the number of keyframes rebuilt"""
    out, n = [], 0
    for k, (b, a, t) in enumerate(zip(before, after, tables)):
        seq, rebuilt = NK.sequential_upkeep(b, t, Ic.CAM_T, NK.deleted_landmarks(b, a))
        bat = NK.batched_upkeep(a, t, Ic.CAM_T)
        same_bytes(seq, bat, (tag, "sequential vs batched", k))
        out.append(bat); n += len(rebuilt)
    return out, n


@pytest.mark.gpu
def test_key_points_follow_the_selection_and_the_insertion(ctx, P):
    """thirteen unequal streams (tests/insert_cases.py): the table from five NULLs, after a frame's selection (safeDeletePoint of the
    failures), after an insertion that removes the first, a middle, the last or no keyframe (rows close up, holders lost to the removal,
    the new keyframe's row from five NULLs), after a second frame and a second insertion; the selection's and the insertion's own outputs
    and tables are compared with their restatements on the way (frame, insert), so the upkeep disturbs neither"""
    streams = Ic.batch()
    sts = [copy.deepcopy(s["st"]) for s in streams]
    stage(ctx, sts)
    ctx.candidates_set_keypts()
    want = [NK.fresh(st, Ic.CAM_T) for st in sts]
    for k, (g, w) in enumerate(zip(fetch_tables(ctx, sts), want)):
        same_bytes(g, w, ("fresh", k))
    rebuilt, lost = 0, dict(first=0, middle=0, last=0)      # keyframes rebuilt behind a selection; behind the removal of the first / a middle / the last row
    T2 = ov2 = None
    for rnd in (1, 2):
        before = copy.deepcopy(sts)
        _, _, sel = frame(ctx, P, streams, sts, T2, ov2, tag="frame %d" % rnd)
        want, n = selection_upkeep(before, sts, want, "selection %d" % rnd)
        rebuilt += n
        for k, (g, w) in enumerate(zip(fetch_tables(ctx, sts), want)):
            same_bytes(g, w, ("selection", rnd, k))
        active = [s["is_kf"] for s in streams] if rnd == 1 else [(not s["is_kf"]) or k % 2 == 0 for k, s in enumerate(streams)]
        remove = [s["remove_kf"] for s in streams] if rnd == 1 else [0 if len(st["kf_T"]) >= 2 else -1 for st in sts]
        mid = copy.deepcopy(sts)
        insert(ctx, streams, sts, sel, active, remove, tag="insertion %d" % rnd)
        new = []
        for k, (s, b, st, w, f, a, r) in enumerate(zip(streams, mid, sts, want, sel, active, remove)):
            if not a:
                new.append(w)
                continue
            # event by event on np_insert's order (the tables before the insertion), and all at once on the tables after it: the same
            seq, events = NK.sequential_insert_upkeep(b, f, Ic.keep_masks(s, f)[0], w, Ic.CAM_T, r)
            same_bytes(NK.insert_upkeep(st, w, Ic.CAM_T, r), seq, ("insertion: sequential vs batched", rnd, k))
            new.append(seq)
            if r >= 0 and events:
                where = "first" if r == 0 else "last" if r == len(b["kf_T"]) - 1 else "middle"
                lost[where] += len(events)
        want = new
        for k, (g, w) in enumerate(zip(fetch_tables(ctx, sts), want)):
            same_bytes(g, w, ("insertion", rnd, k))
        two = [Ic.second_frame_of(s, st, k) for k, (s, st) in enumerate(zip(streams, sts))]
        T2, ov2 = [t for t, _ in two], [o for _, o in two]
    print("keyframes rebuilt behind selections: %d, behind removals: %s" % (rebuilt, lost))
    assert rebuilt > 0 and all(v > 0 for v in lost.values()), (rebuilt, lost)
    # the overlap list from the table as it now stands feeds a third frame
    ctx.candidates_run_close([P.abi.CandidateFrameJob(T, (), cur_slot=0) for T in T2], 10)
    for k, (g, st, w, T) in enumerate(zip(ctx.candidates_close_fetch(), sts, want, T2)):
        check_close(g, NK.close(st, w, T, Ic.CAM_T, 10), ("third frame", k))


def directed_upkeep_stream():
    """four keyframes, each a scenario; a landmark is seen by one keyframe, and its px THERE is set by hand (cu = 163, cv = 123)"""
    b = Ic.Builder(4)
    cells = iter(range(12, 88))

    def pt(kf, px, typ=G, found=1, nfail=0):
        lm = b.pt(*Ic.pc(next(cells)), typ, found, kfs=(kf,), nfail=nfail)
        b.st["pt_obs"][lm][0]["px"] = [float(px[0]), float(px[1])]
        return lm

    nm = {}
    # keyframe 0, the pinned tie: A holds slot 0, H slot 1; E stands before H with H's value exactly; G is strictly better and no holder
    nm["A"] = pt(0, (163, 123), U, 0, 15); nm["E"] = pt(0, (173, 133)); nm["H"] = pt(0, (183, 128)); nm["G"] = pt(0, (193, 143), U, 0, 15)
    # keyframe 1: X, no holder, is deleted by the first frame (no rebuild: the better B is NOT taken); Y, a holder, by the second (B is)
    pt(1, (173, 133)); nm["B"] = pt(1, (263, 223)); nm["X"] = pt(1, (100, 200), U, 0, 15); nm["Y"] = pt(1, (200, 50), U, 0, 14)
    # keyframe 2: both holders deleted in one launch, no landmark left
    pt(2, (150, 100), U, 0, 15); pt(2, (200, 200), U, 0, 15)
    # keyframe 3: the holder W goes; Q has cv <= x < cu and y < cv (no slot but the centre's: slot 3 compares x with cv), R has x < cv
    pt(3, (163, 123), U, 0, 15); pt(3, (140, 100)); pt(3, (100, 100))
    given = [[0, 2, -1, -1, -1], [0, 0, 3, -1, -1], [0, 1, -1, -1, -1], [0, -1, -1, -1, -1]]
    return b.done(), nm, given


@pytest.mark.gpu
def test_key_point_upkeep_directed(ctx, P):
    """a holder deleted; no holder deleted (no rebuild, a better feature is not taken) and the same feature taken by the next rebuild;
    two holders of a keyframe deleted in one launch, leaving five NULLs; the x < cv quirk of slots 3 and 4; the tie include/plsvo_hip.h
    pins: the device's batched form keeps the surviving holder where the reference's event order (A's cell before G's) takes the first
    feature of the same value; compaction afterwards moves no feature position"""
    s, nm, given = directed_upkeep_stream()
    streams = [Ic.batch()[6], s, Ic.batch()[10]]                        # (in the middle of other streams)
    sts = [copy.deepcopy(x["st"]) for x in streams]
    stage(ctx, sts)
    ctx.candidates_set_keypts([None, given, None])
    tables = fetch_tables(ctx, sts)
    same_bytes(tables[1], given, "given")
    before = copy.deepcopy(sts)
    frame(ctx, P, streams, sts, tag="frame 1")
    assert NK.deleted_landmarks(before[1], sts[1]) == sorted([nm["A"], nm["G"], nm["X"]] + before[1]["kf_pt"][2] + before[1]["kf_pt"][3][:1])
    got = fetch_tables(ctx, sts)
    for k in range(3):
        same_bytes(got[k], NK.batched_upkeep(sts[k], tables[k], Ic.CAM_T), ("frame 1", k))
    assert got[1].tolist() == [[1, 2, -1, -1, -1], [0, 0, 3, -1, -1], [-1] * 5, [1, -1, -1, 2, -1]], got[1]
    order = [lm for lm in NK.deleted_landmarks(before[1], sts[1])]
    a_first, _ = NK.sequential_upkeep(before[1], tables[1], Ic.CAM_T, order)                                    # A (cell 12) before G (cell 15): the reference's order
    g_first, _ = NK.sequential_upkeep(before[1], tables[1], Ic.CAM_T, [nm["G"]] + [lm for lm in order if lm != nm["G"]])
    assert a_first[0].tolist() == [1, 1, -1, -1, -1] and np.array_equal(a_first[1:], got[1][1:]) and np.array_equal(g_first, got[1])
    # the second frame deletes Y, a holder of keyframe 1: the rebuild takes B
    before = copy.deepcopy(sts)
    frame(ctx, P, streams, sts, tag="frame 2")
    assert NK.deleted_landmarks(before[1], sts[1]) == [nm["Y"]]
    got2 = fetch_tables(ctx, sts)
    for k in range(3):
        seq, _ = NK.sequential_upkeep(before[k], got[k], Ic.CAM_T, NK.deleted_landmarks(before[k], sts[k]))
        same_bytes(got2[k], seq, ("frame 2", k))
    assert got2[1][1].tolist() == [0, 1, -1, -1, -1]
    # compaction: landmark rows move, feature positions do not
    T = [list(Cc.IDENT)] * 3
    ctx.candidates_run_close([P.abi.CandidateFrameJob(t, (), cur_slot=0) for t in T], 10)
    close_before = ctx.candidates_close_fetch()
    ctx.candidates_compact(["always"] * 3)
    assert sum(r["n_pt_before"] - r["n_pt_after"] for r in ctx.candidates_compact_fetch(remap=False)) > 5
    for k, (a, b) in enumerate(zip(fetch_tables(ctx, sts), got2)):
        same_bytes(a, b, ("compacted", k))
    ctx.candidates_run_close([P.abi.CandidateFrameJob(t, (), cur_slot=0) for t in T], 10)
    for k, (a, b) in enumerate(zip(ctx.candidates_close_fetch(), close_before)):
        check_close(a, b, ("compacted", k))
        check_close(a, NK.close(sts[k], got2[k], T[k], Ic.CAM_T, 10), ("compacted, restatement", k))


# ---- states -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_keystage_states_and_arguments(ctx, P):
    E = P.capi.PlsvoError
    rng = np.random.default_rng(9300)
    sts = [Cc.rand_stream(rng, [(4, 1)] * 3, 12, 3, max_obs=3) for _ in range(2)]
    frames = [P.abi.CandidateFrameJob(Cc.IDENT, (), cur_slot=0) for _ in sts]

    def code(f, *a):
        with pytest.raises(E) as e:
            f(*a)
        return e.value.code

    stage_plain(ctx, sts)
    assert code(ctx.candidates_run_close, frames, 10) == P.abi.E_STATE          # no live table
    assert code(ctx.candidates_fetch_keypts) == P.abi.E_STATE
    ctx.candidates_run([P.abi.CandidateFrameJob(Cc.IDENT, (0,), cur_slot=0) for _ in sts])
    assert code(ctx.candidates_close_fetch) == P.abi.E_STATE                     # the last run was a plain one
    assert code(ctx.candidates_set_keypts, [np.full((3, 5), -2, np.int32), None]) == P.abi.E_INVALID
    ctx.candidates_set_keypts()
    assert code(ctx.candidates_run_close, frames[:1], 10) == P.abi.E_INVALID     # another n than staged
    assert code(ctx.candidates_run_close, frames, -1) == P.abi.E_INVALID
    assert code(ctx.candidates_run_close, [P.abi.CandidateFrameJob(Cc.IDENT, (0,), cur_slot=0) for _ in sts], 10) == P.abi.E_INVALID   # a list from the host
    assert ctx.L.plsvo_candidates_run_close(ctx.h, 2, None, 10) == P.abi.E_INVALID
    assert ctx.L.plsvo_candidates_fetch_keypts(ctx.h, 2, None) == P.abi.E_INVALID
    assert ctx.L.plsvo_candidates_close_fetch(ctx.h, 2, None) in (P.abi.E_STATE, P.abi.E_INVALID)
    ctx.candidates_run_close(frames, 10)
    ctx.candidates_close_fetch()
    assert ctx.L.plsvo_candidates_close_fetch(ctx.h, 2, None) == P.abi.E_INVALID
    stage_plain(ctx, sts)                                                        # a stage drops the table
    assert code(ctx.candidates_run_close, frames, 10) == P.abi.E_STATE


@pytest.mark.gpu
def test_without_a_live_table_nothing_changes(ctx, P):
    """a context whose key-point table was live once and was dropped by a stage, against a context that never heard of it: the outputs
    and the fetched map of a frame's selection, an insertion and a compaction are the same bytes"""
    streams = Ic.batch()[:5]
    res = []
    for used in (True, False):
        c = P.capi.Context(0)
        try:
            c.config_pyramids(4, Sc.CAM_T[4], Sc.CAM_T[5], 3)
            for s in range(4):
                c.build_pyramid(s, np.zeros((Sc.CAM_T[5], Sc.CAM_T[4]), np.uint8))
            sts = [copy.deepcopy(s["st"]) for s in streams]
            if used:
                stage(c, sts)
                c.candidates_set_keypts()
                c.candidates_run_close([P.abi.CandidateFrameJob(s["T"], (), cur_slot=0) for s in streams], 10)
            stage(c, sts)
            _, got, sel = frame(c, P, streams, sts, tag="frame")
            out = [got, c.candidates_fetch_map(), c.candidates_fetch_quality()]
            insert(c, streams, sts, sel, [s["is_kf"] for s in streams], [s["remove_kf"] for s in streams], tag="insertion")
            out += [c.candidates_fetch_map(), c.candidates_insert_fetch()]
            c.candidates_compact(["always"] * len(streams))
            out += [c.candidates_fetch_map(), c.candidates_fetch_quality(), c.candidates_compact_fetch()]
            res.append(out)
        finally:
            c.close()
    for a, b in zip(*res):
        for k, (x, y) in enumerate(zip(a, b)):
            assert x.keys() == y.keys()
            for f in x:
                assert np.asarray(x[f]).tobytes() == np.asarray(y[f]).tobytes(), (k, f)


# ---- the keyframe decision on the resident selection ---------------------------------------------------------------------------------------
DEC_CELL = 15                                              # 21 x 16 whole cells inside the border: room for 130 winners
DEC_SIZES = (0, 1, 63, 64, 65, 130, 40)


def decision_stream(n, seed):
    """n point landmarks, one per cell of 15 pixels (each wins its cell), and a few segments; four keyframes of which 1 and 3 have the
    SAME pose, far away (the furthest-keyframe tie); depths repeat (seven values); points on both sides of cu, cv and between cv and cu"""
    rng = np.random.default_rng(seed)
    b = Ic.Builder(4)
    far = Cc.kf_at((0.5, 0.0, 0.0))
    for k in (1, 3):
        b.kf_T[k] = list(far); b.st["kf_T"][k] = list(far)
    cells = [(cx, cy) for cy in range(1, 15) for cx in range(1, 20)]
    for i, k in enumerate(rng.permutation(len(cells))[:n]):
        cx, cy = cells[k]
        b.pt(cx * DEC_CELL + 7.5, cy * DEC_CELL + 7.5, (U, G)[i % 2], 1, kfs=(0, 2)[: 1 + i % 2], z=2.0 + 0.5 * (i % 7))
    for i in range(min(n, 6)):
        p = Ic.sc(16 + 6 * i)
        b.seg((p[0] - 4, p[1]), (p[0] + 4, p[1] + 2), G, (1, 1), kfs=(0,))
    return b.done()


def decision_frame(c, P, streams, sts, reproj_thresh=2.0):
    """candidates -> constructed match -> selection -> the resident pose optimiser; returns the device's selection, the keep masks and the
    optimised poses"""
    c.candidates_run([P.abi.CandidateFrameJob(s["T"], s["overlap"], cur_slot=0) for s in streams])
    cand = c.candidates_fetch()
    c.candidates_set_match([Sc.match_of(s, r) for s, r in zip(streams, cand)])
    c.candidates_select(max_fts=200, max_fts_segs=100, reproj_thresh=reproj_thresh)
    sel = c.candidates_select_fetch()
    c.candidates_pose_optimize()
    po = c.candidates_pose_fetch([(g["n_matches"], g["n_ls_matches"]) for g in sel])
    return sel, [(p.pt_keep, p.seg_keep) for p in po], [[float(v) for v in p.T] for p in po]


def check_decision(c, P, sts, sel, masks, poses, decides, overlaps, tag, prev=None):
    got = c.candidates_decide_fetch()
    jobs, idx = [], []
    for k, (st, s, m, T, d, ov) in enumerate(zip(sts, sel, masks, poses, decides, overlaps)):
        if d is None:
            want = prev[k] if prev else dict(has_depth=0, n_depth=0, depth_mean=0.0, depth_min=0.0, need_new_kf=0, blocking=0, key_pts=np.zeros(5, np.int32), furthest_kf=0)
            for f in want:
                assert np.asarray(got[k][f]).tobytes() == np.asarray(want[f]).tobytes(), (tag, "left alone", k, f)
            continue
        want = NK.decide(st, s, m[0], m[1], T, d["T_last_w"], ov, Ic.CAM_T, d.get("kfselect_mindist_t", 0.06), d.get("kfselect_mindist_r", 3.0))
        for f in ("has_depth", "n_depth", "need_new_kf", "blocking", "furthest_kf"):
            assert got[k][f] == want[f], (tag, k, f, got[k][f], want[f])
        for f in ("depth_mean", "depth_min"):
            assert bits(got[k][f]) == bits(want[f]), (tag, k, f, got[k][f], want[f])
        assert np.array_equal(got[k]["key_pts"], want["key_pts"]), (tag, k, got[k]["key_pts"], want["key_pts"])
        n_seg = len(s["seg_lm"])
        jobs.append(P.abi.KeyframeDecideJob(Ic.CAM, T, d["T_last_w"], s["pt_px"], np.array([st["pt_pos"][lm] for lm in s["pt_lm"]]).reshape(-1, 3), m[0],
                                            np.array([st["seg_spos"][lm] for lm in s["seg_lm"]]).reshape(-1, 3), np.array([st["seg_epos"][lm] for lm in s["seg_lm"]]).reshape(-1, 3),
                                            m[1][:n_seg], np.array(st["kf_T"]).reshape(-1, 7), list(ov), [-1] * 5, d.get("kfselect_mindist_t", 0.06), d.get("kfselect_mindist_r", 3.0)))
        idx.append(k)
    for k, r in zip(idx, c.keyframe_decide(jobs)):                     # the synchronous call on gathered inputs: the same device code, deltas included
        for f in r:
            assert np.asarray(r[f]).tobytes() == np.asarray(got[k][f]).tobytes(), (tag, "plsvo_keyframe_decide", k, f)
    return got


@pytest.mark.gpu
def test_keyframe_decision_on_the_resident_selection(ctx, P):
    """seven streams of 0, 1, 63, 64, 65, 130 and 40 selected points with segments (two workgroups, the second partial): scene depth with
    repeated depths, key points (cv <= x < cu among the pixels), a blocking keyframe at the first and at the last overlap position and
    none, the furthest of two keyframes with one pose; a stream that sits a call out keeps its record; positions moved by the resident
    structure optimiser behind the selection are the ones the depth is taken from; every feature rejected gives no depth"""
    streams = [decision_stream(n, 9400 + n) for n in DEC_SIZES]
    sts = [copy.deepcopy(s["st"]) for s in streams]
    ctx.candidates_reserve(**Ic.RESERVE); ctx.candidates_reserve_landmarks()
    ctx.candidates_stage([Cc.to_job(st) for st in sts], Ic.CAM, DEC_CELL, Ic.SEG_CELL, Ic.BOUNDARY)
    ctx.candidates_set_quality([dict(pt_n_failed=st["pt_nfail"], pt_n_succeeded=st["pt_nsucc"], seg_n_failed=st["seg_nfail"], seg_n_succeeded=st["seg_nsucc"]) for st in sts])
    E = P.capi.PlsvoError
    dec = lambda T, **kw: dict(T_last_w=list(T), **kw)
    with pytest.raises(E) as e:
        ctx.candidates_decide_fetch()
    assert e.value.code == P.abi.E_STATE
    ctx.candidates_run([P.abi.CandidateFrameJob(s["T"], s["overlap"], cur_slot=0) for s in streams])
    with pytest.raises(E) as e:                                        # before the pose optimisation
        ctx.candidates_keyframe_decide([dec(Cc.IDENT)] * len(streams))
    assert e.value.code == P.abi.E_STATE
    sel, masks, poses = decision_frame(ctx, P, streams, sts)
    assert [g["n_matches"] for g in sel] == list(DEC_SIZES) and all(g["n_ls_matches"] == min(n, 6) for g, n in zip(sel, DEC_SIZES))
    assert any(123 <= p[0] < 163 and p[1] < 123 for p in sel[5]["pt_px"])
    ovs = [s["overlap"] for s in streams]
    assert ctx.L.plsvo_candidates_keyframe_decide(ctx.h, len(streams) - 1, (P.abi.CandKfDecide * 8)()) == P.abi.E_INVALID
    assert ctx.L.plsvo_candidates_keyframe_decide(ctx.h, len(streams), None) == P.abi.E_INVALID
    # blocking at the first overlap position, at the last, nowhere; stream 6 sits the first call out
    far_T = Cc.kf_at((3.0, 3.0, 3.0))
    d1 = [dec(sts[0]["kf_T"][0], kfselect_mindist_t=0.01), dec(sts[1]["kf_T"][3], kfselect_mindist_t=0.01), dec(far_T), dec(sts[3]["kf_T"][0]), dec(far_T),
          dec(sts[5]["kf_T"][2], kfselect_mindist_t=0.01), None]
    ctx.candidates_keyframe_decide(d1)
    got1 = check_decision(ctx, P, sts, sel, masks, poses, d1, ovs, "first")
    assert [g["blocking"] for g in got1[:6]] == [0, 1, -1, 0, -1, 2] and got1[0]["has_depth"] == 0 and got1[0]["depth_min"] == np.finfo(np.float64).max
    assert all(g["furthest_kf"] == 1 for g in got1[:6])                  # keyframes 1 and 3 tie: the lower index
    d2 = [None] * 6 + [dec(far_T)]
    ctx.candidates_keyframe_decide(d2)
    got2 = check_decision(ctx, P, sts, sel, masks, poses, d2, ovs, "second", prev=got1)
    assert got2[6]["n_depth"] == int(masks[6][0].sum()) + 2 * int(masks[6][1].sum()) > 0
    # the resident structure optimiser moves landmarks of the selection: the decision reads the tables
    ctx.candidates_optimize_structure([dict(frame_id=1)] * len(streams))
    moved = ctx.candidates_fetch_map()
    sts2 = copy.deepcopy(sts)
    n_moved = 0
    for st, mv in zip(sts2, moved):
        n_moved += int(np.any(np.asarray(st["pt_pos"]).reshape(-1, 3) != mv["pt_pos"].reshape(-1, 3), axis=1).sum())
        st["pt_pos"] = [[float(v) for v in p] for p in mv["pt_pos"].reshape(-1, 3)]
        st["seg_spos"] = [[float(v) for v in p] for p in mv["seg_spos"].reshape(-1, 3)]
        st["seg_epos"] = [[float(v) for v in p] for p in mv["seg_epos"].reshape(-1, 3)]
    assert n_moved > 20
    # (the optimiser's steps are small and may leave a stream's median and minimum where they were: every selected point of stream 4 also moves by hand)
    lms = [int(v) for v in sel[4]["pt_lm"]]
    for lm in lms:
        sts2[4]["pt_pos"][lm][2] += 0.25
    ctx.candidates_set_positions([dict(pt_idx=lms, pt_pos=[sts2[4]["pt_pos"][lm] for lm in lms]) if k == 4 else None for k in range(len(streams))])
    d3 = [dec(far_T)] * len(streams)
    ctx.candidates_keyframe_decide(d3)
    got3 = check_decision(ctx, P, sts2, sel, masks, poses, d3, ovs, "moved")
    stale = [NK.decide(st, s, m[0], m[1], T, far_T, ov, Ic.CAM_T) for st, s, m, T, ov in zip(sts, sel, masks, poses, ovs)]
    assert got3[4]["depth_mean"] != stale[4]["depth_mean"] and got3[4]["depth_min"] != stale[4]["depth_min"]
    # the insertion closes the run
    ctx.candidates_insert_keyframe([dict(remove_kf=-1, kf_slot=1) for _ in streams])
    with pytest.raises(E) as e:
        ctx.candidates_keyframe_decide(d3)
    assert e.value.code == P.abi.E_STATE
    # a second frame whose features the pose optimiser rejects all (a threshold no residual passes)
    sts3 = [copy.deepcopy(s["st"]) for s in streams]
    ctx.candidates_stage([Cc.to_job(st) for st in sts3], Ic.CAM, DEC_CELL, Ic.SEG_CELL, Ic.BOUNDARY)
    sel4, masks4, poses4 = decision_frame(ctx, P, streams, sts3, reproj_thresh=1e-12)
    assert sum(int(m[0].sum()) + int(m[1].sum()) for m in masks4) == 0 and sel4[5]["n_matches"] == 130
    ctx.candidates_keyframe_decide(d3)
    got4 = check_decision(ctx, P, sts3, sel4, masks4, poses4, d3, ovs, "all rejected")
    assert all((g["has_depth"], g["depth_mean"], g["depth_min"]) == (0, 0.0, np.finfo(np.float64).max) and list(g["key_pts"]) == [-1] * 5 for g in got4)


@pytest.mark.gpu
def test_the_new_keyframe_row_is_the_decisions_key_points(ctx, P):
    """an insertion behind a resident decision: the new keyframe's row holds the decision's key points (selection order = its feature
    list), a key point whose feature the insertion leaves without a landmark is dropped and the row rebuilt; without a decision the row
    is built from five NULLs (test_key_points_follow_the_selection_and_the_insertion)"""
    streams = Ic.batch()
    sts = [copy.deepcopy(s["st"]) for s in streams]
    stage(ctx, sts)
    ctx.candidates_set_keypts()
    _, got, sel = frame(ctx, P, streams, sts, tag="frame", outliers=True)
    tables = fetch_tables(ctx, sts)
    ctx.candidates_pose_optimize()
    po = ctx.candidates_pose_fetch([(g["n_matches"], g["n_ls_matches"]) for g in got])
    decides = [dict(T_last_w=list(Cc.IDENT)) if k % 3 else None for k in range(len(streams))]     # every third stream inserts without a decision
    ctx.candidates_keyframe_decide(decides)
    dec = ctx.candidates_decide_fetch(deltas=False)
    ctx.candidates_insert_keyframe([dict(remove_kf=s["remove_kf"], kf_slot=s["kf_slot"]) if s["is_kf"] else None for s in streams])
    mid = copy.deepcopy(sts)
    for s, st, w, p in zip(streams, sts, sel, po):
        if s["is_kf"]:
            Ic.I.insert(st, w, p.pt_keep, p.seg_keep, [float(v) for v in p.T], s["kf_slot"], s["remove_kf"], Ic.CAM_T)
    after = fetch_tables(ctx, sts)
    n_decided = n_dropped = 0
    for k, (s, st, w, p, d, t) in enumerate(zip(streams, sts, sel, po, dec, tables)):
        if not s["is_kf"]:
            same_bytes(after[k], t, ("stands by", k))
            continue
        want, _ = NK.sequential_insert_upkeep(mid[k], w, p.pt_keep, t, Ic.CAM_T, s["remove_kf"], decided=None if decides[k] is None else d["key_pts"])
        if decides[k] is not None:
            n_decided += 1
            n_dropped += int(any(h >= 0 and st["kf_pt"][-1][h] < 0 for h in d["key_pts"]))
        same_bytes(after[k], want, ("inserted", k))
    assert n_decided >= 5
    print("new rows from a decision: %d, of them rebuilt over a dropped key point: %d" % (n_decided, n_dropped))


@pytest.mark.gpu
def test_a_feature_that_joined_is_taken_by_the_next_rebuild_only(ctx, P):
    """a candidate J whose original feature lies in keyframe 0 is matched by the new frame: the insertion's addCandidatePointToFrame
    appends it to keyframe 0, where it is strictly better than slot 1's holder -- and is NOT taken, no holder of keyframe 0 being lost
    (checkKeyPoints is not called for it).  The next frame's selection deletes Y, a holder of keyframe 0: the rebuild takes J, whose px
    is found in its observation list behind the new keyframe's observation that the insertion pushed in front"""
    b = Ic.Builder(3)
    cells = iter(range(12, 88))

    def pt(px, typ=G, found=1, nfail=0, cand=False):
        lm = b.pt(*Ic.pc(next(cells)), typ, found, kfs=(0,), nfail=nfail, cand=cand)
        b.st["pt_obs"][lm][0]["px"] = [float(px[0]), float(px[1])]
        return lm

    pt((173, 133)); Y = pt((200, 50), U, 0, 14); J = pt((263, 223), Sc.C_, 1, cand=True)
    s = b.done(remove_kf=-1)
    streams = [Ic.batch()[6], s]
    sts = [copy.deepcopy(x["st"]) for x in streams]
    stage(ctx, sts)
    given = [[0, 0, 1, -1, -1], [-1] * 5, [-1] * 5]
    ctx.candidates_set_keypts([None, given])
    t0 = fetch_tables(ctx, sts)
    _, _, sel = frame(ctx, P, streams, sts, tag="frame 1")
    mid = copy.deepcopy(sts)
    insert(ctx, streams, sts, sel, [True, True], [-1, -1], tag="insertion")
    assert sts[1]["kf_pt"][0] == [0, Y, J] and sts[1]["pt_obs"][J][0]["kf"] == 3 and sts[1]["pt_obs"][J][1]["kf"] == 0       # joined; the new observation in front
    t1 = fetch_tables(ctx, sts)
    for k in range(2):
        seq, _ = NK.sequential_insert_upkeep(mid[k], sel[k], Ic.keep_masks(streams[k], sel[k])[0], t0[k], Ic.CAM_T, -1)
        same_bytes(t1[k], seq, ("insertion", k))
    assert t1[1][0].tolist() == [0, 0, 1, -1, -1]                      # J, better in slot 1, is left alone
    two = [Ic.second_frame_of(x, st, k) for k, (x, st) in enumerate(zip(streams, sts))]
    before = copy.deepcopy(sts)
    frame(ctx, P, streams, sts, [t for t, _ in two], [o for _, o in two], tag="frame 2")
    assert Y in NK.deleted_landmarks(before[1], sts[1])
    t2 = fetch_tables(ctx, sts)
    for k in range(2):
        seq, _ = NK.sequential_upkeep(before[k], t1[k], Ic.CAM_T, NK.deleted_landmarks(before[k], sts[k]))
        same_bytes(t2[k], seq, ("frame 2", k))
    assert t2[1][0].tolist() == [0, 2, -1, -1, -1]                     # Y gone, the rebuild takes J (position 2) for slot 1


def two_cell_segments_stream():
    """two points and twelve segments whose end points lie in neighbouring cells of the segments' grid and win both: each is a feature
    of the new frame TWICE, so the depths number 2 + 2 * 24 where the filed landmarks are 2 + 12"""
    b = Ic.Builder(3)
    b.pt(*Ic.pc(13), G, 1, kfs=(0,)); b.pt(*Ic.pc(15), G, 1, kfs=(1,), z=3.0)
    for row in range(1, 7):
        for col in (1, 4):
            b.seg(Ic.sc(row * Sc.SEG_COLS + col), Ic.sc(row * Sc.SEG_COLS + col + 1), G, (1, 1), kfs=(0,))
    return b.done()


@pytest.mark.gpu
def test_keyframe_decision_with_segments_that_are_features_twice(ctx, P):
    """a stream with few points and many segments that each won both of their cells, ahead of two ordinary streams: its depth keys
    (n_matches + 2 * n_ls_matches, more than its filed landmarks' matcher entries) stay in its own row"""
    streams = [two_cell_segments_stream(), decision_stream(40, 9440), two_cell_segments_stream()]
    sts = [copy.deepcopy(s["st"]) for s in streams]
    ctx.candidates_reserve(); ctx.candidates_reserve_landmarks()
    ctx.candidates_stage([Cc.to_job(st) for st in sts], Ic.CAM, DEC_CELL, Ic.SEG_CELL, Ic.BOUNDARY)
    ctx.candidates_set_quality([dict(pt_n_failed=st["pt_nfail"], pt_n_succeeded=st["pt_nsucc"], seg_n_failed=st["seg_nfail"], seg_n_succeeded=st["seg_nsucc"]) for st in sts])
    sel, masks, poses = decision_frame(ctx, P, streams, sts)
    assert [(g["n_matches"], g["n_ls_matches"]) for g in sel] == [(2, 24), (40, 6), (2, 24)]
    assert 2 + 2 * 24 > 2 + 2 * 12                                      # the keys needed against the stream's matcher entries
    decides = [dict(T_last_w=list(Cc.kf_at((3.0, 3.0, 3.0))))] * 3
    ctx.candidates_keyframe_decide(decides)
    got = check_decision(ctx, P, sts, sel, masks, poses, decides, [s["overlap"] for s in streams], "segments twice")
    assert got[0]["n_depth"] == int(masks[0][0].sum()) + 2 * int(masks[0][1].sum()) > 26
