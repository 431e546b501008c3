"""The restatement of FrameHandlerBase::optimizeStructure on the map tables (tests/np_structsel.py) on the CPU: its arithmetic is held
to the C oracle's structure optimiser on the gathered jobs (oracle/binding.py), bit for bit, and its pinned choice to hand-made keys."""
import copy

import numpy as np

import insert_cases as Ic
import np_structsel as NS
import structsel_cases as K


def test_the_pinned_choice_takes_the_smallest_keys_and_the_earlier_of_equal_ones():
    keys = {lm: k for lm, k in enumerate([5, -3, 5, 7, 5, -3, 2 ** 31 - 1, -2 ** 31, 5, 5])}
    deque = list(range(10))
    assert NS.choose(deque, keys, 0) == [] and NS.choose(deque, keys, 10) == deque and NS.choose(deque, keys, 99) == deque
    assert NS.choose(deque, keys, 3) == [1, 5, 7]                      # signed: the most negative key first
    assert NS.choose(deque, keys, 5) == [0, 1, 2, 5, 7]                # two of the five equal keys at the cut: the earlier ones
    assert NS.choose([3, 3, 0], keys, 1) == [2] and NS.choose([0, 4, 4, 3], keys, 2) == [0, 1]   # a landmark twice in the deque


def restated(s, caps, mask=None):
    st = NS.keys(copy.deepcopy(s["st"]))
    _, _, sel = Ic.frame(s, st)
    pk = np.ones(len(sel["pt_lm"]), np.uint8) if mask is None else mask(sel)[0]
    sk = np.ones(len(sel["seg_lm"]), np.uint8) if mask is None else mask(sel)[1]
    before = copy.deepcopy(st)
    return before, st, sel, NS.optimize_structure(st, sel, pk, sk, 77, **caps)


def test_restatement_equals_the_oracle_on_the_gathered_jobs(P, ob):
    """every chosen landmark's new position and iteration count are the oracle's on the job gathered from the tables before the call; a
    segment chosen twice equals two oracle runs in sequence; what was not chosen is untouched and keeps its key"""
    for s, caps in ((K.seventy(), dict(max_n_pts=20, n_iter_pts=5, max_n_segs=20, n_iter_segs=5)), (K.observations(), dict(max_n_pts=30, n_iter_pts=5, max_n_segs=10, n_iter_segs=3)),
                    (K.batch()[3], dict(max_n_pts=2, n_iter_pts=1, max_n_segs=9, n_iter_segs=1))):
        before, st, sel, w = restated(s, caps)
        pts, segs = [int(v) for v in w["pt_lm"]], [int(v) for v in w["seg_lm"]]
        first = [i for i, lm in enumerate(segs) if lm not in segs[:i]]
        uniq = [segs[i] for i in first]
        r = ob.structure_optimize(P.structopt_job_from_batch(NS.gathered_job(before, pts, uniq), caps["n_iter_pts"], caps["n_iter_segs"]))
        assert np.array_equal(r["pt_pos"], w["pt_pos"], equal_nan=True) and np.array_equal(r["pt_iters"], w["pt_iters"])
        assert np.array_equal(r["seg_spos"], w["seg_spos"][first], equal_nan=True) and np.array_equal(r["seg_epos"], w["seg_epos"][first], equal_nan=True)
        assert np.array_equal(r["seg_iters"], w["seg_iters"][first])
        twice = [lm for lm in uniq if segs.count(lm) == 2]
        if s is K.seventy():
            assert len(twice) == 2
        if twice:                                                      # the second run starts from the first's result
            mid = copy.deepcopy(before)
            for lm, a, b in zip(uniq, r["seg_spos"], r["seg_epos"]):
                mid["seg_spos"][lm], mid["seg_epos"][lm] = [float(v) for v in a], [float(v) for v in b]
            r2 = ob.structure_optimize(P.structopt_job_from_batch(NS.gathered_job(mid, [], twice), caps["n_iter_pts"], caps["n_iter_segs"]))
            second = [max(i for i, v in enumerate(segs) if v == lm) for lm in twice]
            assert np.array_equal(r2["seg_spos"], w["seg_spos"][second]) and np.array_equal(r2["seg_epos"], w["seg_epos"][second]) and np.array_equal(r2["seg_iters"], w["seg_iters"][second])
        for lm in range(len(st["pt_pos"])):
            assert st["pt_last_optim"][lm] == (77 if lm in pts else 0) and (lm in pts or st["pt_pos"][lm] == before["pt_pos"][lm])
            if lm in pts:
                assert st["pt_pos"][lm] == [float(v) for v in w["pt_pos"][pts.index(lm)]]
        for lm in range(len(st["seg_spos"])):
            assert st["seg_last_optim"][lm] == (77 if lm in segs else 0) and (lm in segs or st["seg_epos"][lm] == before["seg_epos"][lm])


def test_masked_features_are_not_in_the_deque():
    s = K.seventy()
    mask = lambda sel: (np.array([i % 3 != 0 for i in range(len(sel["pt_lm"]))], np.uint8), np.zeros(len(sel["seg_lm"]), np.uint8))
    _, st, sel, w = restated(s, dict(max_n_pts=64, max_n_segs=20), mask)
    assert [int(v) for v in w["pt_lm"]] == [int(v) for i, v in enumerate(sel["pt_lm"]) if i % 3] and len(w["seg_lm"]) == 0 and not any(st["seg_last_optim"])
