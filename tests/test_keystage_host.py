"""tests/np_keystage.py against its own invariants and against tests/np_keyframe.py on gathered inputs (no device): the restatement of the
keyframe stage on the resident map tables is what tests/test_gpu_keystage.py compares the kernels with."""
import copy

import numpy as np

import candidates_cases as Cc
import insert_cases as Ic
import keyframe_cases as Kc
import np_keyframe as K
import np_keystage as NK


def streams():
    rng = np.random.default_rng(9500)
    return [Ic.random_stream(rng, n_kf, 60, 10, 3, 2, remove_kf=-1)["st"] for n_kf in (1, 3, 6)] + [s["st"] for s in Ic.batch()[:6]]


def test_fresh_key_points_are_np_keyframe_on_the_gathered_features():
    """a keyframe's row from five NULLs = set_key_points over its features' pixels with `holds a landmark` as alive; every holder holds a
    landmark; slot 0 is filled whenever a feature does"""
    for st in streams():
        tab = NK.fresh(st, Ic.CAM_T)
        assert tab.shape == (len(st["kf_T"]), 5)
        for k, l in enumerate(st["kf_pt"]):
            px = [NK.feature_px(st, k, lm) if lm >= 0 else None for lm in l]
            alive = [p is not None for p in px]
            want = K.set_key_points(Ic.CAM_T[4], Ic.CAM_T[5], np.array([p or [0.0, 0.0] for p in px]).reshape(-1, 2), alive, [-1] * 5)
            assert np.array_equal(tab[k], want)
            assert all(h < 0 or l[h] >= 0 for h in tab[k]) and (tab[k][0] >= 0) == any(alive)


def test_a_rebuild_happens_only_for_a_holder_and_keeps_the_survivors():
    rng = np.random.default_rng(9501)
    n_rebuilt = n_quiet = 0
    for st in streams():
        tab = NK.fresh(st, Ic.CAM_T)
        held = [lm for l in st["kf_pt"] for lm in l if lm >= 0]
        for lm in rng.permutation(sorted(set(held)))[:12]:
            lm = int(lm)
            holders = {k for k, l in enumerate(st["kf_pt"]) if any(h >= 0 and l[h] == lm for h in tab[k])}
            new, rebuilt = NK.sequential_upkeep(st, tab, Ic.CAM_T, [lm])
            assert set(rebuilt) == holders
            for k in range(len(tab)):
                if k not in holders:
                    assert np.array_equal(new[k], tab[k])               # no holder lost: not even a better feature is taken
                else:
                    assert all(h < 0 or st["kf_pt"][k][h] != lm for h in new[k])
            after = copy.deepcopy(st)
            after["kf_pt"] = [[-1 if v == lm else v for v in l] for l in st["kf_pt"]]
            assert np.array_equal(NK.batched_upkeep(after, tab, Ic.CAM_T), new)       # one deletion: the two forms are the same
            n_rebuilt += len(holders); n_quiet += int(not holders)
    assert n_rebuilt > 10 and n_quiet > 3


def test_sequential_and_batched_forms_agree_on_random_deletions():
    rng = np.random.default_rng(9502)
    for st in streams():
        tab = NK.fresh(st, Ic.CAM_T)
        held = sorted({lm for l in st["kf_pt"] for lm in l if lm >= 0})
        gone = [int(v) for v in rng.permutation(held)[: len(held) // 3]]
        after = copy.deepcopy(st)
        after["kf_pt"] = [[-1 if v in gone else v for v in l] for l in st["kf_pt"]]
        assert NK.deleted_landmarks(st, after) == sorted(gone)
        seq, _ = NK.sequential_upkeep(st, tab, Ic.CAM_T, gone)
        assert np.array_equal(seq, NK.batched_upkeep(after, tab, Ic.CAM_T))


def test_close_is_np_keyframe_on_the_gathered_table_and_reads_live_positions():
    rng = np.random.default_rng(9503)
    st = Cc.rand_stream(rng, [(6, 1)] * 12, 40, 4, max_obs=3)
    tab = NK.fresh(st, Cc.CAM_T)
    T = Cc.rand_pose(rng, 0.5, 0.8)
    r = NK.close(st, tab, T, Cc.CAM_T, 4)
    assert r["n_overlap"] == min(4, r["n_close"]) and np.all(np.diff(r["close_dist"]) >= 0)
    for k in range(12):
        vis = any(h >= 0 and st["kf_pt"][k][h] >= 0 and K.is_visible(T, Cc.CAM_T, st["pt_pos"][st["kf_pt"][k][h]]) for h in tab[k])
        assert vis == (k in r["close_idx"])
    moved = copy.deepcopy(st)
    for k in r["close_idx"][:2]:
        for h in tab[k]:
            if h >= 0 and st["kf_pt"][k][h] >= 0:
                moved["pt_pos"][st["kf_pt"][k][h]] = [0.0, 0.0, -1.0]      # behind the camera
    r2 = NK.close(moved, tab, T, Cc.CAM_T, 4)
    assert not set(r["close_idx"][:2]) & set(r2["close_idx"])


def test_decide_is_np_keyframe_on_the_gathered_selection():
    rng = np.random.default_rng(9504)
    s = Ic.batch()[4]
    st = copy.deepcopy(s["st"])
    _, _, sel = Ic.frame(s, st)
    pk, sk = Ic.keep_masks(s, sel)
    T_new, T_last = Kc.rand_pose(rng, 0.05, 0.1), Kc.rand_pose(rng, 0.05, 0.1)
    got = NK.decide(st, sel, pk, sk, T_new, T_last, s["overlap"], Ic.CAM_T)
    job = Ic.Sc.abi.KeyframeDecideJob(Ic.CAM, T_new, T_last, sel["pt_px"], [st["pt_pos"][lm] for lm in sel["pt_lm"]], pk, [st["seg_spos"][lm] for lm in sel["seg_lm"]],
                                      [st["seg_epos"][lm] for lm in sel["seg_lm"]], sk, st["kf_T"], list(s["overlap"]), [-1] * 5)
    want = K.decide(job)
    assert got.keys() == want.keys() and got["n_depth"] == int(pk.sum()) + 2 * int(sk.sum()) > 10
    for f in want:
        assert np.asarray(got[f]).tobytes() == np.asarray(want[f]).tobytes(), f
