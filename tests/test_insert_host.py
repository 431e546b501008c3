"""The restatement of the keyframe insertion (tests/np_insert.py) on the CPU: that the cases of tests/insert_cases.py hold every path --
asserted on the inputs and on what the restatement does with them -- and that the restatement keeps an independent statement of its
invariants.  These tests need no kernel and pass without the feature: they test the restatement, not the device."""
import copy

import numpy as np
import pytest

import insert_cases as Ic
import np_candidates as N
import np_insert as I

D, C_, U, G = Ic.D, Ic.C_, Ic.U, Ic.G


def run(s, st=None):
    """one frame and the insertion behind it on a copy: (tables before the insertion, selection, report, tables after)"""
    st = copy.deepcopy(s["st"]) if st is None else st
    _, _, sel = Ic.frame(s, st)
    before = copy.deepcopy(st)
    out = Ic.insert(s, st, sel) if s["is_kf"] else None
    return before, sel, out, st


@pytest.fixture(scope="module")
def results():
    return [run(s) for s in Ic.batch()]


def test_the_batch_holds_every_size_and_choice(results):
    streams = Ic.batch()
    pt_sizes = {len(l) for s in streams for l in s["st"]["kf_pt"]}
    seg_sizes = {len(l) for s in streams for l in s["st"]["kf_seg"]}
    assert {0, 1, 63, 64, 65, 130} <= pt_sizes and {0, 1, 63, 64, 65, 130} <= seg_sizes
    sizes = Ic.sizes_stream()
    assert len(sizes["st"]["kf_pt"][sizes["remove_kf"]]) == 64                       # the removed list is exactly one round
    feats = [(sel["n_matches"], sel["n_ls_matches"]) for _, sel, _, _ in results]
    assert feats[7] == (0, 0) and streams[7]["is_kf"]                                # a new frame with 0 features
    pk, sk = Ic.keep_masks(streams[9], results[9][1])
    assert feats[9][0] >= 65 and not pk.any() and not sk.any()                       # every feature culled
    assert feats[10][0] >= 65 and Ic.keep_masks(streams[10], results[10][1])[0].all()   # 65 point features and more
    removed = [(s["remove_kf"], len(s["st"]["kf_T"])) for s in streams if s["is_kf"]]
    assert any(r == 0 and n > 2 for r, n in removed) and any(0 < r < n - 1 for r, n in removed) and any(r == n - 1 and n > 1 for r, n in removed)
    assert any(r == -1 for r, _ in removed)
    flags = [s["is_kf"] for s in streams]
    assert any(not flags[k - 1] and flags[k] and not flags[k + 1] for k in range(1, len(flags) - 1))   # an inserting stream between two that stand by
    assert len(streams) > 8 and len(streams) % 4                                     # more than two workgroups, the last one partial
    assert len(Ic.first_keyframe_stream()["st"]["kf_T"]) == 0 and results[12][3]["kf_T"] == [Ic.T_NEW]
    assert len(streams[11]["st"]["pt_cand"]) > 64 and results[11][2]["n_joined_pt"] > 64     # more than a round of candidates joins


def test_the_directed_stream_reaches_every_path():
    s = Ic.directed_stream()
    nm, R = s["names"], s["remove_kf"]
    before, sel, out, st = run(s)
    new = out["new_kf"]
    shift = lambda k: k - 1 if k > R else k
    kfs = lambda obs: [o["kf"] for o in obs]
    is_ftr = lambda lm: lm in sel["pt_lm"]
    # observation lists of 1, 2, 3 and 7 entries on both sides of the <= 2 rule
    for n_obs in (1, 2, 3, 7):
        for found in (0, 1):
            lm = nm["obs%d_found%d" % (n_obs, found)]
            assert len(s["st"]["pt_obs"][lm]) == n_obs and R in kfs(s["st"]["pt_obs"][lm]) and is_ftr(lm) == bool(found)
            if n_obs + found <= 2:
                assert st["pt_type"][lm] == D and st["pt_obs"][lm] == [] and out["pt_event"][lm] == I.EVENT_DELETED
                assert all(lm not in l for l in st["kf_pt"])
            else:
                assert st["pt_type"][lm] == G and len(st["pt_obs"][lm]) == n_obs + found - 1 and out["pt_event"][lm] == 0
                assert kfs(st["pt_obs"][lm]) == ([new] if found else []) + [shift(k) for k in kfs(s["st"]["pt_obs"][lm]) if k != R]
                assert (lm in st["kf_pt"][new]) == bool(found)
    lm = nm["culled_in_removed"]
    assert is_ftr(lm) and st["kf_pt"][new][sel["pt_lm"].index(lm)] == -1 and st["pt_type"][lm] == D          # rejected: no new observation, 2 -> deleted
    lm = nm["untouched"]
    assert st["pt_obs"][lm][1:] == s["st"]["pt_obs"][lm] and st["pt_obs"][lm][0]["kf"] == new
    lm = nm["edgelet"]
    assert st["pt_obs"][lm][0]["type"] == 1 and st["pt_obs"][lm][0]["grad"] != [1.0, 0.0] and st["pt_obs"][lm][0]["kf"] == new
    lm = nm["deleted_earlier"]
    assert before["pt_type"][lm] == D and kfs(st["pt_obs"][lm]) == [shift(4), shift(R + 2)] and out["pt_event"][lm] == 0
    lm = nm["deleted_by_selection"]
    assert s["st"]["pt_type"][lm] == U and before["pt_type"][lm] == D and kfs(st["pt_obs"][lm]) == [shift(6), shift(7)]
    # candidates
    lm = nm["cand_joins_removed"]
    assert is_ftr(lm) and lm in before["pt_cand"] and lm not in st["pt_cand"] and out["pt_event"][lm] == I.EVENT_JOINED | I.EVENT_DELETED
    assert st["pt_type"][lm] == D and st["pt_nfail"][lm] == 0 and st["kf_pt"][new][sel["pt_lm"].index(lm)] == -1
    lm = nm["cand_unmatched_removed"]
    assert not is_ftr(lm) and lm not in st["pt_cand"] and st["pt_type"][lm] == D and st["pt_obs"][lm] == [] and out["pt_event"][lm] == I.EVENT_DELETED
    lm = nm["cand_unmatched_stays"]
    assert lm in st["pt_cand"] and st["pt_type"][lm] == C_ and kfs(st["pt_obs"][lm]) == [2]
    lm = nm["cand_culled"]
    assert is_ftr(lm) and lm in st["pt_cand"] and st["pt_type"][lm] == C_ and len(st["pt_obs"][lm]) == 1 and lm not in st["kf_pt"][new]
    a, b = nm["cand_pair"]
    assert before["pt_cand"].index(a) < before["pt_cand"].index(b) and sel["pt_lm"].index(a) > sel["pt_lm"].index(b)     # list order against feature order
    assert st["kf_pt"][shift(6)][-2:] == [a, b] and st["pt_type"][a] == st["pt_type"][b] == U and out["pt_event"][a] == I.EVENT_JOINED
    # segments
    lm = nm["seg_twice_in_removed"]
    assert before["kf_seg"][R].count(lm) == 2 and sel["seg_lm"].count(lm) == 1 and st["seg_type"][lm] == D and st["seg_obs"][lm] == []
    assert st["kf_seg"][new][sel["seg_lm"].index(lm)] == -1
    lm = nm["seg_wins_both"]
    i0, i1 = [i for i, v in enumerate(sel["seg_lm"]) if v == lm]
    assert kfs(st["seg_obs"][lm]) == [new, new, 0, 1] and st["seg_obs"][lm][0]["level"] == sel["seg_level"][i1] and st["seg_obs"][lm][1]["level"] == sel["seg_level"][i0]
    assert st["seg_obs"][lm][0]["spx"] == sel["seg_px"][i1][0:2] and st["kf_seg"][new].count(lm) == 2
    lm = nm["seg_wins_both_removed"]
    assert kfs(st["seg_obs"][lm]) == [new, new, 2, shift(4)] and st["seg_type"][lm] == G
    lm = nm["seg_unmatched_removed"]
    assert lm not in sel["seg_lm"] and st["seg_type"][lm] == D and all(lm not in l for l in st["kf_seg"])
    lm = nm["seg_cand_joins"]
    assert st["seg_type"][lm] == U and st["kf_seg"][shift(5)][-1] == lm and lm not in st["seg_cand"]
    lm = nm["seg_cand_unmatched_removed"]                                              # pinned: the reference leaves it listed
    assert lm not in sel["seg_lm"] and lm in before["seg_cand"] and lm not in st["seg_cand"] and st["seg_type"][lm] == D
    lm = nm["seg_cand_stays"]
    assert lm in st["seg_cand"] and st["seg_type"][lm] == C_
    lm = nm["seg_cand_joins_removed"]
    assert st["seg_type"][lm] == D and out["seg_event"][lm] == I.EVENT_JOINED | I.EVENT_DELETED
    assert len(st["kf_T"]) == 8 and st["kf_T"][new] == Ic.T_NEW and st["kf_slot"][new] == s["kf_slot"]


def test_a_feature_on_a_deleted_landmark_has_no_landmark():
    """pinned: with a deterministic matcher the selection never leaves such a feature, so it is constructed -- the landmark of the second
    feature is deleted between the selection and the insertion"""
    s = Ic.directed_stream()
    st = copy.deepcopy(s["st"])
    _, _, sel = Ic.frame(s, st)
    lm = s["names"]["untouched"]
    st["pt_type"][lm] = D
    obs = copy.deepcopy(st["pt_obs"][lm])
    out = Ic.insert(s, st, sel)
    assert st["kf_pt"][out["new_kf"]][sel["pt_lm"].index(lm)] == -1 and [o["kf"] for o in st["pt_obs"][lm]] == [o["kf"] for o in obs]
    assert st["pt_type"][lm] == D and out["pt_event"][lm] == 0 and out["n_deleted_pt"] == run(s)[2]["n_deleted_pt"]


def test_the_restatement_keeps_its_invariants(results):
    """an independent statement: every observation's keyframe holds a feature with that landmark, or it is a candidate's original; no index
    refers to a row outside the table; untouched landmarks keep their lists; counts add up"""
    for k, (s, (before, sel, out, st)) in enumerate(zip(Ic.batch(), results)):
        if out is None:
            assert st == before
            continue
        R, n_before, n_kf = s["remove_kf"], len(before["kf_T"]), len(st["kf_T"])
        assert n_kf == n_before + 1 - (R >= 0) == len(st["kf_slot"]) == len(st["kf_pt"]) == len(st["kf_seg"]) and out["new_kf"] == n_kf - 1
        pk, sk = Ic.keep_masks(s, sel)
        for name, keep in (("pt", pk), ("seg", sk)):
            obs, types, cand, lists = st[name + "_obs"], st[name + "_type"], st[name + "_cand"], st["kf_" + name]
            for lm, l in enumerate(obs):
                for o in l:
                    assert 0 <= o["kf"] < n_kf, (k, name, lm)
                    if types[lm] != D:
                        assert lm in lists[o["kf"]] or (lm in cand and len(l) == 1), (k, name, lm)
                if types[lm] != D:
                    for kf in range(n_kf):
                        assert lists[kf].count(lm) == [o["kf"] for o in l].count(kf) or lm in cand, (k, name, lm, kf)
                elif out[name + "_event"][lm] & I.EVENT_DELETED:
                    assert l == []
                if types[lm] == D:
                    assert all(lm not in f for f in lists) and lm not in cand
            touched = {int(lm) for lm in sel[name + "_lm"]} | {lm for lm in range(len(obs)) if R >= 0 and R in [o["kf"] for o in before[name + "_obs"][lm]]}
            for lm in set(range(len(obs))) - touched:
                want = [dict(o, kf=o["kf"] - (R >= 0 and o["kf"] > R)) for o in before[name + "_obs"][lm]]
                assert obs[lm] == want and types[lm] == before[name + "_type"][lm] and out[name + "_event"][lm] == 0, (k, name, lm)
            n_new = sum(1 for i, lm in enumerate(sel[name + "_lm"]) if keep[i] and before[name + "_type"][lm] != D)
            assert sum(1 for v in st["kf_" + name][-1] if v >= 0) <= n_new and len(st["kf_" + name][-1]) == len(sel[name + "_lm"])
            gone = sum(len(before[name + "_obs"][lm]) + sum(1 for i, v in enumerate(sel[name + "_lm"]) if v == lm and keep[i]) for lm in range(len(obs))
                       if out[name + "_event"][lm] & I.EVENT_DELETED)
            erased = sum(1 for lm in range(len(obs)) for o in before[name + "_obs"][lm] if o["kf"] == R and not out[name + "_event"][lm] & I.EVENT_DELETED) if R >= 0 else 0
            assert sum(map(len, obs)) == sum(map(len, before[name + "_obs"])) + n_new - gone - erased, (k, name)
            assert len(cand) == len(before[name + "_cand"]) - out["n_joined_" + name] - sum(1 for lm in before[name + "_cand"] if st[name + "_type"][lm] == D and
                                                                                              not out[name + "_event"][lm] & I.EVENT_JOINED), (k, name)
            assert out["n_deleted_" + name] == sum(1 for e in out[name + "_event"] if e & I.EVENT_DELETED) and out["n_joined_" + name] == sum(1 for e in out[name + "_event"] if e & I.EVENT_JOINED)
            n_ftr = sum(map(len, before["kf_" + name])) - (len(before["kf_" + name][R]) if R >= 0 else 0) + len(sel[name + "_lm"])
            joined_kept = sum(1 for lm in before[name + "_cand"] if out[name + "_event"][lm] & I.EVENT_JOINED and (R < 0 or before[name + "_obs"][lm][-1]["kf"] != R))
            assert sum(map(len, st["kf_" + name])) == n_ftr + joined_kept, (k, name)


def test_fetch_layout_of_the_restatement_is_the_stage_layout():
    """Ic.tables() gives what plsvo_candidates_stage takes: staging the restatement's tables and fetching them must be the identity"""
    st = run(Ic.directed_stream())[3]
    t = Ic.tables(st)
    assert t["kf_T"].shape == (8, 7) and t["kf_pt_off"][-1] == t["kf_pt_lm"].size and t["pt_obs_off"][-1] == t["pt_obs_kf"].size == len(t["pt_obs_px"])
    assert t["seg_obs_off"][-1] == t["seg_obs_kf"].size and t["pt_obs_kf"].max() == 7 and np.all(t["kf_T"][7] == Ic.T_NEW)
