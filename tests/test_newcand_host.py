"""The restatement of the new map candidates (tests/np_newcand.py) on the CPU: that the cases of tests/newcand_cases.py hold every size and
choice -- asserted on the inputs -- and that the restatement keeps an independent statement of its invariants.  These tests need no kernel
and pass without the feature: they test the restatement, not the device."""
import copy

import pytest

import insert_cases as Ic
import newcand_cases as Nc
import np_candidates as N
import np_newcand as NC


@pytest.fixture(scope="module")
def results():
    out = []
    for s in Nc.batch():
        st = copy.deepcopy(s["st"])
        rep = Nc.add(s, st)
        out.append((s, st, rep))
    return out


def test_the_batch_holds_every_size_and_choice():
    cases = Nc.batch()
    counts = [(len(s["new"]["pt"]), len(s["new"]["seg"])) for s in cases]
    assert counts == list(Nc.COUNTS)
    assert {0, 1, 63, 64, 65, 130} <= {a for a, _ in counts} and {0, 1, 63, 64, 65, 130} <= {b for _, b in counts}
    assert len(cases) >= 10 and len(cases) % 4                                       # more than two workgroups, the last one partial
    assert any(a > 0 and b == 0 for a, b in counts) and any(a == 0 and b > 0 for a, b in counts) and sum(a + b == 0 for a, b in counts) >= 3
    assert any(a + b == 0 and counts[k - 1] != (0, 0) and counts[k + 1] != (0, 0) for k, (a, b) in enumerate(counts[:-1]) if k)   # standing by between two that add
    adding = [s for s, c in zip(cases, counts) if c != (0, 0)]
    assert any(len(s["st"]["pt_pos"]) == 0 and s["new"]["pt"] for s in adding) and any(len(s["st"]["seg_spos"]) == 0 and s["new"]["seg"] for s in adding)
    assert any(not s["st"]["pt_cand"] and not s["st"]["seg_cand"] for s in adding) and any(s["st"]["pt_cand"] and s["st"]["seg_cand"] for s in adding)
    assert any(len(s["st"]["pt_cand"]) > 64 for s in adding)                          # a list longer than a round grows
    edgelets = [p["obs"] for s in cases for p in s["new"]["pt"] if p["obs"]["type"] == 1]
    assert len(edgelets) > 20 and all(o["grad"] == [0.6, 0.8] for o in edgelets)
    for s in cases:                                                                   # an observation above every staged level
        staged = [o["level"] for l in s["st"]["pt_obs"] + s["st"]["seg_obs"] for o in l]
        assert not staged or max(staged) < Nc.HIGH_LEVEL
    assert any(p["obs"]["level"] == Nc.HIGH_LEVEL for s in cases for p in s["new"]["pt"]) and any(q["obs"]["level"] == Nc.HIGH_LEVEL for s in cases for q in s["new"]["seg"])
    for s in adding:                                                                  # observations in the first and in the last keyframe
        n_kf = len(s["st"]["kf_T"])
        kfs = [r["obs"]["kf"] for r in s["new"]["pt"] + s["new"]["seg"]]
        assert all(0 <= k < n_kf for k in kfs)
        if len(s["new"]["pt"]) >= 2 or len(s["new"]["seg"]) >= 2:
            assert 0 in kfs and n_kf - 1 in kfs
    assert any(len(s["st"]["kf_T"]) == 0 for s in cases)                              # a map without keyframes stands by


def test_untouched_landmarks_and_lists_are_byte_equal(results):
    for s, st, _ in results:
        old = s["st"]
        for name, fields in (("pt", ("pt_pos", "pt_type", "pt_obs", "pt_nfail", "pt_nsucc")), ("seg", ("seg_spos", "seg_epos", "seg_type", "seg_obs", "seg_nfail", "seg_nsucc"))):
            n = len(old[fields[0]])
            for f in fields:
                assert st[f][:n] == old[f] and repr(st[f][:n]) == repr(old[f]), f
        for f in ("kf_T", "kf_slot", "kf_pt", "kf_seg"):
            assert st[f] == old[f], f
        assert Ic.sizes(st)["n_kf_pt"] == Ic.sizes(old)["n_kf_pt"] and Ic.sizes(st)["n_kf_seg"] == Ic.sizes(old)["n_kf_seg"]


def test_every_new_landmark_is_a_candidate_with_one_observation_no_keyframe_holds(results):
    for s, st, rep in results:
        for name, pos in (("pt", "pt_pos"), ("seg", "seg_spos")):
            n_old, n_new = len(s["st"][pos]), len(s["new"][name])
            assert rep["n_added_" + name] == n_new and rep["first_" + name] == (n_old if n_new else -1)
            assert rep[name + "_event"] == [0] * n_old + [NC.EVENT_NEW] * n_new
            for j in range(n_new):
                lm = n_old + j
                rec = s["new"][name][j]
                assert st[name + "_type"][lm] == N.TYPE_CANDIDATE and st[name + "_nfail"][lm] == 0 and st[name + "_nsucc"][lm] == 0
                obs = st[name + "_obs"][lm]
                assert len(obs) == 1 and 0 <= obs[0]["kf"] < len(st["kf_T"])
                assert all(lm not in fts for fts in st["kf_" + name])                   # the seed's feature is not in its keyframe's list
                for f, v in rec["obs"].items():                                         # the record, passed through unchanged
                    assert obs[0][f] == v and repr(obs[0][f]) == repr(v if not isinstance(v, (list, tuple)) else [float(x) for x in v]), (name, lm, f)
                if name == "pt":
                    assert st["pt_pos"][lm] == [float(v) for v in rec["pos"]]
                else:
                    assert st["seg_spos"][lm] == [float(v) for v in rec["spos"]] and st["seg_epos"][lm] == [float(v) for v in rec["epos"]]


def test_the_candidate_list_is_the_old_list_plus_the_new_indices_in_order_and_counts_add_up(results):
    for s, st, rep in results:
        for name, pos in (("pt", "pt_pos"), ("seg", "seg_spos")):
            n_old, n_new = len(s["st"][pos]), len(s["new"][name])
            assert st[name + "_cand"] == s["st"][name + "_cand"] + list(range(n_old, n_old + n_new))
            assert len(st[pos]) == len(st[name + "_type"]) == len(st[name + "_obs"]) == len(st[name + "_nfail"]) == len(st[name + "_nsucc"]) == n_old + n_new
        before, after = Ic.sizes(s["st"]), Ic.sizes(st)
        assert after["n_pt_obs"] == before["n_pt_obs"] + len(s["new"]["pt"]) and after["n_seg_obs"] == before["n_seg_obs"] + len(s["new"]["seg"])
        assert after["n_pt_cand"] == before["n_pt_cand"] + len(s["new"]["pt"]) and after["n_kf"] == before["n_kf"]


def test_the_grown_tables_keep_the_insertion_s_preconditions_and_the_next_frame_uses_them(results):
    """a frame and an insertion behind the add on the restatement: new candidates are filed and matched, the kept ones join their keyframe
    (TYPE_UNKNOWN, their original feature appended), those observed in the removed keyframe are deleted and erased"""
    joined = deleted = 0
    for s, st0, _ in results:
        if not st0["kf_T"]:
            continue
        st = copy.deepcopy(st0)
        n_old = len(s["st"]["pt_pos"])
        new_lm = set(range(n_old, len(st["pt_pos"])))
        _, _, sel = Ic.frame(s, st)
        remove = Nc.removal_of(s, st)
        in_removed = {lm for lm in new_lm if st["pt_obs"][lm][-1]["kf"] == remove and lm in st["pt_cand"]}
        out = Ic.insert(s, st, sel, remove_kf=remove)
        for lm in new_lm:
            if out["pt_event"][lm] & 4:
                joined += 1
                assert st["pt_type"][lm] in (N.TYPE_UNKNOWN, N.TYPE_DELETED) and lm not in st["pt_cand"]
        for lm in in_removed:
            if not out["pt_event"][lm] & 4:
                deleted += 1
                assert st["pt_type"][lm] == N.TYPE_DELETED and lm not in st["pt_cand"] and st["pt_obs"][lm] == []
    assert joined > 40 and deleted > 10
