"""The restatement of the map tables' compaction (tests/np_compact.py) against an independent statement of its invariants, on the cases of
tests/compact_cases.py -- and the cases themselves: that every path the kernel can take is in them.  CPU only."""
import copy

import compact_cases as K
import np_candidates as N
import np_compact as NK

PT_ROW = ("pt_pos", "pt_type", "pt_nfail", "pt_nsucc", "pt_obs")
SEG_ROW = ("seg_spos", "seg_epos", "seg_type", "seg_nfail", "seg_nsucc", "seg_obs")


def dead(st, name):
    return [lm for lm, t in enumerate(st[name + "_type"]) if t == N.TYPE_DELETED]


def test_the_cases_contain_every_path():
    cases = K.batch()
    assert len(cases) % 4 != 0 and len(cases) > 16                   # several workgroups, the last one partial
    seen = dict(pt=set(), seg=set())
    for s in cases:
        st = s["st"]
        for name in ("pt", "seg"):
            n = len(st[name + "_type"]) - len(st[name + "_cand"])
            d = set(dead(st, name))
            for pat in ("none", "all", "first", "last", "alternating", "run64", "behind129"):
                if n and d == K.dead_rows(pat, n):
                    seen[name].add((n, pat))
    for name in ("pt", "seg"):
        sizes = {n for n, _ in seen[name]}
        assert {1, 63, 64, 65, 130} <= sizes, (name, sizes)
        assert {"none", "all", "first", "last", "alternating", "run64", "behind129"} <= {p for _, p in seen[name]}, name
        assert any(len(s["st"][name + "_type"]) == 0 for s in cases)
        assert (130, "run64") in seen[name] and (130, "behind129") in seen[name]
        # deleted rows with a leftover list and with an emptied one
        assert any(st_obs for s in cases for lm in dead(s["st"], name) for st_obs in [s["st"][name + "_obs"][lm]] if st_obs)
        assert any(not s["st"][name + "_obs"][lm] for s in cases for lm in dead(s["st"], name))
        assert {0, 70} <= {len(s["st"][name + "_cand"]) for s in cases}
        assert any(len(o) > 64 and s["st"][name + "_type"][lm] != N.TYPE_DELETED for s in cases for lm, o in enumerate(s["st"][name + "_obs"]))
        # pin 7: a keyframe feature and a candidate entry on a deleted row
        assert any(lm >= 0 and s["st"][name + "_type"][lm] == N.TYPE_DELETED for s in cases for fts in s["st"]["kf_" + name] for lm in fts)
        assert any(s["st"][name + "_type"][lm] == N.TYPE_DELETED for s in cases for lm in s["st"][name + "_cand"])
    assert any(fts.count(lm) == 2 for s in cases for fts in s["st"]["kf_seg"] for lm in set(fts) if lm >= 0)      # a segment that is a feature twice
    assert any(s["st"]["pt_pos"] and not s["st"]["seg_spos"] for s in cases) and any(s["st"]["seg_spos"] and not s["st"]["pt_pos"] for s in cases)
    assert any(not s["st"]["kf_T"] and s["st"]["pt_pos"] for s in cases)
    assert sum(1 for s in cases if s["mode"][0] == NK.STANDBY) >= 2
    # mode 2 on both sides of its threshold, for each kind
    rooms = {(s["mode"][1] - K.LM_RESERVE["extra_pt"], s["mode"][2] - K.LM_RESERVE["extra_seg"]) for s in cases if s["mode"][0] == NK.ROOM}
    assert rooms == {(1, 0), (0, 1), (1, 1), (0, 0)}


def landmarks(st, name, events, keys):
    """per row everything that belongs to it, as one comparable value"""
    cols = [st[f] for f in (PT_ROW if name == "pt" else SEG_ROW)] + [events[name], keys[name]]
    return [tuple(copy.deepcopy(c[lm]) for c in cols) for lm in range(len(cols[0]))]


def test_the_restatement_keeps_its_invariants():
    for k, s in enumerate(K.batch()):
        before = copy.deepcopy(s["st"])
        st = copy.deepcopy(s["st"])
        ev0 = dict(pt=[(7 * i) % 5 for i in range(len(st["pt_pos"]))], seg=[(3 * i) % 7 for i in range(len(st["seg_spos"]))])
        events, keys = copy.deepcopy(ev0), copy.deepcopy(s["keys"])
        rows = K.rows_of(st)
        rep = K.compact(s, st, rows, events=events, keys=keys)
        mode, mp, ms = s["mode"]
        for name, min_room, room in (("pt", mp, K.LM_RESERVE["extra_pt"]), ("seg", ms, K.LM_RESERVE["extra_seg"])):
            old, new = landmarks(before, name, ev0, s["keys"]), landmarks(st, name, events, keys)
            ran = mode == NK.ALWAYS or (mode == NK.ROOM and room < min_room)
            assert rep["ran_" + name] == int(ran), (k, name)
            remap = rep[name + "_remap"]
            gone = dead(before, name) if ran else []
            # the live rows, whole and in order
            assert new == [r for lm, r in enumerate(old) if lm not in gone], (k, name)
            assert remap == [(-1 if lm in gone else lm - sum(1 for g in gone if g < lm)) for lm in range(len(old))], (k, name)
            if ran:
                assert not dead(st, name), (k, name)
            # every reference names the same landmark after as before
            n_rep = 0
            assert [len(f) for f in st["kf_" + name]] == [len(f) for f in before["kf_" + name]], (k, name)
            for fa, fb in zip(st["kf_" + name], before["kf_" + name]):
                for a, b in zip(fa, fb):
                    if b >= 0 and b in gone:
                        assert a == -1
                        n_rep += 1
                    else:
                        assert (a == -1 and b == -1) or new[a] == old[b], (k, name)
            kept = [lm for lm in before[name + "_cand"] if lm not in gone]
            assert [new[a] for a in st[name + "_cand"]] == [old[b] for b in kept], (k, name)
            assert all(0 <= a < len(new) for a in st[name + "_cand"]) and all(-1 <= a < len(new) for f in st["kf_" + name] for a in f), (k, name)
            # the sizes add up
            n_obs = lambda t: sum(len(o) for o in t[name + "_obs"])
            want = {"n_%s_before" % name: len(old), "n_%s_after" % name: len(old) - len(gone), "n_%s_obs_before" % name: n_obs(before),
                    "n_%s_obs_after" % name: n_obs(before) - sum(len(before[name + "_obs"][g]) for g in gone), "n_%s_cand_before" % name: len(before[name + "_cand"]),
                    "n_%s_cand_after" % name: len(kept), "n_repointed_" + name: n_rep, "n_erased_%s_cand" % name: len(before[name + "_cand"]) - len(kept)}
            assert {f: rep[f] for f in want} == want, (k, name, rep)
        # keyframe rows and seed-side state are not the compaction's
        assert st["kf_T"] == before["kf_T"] and st["kf_slot"] == before["kf_slot"], k
        if mode == NK.STANDBY:
            assert st == before and events == ev0 and keys == s["keys"], k
    assert sum(1 for s in K.batch() if s["mode"][0] == NK.ALWAYS) > 10


def test_the_remapped_case_follows_its_landmarks():
    s = K.batch()[0]
    st = copy.deepcopy(s["st"])
    rep = K.compact(s, st, K.rows_of(st))
    t = K.remapped(s, rep)
    live = [lm for lm, r in enumerate(rep["pt_remap"]) if r >= 0]
    assert [t["found_pt"][rep["pt_remap"][lm]] for lm in live] == [s["found_pt"][lm] for lm in live]
