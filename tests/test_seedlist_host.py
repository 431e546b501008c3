"""The restatement of the resident seed lists (tests/np_seedlist.py) on the CPU: that the cases of tests/seedlist_cases.py hold every size
and choice -- asserted on the inputs -- that the restatement keeps an independent statement of its invariants, and that its update equals
the oracle-backed host path (the oracle's per-seed body, the caller's lists).  These tests need no kernel and pass without the feature:
they test the restatement, not the device."""
import copy
import importlib

import numpy as np
import pytest

import candidates_cases as Cc
import insert_cases as Ic
import np_candidates as N
import np_seedlist as SL
import seedlist_cases as Sl


@pytest.fixture(scope="module")
def results():
    out = []
    for c in Sl.batch():
        st, sd = copy.deepcopy(c["st"]), copy.deepcopy(c["seeds"])
        rep, ev = Sl.commit(c, sd, st, Sl.room_of(c["st"]))
        out.append((c, st, sd, rep, ev))
    return out


def test_the_batch_holds_every_size_and_choice():
    cases = Sl.batch()
    counts = [(len(c["seeds"]["pt"]), len(c["seeds"]["seg"])) for c in cases]
    assert counts == [((0, 0) if not c["st"]["kf_T"] else n) for c, n in zip(cases, Sl.SEEDS)]
    assert {0, 1, 63, 64, 65, 130} <= {a for a, _ in counts} and {0, 1, 63, 64, 65, 130} <= {b for _, b in counts}
    conv = [tuple(sum(r["status"] == SL.CONVERGED for r in c["rows"][k]) for k in ("pt", "seg")) for c in cases if c["active"]]
    assert {0, 1, 63, 64, 65, 130} <= {a for a, _ in conv} and {0, 1, 63, 64, 65, 130} <= {b for _, b in conv}
    assert len(cases) >= 10 and len(cases) % 4                                       # more than two workgroups of four waves, the last one partial
    assert any(a > 0 and b == 0 for a, b in counts) and any(a == 0 and b > 0 for a, b in counts)
    assert any(not c["active"] and c["seeds"]["pt"] for c in cases) and any(not c["st"]["kf_T"] for c in cases)
    mixed = [c for c in cases if c["pattern"] == "mixed" and len(c["rows"]["pt"]) > 64]
    assert mixed
    for c in mixed:                                                                   # every status in one round and across rounds, converged rows between the others
        st = [r["status"] for r in c["rows"]["pt"]]
        assert set(st[:64]) == set(st[64:128]) == {0, 1, 2, 3, 4, 5}
        assert any(st[j] == SL.CONVERGED and st[j + 1] != SL.CONVERGED and st[j + 2] == SL.CONVERGED for j in range(62))
    assert any(c["pattern"] == "aged" and all(r["status"] == SL.AGED for r in c["rows"]["pt"] + c["rows"]["seg"]) for c in cases)
    assert any(c["pattern"] == "converged" and len(c["rows"]["pt"]) == 130 for c in cases)
    for c in cases:                                                                   # a row is aged exactly where the batch ids say so; several batch ids
        sd = c["seeds"]
        for kind in ("pt", "seg"):
            assert [r["status"] == SL.AGED for r in c["rows"][kind]] == [SL.aged(sd, x, Sl.MAX_N_KFS) for x in sd[kind]]
            kfs = [x["ref_kf"] for x in sd[kind]]
            assert all(0 <= k < len(c["st"]["kf_T"]) for k in kfs)
            if len(kfs) >= 2:
                assert 0 in kfs and len(c["st"]["kf_T"]) - 1 in kfs                   # seeds in the first and in the last keyframe
    assert len({x["batch_id"] for c in cases for x in c["seeds"]["pt"]}) >= 5
    edgelets = [x for c in cases for x in c["seeds"]["pt"] if x["type"] == 1]
    assert len(edgelets) > 20 and all(x["grad"] == [0.6, 0.8] for x in edgelets)


def test_the_lists_close_up_in_order_and_the_kept_seeds_take_the_body_s_parameters(results):
    for c, st, sd, rep, _ in results:
        if not c["active"]:
            assert sd == c["seeds"] and st == c["st"] and sum(rep["pt"]) + sum(rep["seg"]) == 0
            continue
        for kind, params in (("pt", SL.PT_PARAMS), ("seg", SL.SEG_PARAMS)):
            kept = [(x, r) for x, r in zip(c["seeds"][kind], c["rows"][kind]) if r["status"] in (SL.NOT_VISIBLE, SL.NO_MATCH, SL.UPDATED)]
            assert len(sd[kind]) == len(kept) == rep["n_%s_seeds" % kind]
            for now, (x, r) in zip(sd[kind], kept):
                assert all(now[k] == x[k] and repr(now[k]) == repr(x[k]) for k in x if k not in params)
                assert all(np.float32(now[p]).tobytes() == np.float32(r[p]).tobytes() for p in params)
            assert rep[kind] == [sum(r["status"] == k for r in c["rows"][kind]) for k in range(6)]
        assert rep["batch_counter"] == c["seeds"]["batch_counter"] == sd["batch_counter"]


def test_converged_seeds_become_candidates_in_list_order_exactly_as_an_add_writes_them(results):
    for c, st, sd, rep, ev in results:
        if not c["active"]:
            continue
        for kind, pos in (("pt", "pt_pos"), ("seg", "seg_spos")):
            n_old = len(c["st"][pos])
            conv = [(x, r) for x, r in zip(c["seeds"][kind], c["rows"][kind]) if r["status"] == SL.CONVERGED]
            assert len(st[pos]) == n_old + len(conv) and rep["first_" + kind] == (n_old if conv else -1)
            assert st[kind + "_cand"] == c["st"][kind + "_cand"] + list(range(n_old, n_old + len(conv)))
            assert ev[0 if kind == "pt" else 1] == [0] * n_old + [8] * len(conv)
            for j, (x, r) in enumerate(conv):
                lm = n_old + j
                assert st[kind + "_type"][lm] == N.TYPE_CANDIDATE and st[kind + "_nfail"][lm] == 0 and st[kind + "_nsucc"][lm] == 0
                obs = st[kind + "_obs"][lm]
                assert len(obs) == 1 and obs[0]["kf"] == x["ref_kf"] and obs[0]["level"] == x["level"]
                if kind == "pt":
                    assert st["pt_pos"][lm] == r["xyz"] and (obs[0]["px"], obs[0]["f"], obs[0]["type"], obs[0]["grad"]) == (x["px"], x["f"], x["type"], x["grad"])
                else:
                    assert (st["seg_spos"][lm], st["seg_epos"][lm]) == (r["xyz_s"], r["xyz_e"])
                    assert (obs[0]["spx"], obs[0]["epx"], obs[0]["sf"], obs[0]["ef"]) == (x["spx"], x["epx"], x["sf"], x["ef"])
        z0, z1 = Ic.sizes(c["st"]), Ic.sizes(st)
        assert z1["n_kf_pt"] == z0["n_kf_pt"] and z1["n_kf"] == z0["n_kf"] and (rep["n_pt_obs"], rep["n_seg_obs"]) == (z1["n_pt_obs"], z1["n_seg_obs"])


def test_no_room_is_all_or_nothing_per_stream():
    c = Sl.batch()[7]
    conv = [sum(r["status"] == SL.CONVERGED for r in c["rows"][k]) for k in ("pt", "seg")]
    full = Sl.room_of(c["st"], dict(extra_pt=conv[0], extra_seg=conv[1]), dict(extra_pt_obs=conv[0], extra_seg_obs=conv[1]))
    for short in (None, "rows_pt", "rows_seg", "cap_pt_obs", "cap_seg_obs", "rows_pt_cand", "rows_seg_cand"):
        room = dict(full)
        if short:
            room[short] -= 1
        st, sd = copy.deepcopy(c["st"]), copy.deepcopy(c["seeds"])
        rep, ev = SL.commit(sd, st, c["rows"], room)
        assert rep["no_room"] == (1 if short else 0)
        if short:
            assert st == c["st"] and sd == c["seeds"] and ev == (None, None) and rep["n_pt"] == len(st["pt_pos"]) and rep["pt"][SL.CONVERGED] == conv[0]


def test_keyframe_event_erases_renumbers_and_appends_with_the_constructor_s_float_arithmetic():
    seqm = importlib.import_module("pl-svo_amd.sequence")
    rng = np.random.default_rng(3)
    for c in Sl.batch():
        n_kf = len(c["st"]["kf_T"])
        if n_kf < 3 or not c["seeds"]["pt"]:
            continue
        for removed in (0, n_kf // 2, n_kf - 1, -1):
            sd = copy.deepcopy(c["seeds"])
            pt, seg = Sl.new_features(rng, c["st"], c, 3, 2)
            SL.keyframe(sd, removed, True, n_kf - 1, 2.75, 0.6, pt, seg)
            assert sd["batch_counter"] == c["seeds"]["batch_counter"] + 1
            for kind, n_new in (("pt", 3), ("seg", 2)):
                old = [x for x in c["seeds"][kind] if x["ref_kf"] != removed or removed < 0]
                assert len(sd[kind]) == len(old) + n_new
                for now, x in zip(sd[kind], old):
                    assert now["ref_kf"] == x["ref_kf"] - (1 if 0 <= removed < x["ref_kf"] else 0) and all(now[k] == x[k] for k in x if k != "ref_kf")
                for now in sd[kind][len(old):]:
                    assert now["ref_kf"] == n_kf - 1 and now["batch_id"] == sd["batch_counter"] and now["a"] == now["b"] == 10
        # the point half equals sequence.seeds_from_corners, which restates the same constructor
        corners = np.zeros(3, dtype=Cc.abi.CORNER_DTYPE)
        corners["x"], corners["y"] = [10, 20, 30], [12, 22, 32]
        want = seqm.seeds_from_corners(corners, Sl.CAM_T, 2.75, 0.6)
        got = SL.new_point_seed(dict(px=[0, 0], f=[0, 0, 1], level=0, type=0, grad=[1, 0]), 0, 0, 2.75, 0.6)
        for k in ("a", "b", "mu", "z_range", "sigma2"):
            assert np.float32(got[k]).tobytes() == want[k][0].tobytes(), k
        return
    raise AssertionError("no case with three keyframes")


def test_update_equals_the_oracle_backed_host_path(P, ob):
    """np_seedlist.update with the oracle's per-seed body against the host path written out: the caller ages its lists, calls the seed
    update on what is left, erases converged and NaN seeds and appends the converged ones with np_newcand.add"""
    import np_newcand as NC
    seqm = importlib.import_module("pl-svo_amd.sequence")
    seq = seqm.make_sequence(26, n_frames=3, W=320, H=240, n_pts=40, n_seg=8, step_scale=1.0)
    frames = [ob.build_pyramid(im, 4) for im in seq["images"]]
    pt, seg, truth = P.synth.make_seeds(seq, cur_frame=2)
    for i in range(1, 40, 4):
        pt["sigma2"][i], pt["mu"][i] = 1e-8, 1.0 / truth["pt_depth"][i]
    for i in range(0, 8, 2):
        seg["sigma2_s"][i] = seg["sigma2_e"][i] = 1e-8
        seg["mu_s"][i], seg["mu_e"][i] = 1.0 / truth["seg_sdepth"][i], 1.0 / truth["seg_edepth"][i]
    pt["sigma2"][2] = np.nan
    f32 = np.float32
    sd = dict(pt=[], seg=[], batch_counter=9)
    for i in range(40):
        sd["pt"].append(dict(ref_kf=0, batch_id=9 - i % 6, px=pt["px"][i].tolist(), f=pt["f"][i].tolist(), level=0, type=int(pt["type"][i]), grad=pt["grad"][i].tolist(),
                             **{k: f32(pt[k][i]) for k in ("a", "b", "mu", "z_range", "sigma2")}))
    for i in range(8):
        sd["seg"].append(dict(ref_kf=0, batch_id=9 - i % 5, px=seg["px"][i].tolist(), f=seg["f"][i].tolist(), sf=seg["sf"][i].tolist(), ef=seg["ef"][i].tolist(),
                              spx=seq["seg_spx0"][i].tolist(), epx=seq["seg_epx0"][i].tolist(), level=0,
                              **{k: f32(seg[k][i]) for k in ("a", "b", "mu_s", "mu_e", "z_range_s", "z_range_e", "sigma2_s", "sigma2_e")}))
    st = Cc.empty_stream([list(map(float, seq["poses_true"][0]))])
    st.update(pt_nfail=[], pt_nsucc=[], seg_nfail=[], seg_nsucc=[])
    # -- the host path, written out
    keep = dict(pt=[i for i, x in enumerate(sd["pt"]) if 9 - x["batch_id"] <= 3], seg=[i for i, x in enumerate(sd["seg"]) if 9 - x["batch_id"] <= 3])
    sub = lambda d, idx: {k: np.asarray(v)[idx] for k, v in d.items()}
    res = ob.update_seeds(P.abi.SeedsJob(seq["cam"], seq["poses_true"], np.arange(3), sub(pt, keep["pt"]), sub(seg, keep["seg"])), frames)
    assert (res["pt_status"] == SL.CONVERGED).sum() >= 2 and (res["seg_status"] == SL.CONVERGED).sum() >= 1 and len(keep["pt"]) < 40
    host_st, host_sd = copy.deepcopy(st), dict(pt=[], seg=[], batch_counter=9)
    new = dict(pt=[], seg=[])
    for j, i in enumerate(keep["pt"]):
        x = dict(sd["pt"][i])
        if res["pt_status"][j] == SL.CONVERGED:
            new["pt"].append(dict(pos=res["pt_xyz_world"][j].tolist(), obs=dict(kf=0, px=x["px"], f=x["f"], level=0, type=x["type"], grad=x["grad"])))
        elif res["pt_status"][j] != SL.NAN:
            x.update(a=res["pt_a"][j], b=res["pt_b"][j], mu=res["pt_mu"][j], sigma2=res["pt_sigma2"][j])
            host_sd["pt"].append(x)
    for j, i in enumerate(keep["seg"]):
        x = dict(sd["seg"][i])
        if res["seg_status"][j] == SL.CONVERGED:
            new["seg"].append(dict(spos=res["seg_xyz_world_s"][j].tolist(), epos=res["seg_xyz_world_e"][j].tolist(),
                                   obs=dict(kf=0, spx=x["spx"], epx=x["epx"], sf=x["sf"], ef=x["ef"], level=0)))
        elif res["seg_status"][j] != SL.NAN:
            x.update({k: res["seg_" + k][j] for k in SL.SEG_PARAMS})
            host_sd["seg"].append(x)
    NC.add(host_st, new)
    # -- the restatement
    at = dict(pt={id(sd["pt"][i]): j for j, i in enumerate(keep["pt"])}, seg={id(sd["seg"][i]): j for j, i in enumerate(keep["seg"])})

    def body(kind, seed):
        j = at[kind][id(seed)]
        names = SL.PT_ROWS if kind == "pt" else SL.SEG_ROWS
        return {key: (int(res[f][j]) if key == "status" else res[f][j].tolist() if key.startswith("xyz") else res[f][j]) for f, key in names}
    rep, _, _ = SL.update(sd, st, body, 3)
    assert st == host_st and repr(st) == repr(host_st)
    assert repr(SL.lists_of(sd)) == repr(SL.lists_of(host_sd))
    assert rep["pt"][SL.AGED] == 40 - len(keep["pt"]) and rep["n_pt"] == len(new["pt"]) and rep["n_seg_seeds"] == len(host_sd["seg"])
