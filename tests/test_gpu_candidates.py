"""The map-candidate stage on the device (plsvo_candidates_*; pl-svo_amd/csrc/candidates_device.hpp) against its restatement
tests/np_candidates.py on the cases of tests/candidates_cases.py.  Everything is compared bit for bit: the stage has no transcendental
call, sqrt and division are IEEE on both sides."""
import ctypes as C

import numpy as np
import pytest

import candidates_cases as Cc

PT_FIELDS = ("pt_lm", "pt_px", "pt_cell", "pt_obs", "pt_has_view", "pt_active")
SEG_FIELDS = ("seg_lm", "seg_px", "seg_cell", "seg_obs", "seg_has_view", "seg_active")
OTHER_FIELDS = ("kf_count", "pt_cand_failed", "seg_cand_failed")


def run_case(ctx, case, Ts=None, poses_dev=None, **params):
    ctx.candidates_stage([Cc.to_job(st) for st in case["streams"]], Cc.CAM, Cc.CELL, Cc.SEG_CELL, Cc.BOUNDARY, **params)
    return rerun(ctx, case, Ts, poses_dev)


def rerun(ctx, case, Ts=None, poses_dev=None):
    frames = Cc.frames_of(case if Ts is None else dict(case, T=Ts))
    ctx.candidates_run(frames, poses_dev=poses_dev)
    return ctx.candidates_fetch()


def same(a, b):
    return set(a) == set(b) and all(np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes() and np.asarray(a[f]).shape == np.asarray(b[f]).shape for f in a)


def check_against_restatement(got, want, tag):
    assert (got["n_filed_pt"], got["n_filed_seg"]) == (want["n_filed_pt"], want["n_filed_seg"]), tag
    for f in PT_FIELDS + SEG_FIELDS + OTHER_FIELDS:
        g = got[f]
        w = np.asarray(want[f], dtype=g.dtype).reshape(g.shape if g.size else (-1,) + g.shape[1:])
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), (tag, f, g, w)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(Cc.ALL))
def test_candidates_equal_the_restatement(gpu_ctx, name):
    case = Cc.ALL[name]()
    res = run_case(gpu_ctx, case)
    for k, (r, w) in enumerate(zip(res, Cc.restate(case))):
        check_against_restatement(r, w, (name, k))


@pytest.mark.gpu
def test_one_stream_at_a_time_equals_its_place_in_the_batch(gpu_ctx):
    case = Cc.edge_batch_case()
    res = run_case(gpu_ctx, case)
    for k in (0, 3, 5, 8):
        one = run_case(gpu_ctx, dict(streams=case["streams"][k:k + 1], T=case["T"][k:k + 1], overlap=case["overlap"][k:k + 1]))[0]
        assert same(one, res[k]), k


@pytest.mark.gpu
def test_a_second_run_on_the_staged_tables_does_not_see_the_first(gpu_ctx):
    """two runs on the same staged tables with different poses and overlap lists, then the first again: the first result comes back
    (the first-visit words are re-armed ahead of every launch)"""
    case = Cc.sizes_case()
    first = run_case(gpu_ctx, case)
    rng = np.random.default_rng(8)
    other = dict(case, T=tuple(Cc.rand_pose(rng, 0.2, 0.5) for _ in case["T"]), overlap=tuple(tuple(reversed(o)) for o in case["overlap"]))
    second = rerun(gpu_ctx, other)
    for k, (r, w) in enumerate(zip(second, Cc.restate(other))):
        check_against_restatement(r, w, ("second", k))
    assert any(not same(a, b) for a, b in zip(first, second))
    again = rerun(gpu_ctx, case)
    assert all(same(a, b) for a, b in zip(first, again))


@pytest.mark.gpu
def test_the_device_pose_path_equals_the_host_pose_path(gpu_ctx):
    """d_T_f_w: the poses are read from the device (here: where the run before left them, the new frames' entries of the matcher's
    frame table), T_f_w is not looked at"""
    case = Cc.edge_batch_case()
    host = run_case(gpu_ctx, case)
    dev = gpu_ctx.candidates_dev()
    n = len(case["streams"])
    ptrs = [int(dev.d_frame_T) + 56 * (int(dev.f_off[k]) + len(case["streams"][k]["kf_T"])) for k in range(n)]
    wrong = tuple(Cc.IDENT if k != 5 else Cc.rand_pose(np.random.default_rng(1)) for k in range(n))
    from_dev = rerun(gpu_ctx, case, Ts=wrong, poses_dev=ptrs)
    assert all(same(a, b) for a, b in zip(host, from_dev))
    plain = rerun(gpu_ctx, case, Ts=wrong)
    assert any(not same(a, b) for a, b in zip(host, plain))


@pytest.mark.gpu
def test_px_and_cell_are_those_of_plsvo_reproject(gpu_ctx, P):
    case = Cc.edge_batch_case()
    res = run_case(gpu_ctx, case)
    n_checked = 0
    for st, T, r in zip(case["streams"], case["T"], res):
        if r["n_filed_pt"]:
            pr = gpu_ctx.reproject(P.abi.ReprojectJob(Cc.CAM, [T], np.zeros(r["n_filed_pt"], np.int32), np.array(st["pt_pos"])[r["pt_lm"]], Cc.CELL, Cc.BOUNDARY))
            assert pr["px"].tobytes() == r["pt_px"].tobytes() and np.array_equal(pr["cell"], r["pt_cell"])
        if r["n_filed_seg"]:
            pos = np.stack([np.array(st["seg_spos"])[r["seg_lm"]], np.array(st["seg_epos"])[r["seg_lm"]]], 1).reshape(-1, 3)
            pr = gpu_ctx.reproject(P.abi.ReprojectJob(Cc.CAM, [T], np.zeros(len(pos), np.int32), pos, Cc.SEG_CELL, Cc.BOUNDARY))
            assert pr["px"].tobytes() == r["seg_px"].tobytes() and np.array_equal(pr["cell"], r["seg_cell"].reshape(-1))
        n_checked += r["n_filed_pt"] + r["n_filed_seg"]
    assert n_checked > 100


def _texture(rng, w=320, h=240):
    coarse = rng.integers(0, 256, (h // 8 + 2, w // 8 + 2)).astype(np.float64)
    img = np.kron(coarse, np.ones((8, 8)))[:h + 8, :w + 8]
    k = np.ones(7) / 7.0
    img = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 1, img)
    img = np.apply_along_axis(lambda c: np.convolve(c, k, mode="same"), 0, img)
    return np.clip(img[4:h + 4, 4:w + 4], 0, 255).astype(np.uint8)


@pytest.mark.gpu
def test_the_resident_match_equals_plsvo_match_direct_on_the_fetched_candidates(P):
    """plsvo_candidates_match runs the matcher's kernel on the arrays the stage wrote on the device; plsvo_match_direct with host arrays
    built from the FETCHED candidates and the tables gives the same found / px / search_level, byte for byte.  Candidates with
    active == 0 are not matched: found 0, the projection, level -1."""
    case = Cc.edge_batch_case()
    ctx = P.capi.Context(0)
    try:
        n_slots = max(len(st["kf_T"]) for st in case["streams"]) + 1
        ctx.config_pyramids(n_slots, 320, 240, 3)
        rng = np.random.default_rng(31)
        for s in range(n_slots):
            ctx.build_pyramid(s, _texture(rng))
        res = run_case(ctx, case, n_pyr_levels=3, align_max_iter=10)
        ctx.candidates_match()
        got = ctx.candidates_match_fetch([(r["n_filed_pt"], r["n_filed_seg"]) for r in res])
        n_active = n_found = 0
        for k, (st, T, r, g) in enumerate(zip(case["streams"], case["T"], res, got)):
            n_kf = len(st["kf_T"])
            rows = []                                        # (active, ref observation as plsvo_match_in wants it, pos, px_cur)
            for i in range(r["n_filed_pt"]):
                lm, o = int(r["pt_lm"][i]), int(r["pt_obs"][i])
                ob = st["pt_obs"][lm][o] if o >= 0 else None
                rows.append((r["pt_active"][i], ob and (ob["kf"], ob["px"], ob["f"], ob["level"], ob["type"], ob["grad"]), st["pt_pos"][lm], r["pt_px"][i]))
            for e, (pk, fk, posk) in enumerate((("spx", "sf", "seg_spos"), ("epx", "ef", "seg_epos"))):
                for i in range(r["n_filed_seg"]):
                    lm, o = int(r["seg_lm"][i]), int(r["seg_obs"][i])
                    ob = st["seg_obs"][lm][o] if o >= 0 else None
                    rows.append((r["seg_active"][i], ob and (ob["kf"], ob[pk], ob[fk], ob["level"], 0, (0.0, 0.0)), st[posk][lm], r["seg_px"][i, 2 * e:2 * e + 2]))
            assert len(rows) == len(g["found"])
            act = [i for i, row in enumerate(rows) if row[0]]
            for i, row in enumerate(rows):
                if not row[0]:
                    assert g["found"][i] == 0 and g["search_level"][i] == -1 and g["px"][i].tobytes() == np.asarray(row[3], float).tobytes(), (k, i)
            if not act:
                continue
            job = P.abi.MatchJob(Cc.CAM, list(st["kf_T"]) + [T], list(st["kf_slot"]) + [n_kf], [n_kf] * len(act), [rows[i][1][0] for i in act],
                                 [rows[i][1][1] for i in act], [rows[i][1][2] for i in act], [rows[i][1][3] for i in act], [rows[i][1][4] for i in act],
                                 [rows[i][1][5] for i in act], [rows[i][2] for i in act], [rows[i][3] for i in act], n_pyr_levels=3, align_max_iter=10)
            want = ctx.match_direct(job)
            assert g["found"][act].tobytes() == want["found"].tobytes(), k
            assert g["px"][act].tobytes() == want["px_cur"].tobytes(), k
            assert g["search_level"][act].tobytes() == want["search_level"].tobytes(), k
            n_active += len(act); n_found += int(want["found"].sum())
        assert n_active > 100 and n_found > 0, (n_active, n_found)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_candidates_error_paths(gpu_ctx, P):
    L, h, A = gpu_ctx.L, gpu_ctx.h, P.abi
    inv = A.E_INVALID
    case = Cc.edge_case()
    before = run_case(gpu_ctx, case)[0]
    good = Cc.to_job(case["streams"][0])
    pr = A.CandParams()
    pr.cam, pr.cell_size, pr.seg_cell_size, pr.boundary, pr.n_pyr_levels, pr.align_max_iter = Cc.CAM, Cc.CELL, Cc.SEG_CELL, Cc.BOUNDARY, 3, 10
    assert L.plsvo_candidates_stage(h, -1, None, C.byref(pr)) == inv and L.plsvo_candidates_stage(h, 1, None, C.byref(pr)) == inv
    assert L.plsvo_candidates_stage(h, 1, C.byref(good.c), None) == inv
    # negative counts, NULL arrays with non-zero counts
    for field in ("n_kf", "n_pt", "n_seg", "n_pt_cand", "n_seg_cand"):
        m = A.CandMap.from_buffer_copy(good.c)
        setattr(m, field, -1)
        assert L.plsvo_candidates_stage(h, 1, C.byref(m), C.byref(pr)) == inv, field
    for field in A._CAND_MAP_ORDER:
        if field == "pt_obs_grad":                         # may be NULL without edgelets
            continue
        m = A.CandMap.from_buffer_copy(good.c)
        setattr(m, field, None)
        assert L.plsvo_candidates_stage(h, 1, C.byref(m), C.byref(pr)) == inv, field
    # an index out of range in any table, a type outside the enums, offsets that decrease
    for field, value in (("kf_pt_lm", good.n_pt), ("kf_pt_lm", -2), ("kf_seg_lm", good.n_seg), ("pt_obs_kf", good.n_kf), ("pt_obs_kf", -1), ("seg_obs_kf", good.n_kf),
                         ("pt_cand", good.n_pt), ("pt_cand", -1), ("seg_cand", good.n_seg), ("pt_type", 4), ("seg_type", -1), ("pt_obs_level", -1),
                         ("seg_obs_level", 8), ("kf_slot", -1), ("kf_pt_off", 10 ** 6), ("pt_obs_off", 10 ** 6), ("kf_seg_off", -1), ("seg_obs_off", -1)):
        bad = good.t[field].copy()
        bad[1 if field.endswith("_off") else 0] = value
        m = A.CandMap.from_buffer_copy(good.c)
        setattr(m, field, bad.ctypes.data_as(A.c_i32_p))
        assert L.plsvo_candidates_stage(h, 1, C.byref(m), C.byref(pr)) == inv, (field, value)
    bad = good.t["pt_obs_type"].copy(); bad[0] = 2
    m = A.CandMap.from_buffer_copy(good.c)
    m.pt_obs_type = bad.ctypes.data_as(A.c_u8_p)
    assert L.plsvo_candidates_stage(h, 1, C.byref(m), C.byref(pr)) == inv
    for field in ("cell_size", "seg_cell_size"):
        p2 = A.CandParams.from_buffer_copy(pr)
        setattr(p2, field, 0)
        assert L.plsvo_candidates_stage(h, 1, C.byref(good.c), C.byref(p2)) == inv, field
    # the frames: another n than staged, a NULL list, an overlap index outside the table, negative counts
    fr = Cc.frames_of(case)[0]
    assert L.plsvo_candidates_run(h, 2, C.byref(fr.c)) == inv and L.plsvo_candidates_run(h, 1, None) == inv
    for field, value in (("n_overlap", -1), ("overlap_idx", None), ("cur_slot", -1)):
        f2 = A.CandFrame.from_buffer_copy(fr.c)
        setattr(f2, field, value)
        assert L.plsvo_candidates_run(h, 1, C.byref(f2)) == inv, field
    for value in (-1, good.n_kf):
        bad = fr.overlap_idx.copy(); bad[-1] = value
        f2 = A.CandFrame.from_buffer_copy(fr.c)
        f2.overlap_idx = bad.ctypes.data_as(A.c_i32_p)
        assert L.plsvo_candidates_run(h, 1, C.byref(f2)) == inv, value
    out = A.CandOut()
    assert L.plsvo_candidates_fetch(h, 2, C.byref(out)) == inv and L.plsvo_candidates_fetch(h, 1, None) == inv
    # nothing was written: the staged tables and the last run's results are still there
    assert same(gpu_ctx.candidates_fetch()[0], before)
    assert same(rerun(gpu_ctx, case)[0], before)
    # the matcher needs pyramids of the camera's size
    fresh = P.capi.Context(0)
    try:
        assert fresh.L.plsvo_candidates_run(fresh.h, 1, C.byref(fr.c)) == A.E_STATE
        run_case(fresh, case)
        assert fresh.L.plsvo_candidates_match_fetch(fresh.h, 1, C.byref(A.CandMatchOut())) == A.E_STATE
        assert fresh.L.plsvo_candidates_match(fresh.h) == A.E_STATE
        fresh.config_pyramids(3, 320, 240, 3)                # fewer slots than the keyframes use
        assert fresh.L.plsvo_candidates_match(fresh.h) == A.E_CAPACITY
    finally:
        fresh.close()


@pytest.mark.gpu
def test_candidates_full_size_replicas(gpu_ctx):
    """1024 streams: 16 distinct tables x 64 replicas, 10 overlap keyframes of 200 + 80 features.  Every replica equals the first
    sixteen, and those equal the restatement"""
    base = Cc.full_size_tables()
    reps = 64
    case = dict(streams=base["streams"] * reps, T=base["T"] * reps, overlap=base["overlap"] * reps)
    jobs = [Cc.to_job(st) for st in base["streams"]]
    gpu_ctx.candidates_stage(jobs * reps, Cc.CAM, Cc.CELL, Cc.SEG_CELL, Cc.BOUNDARY)
    res = rerun(gpu_ctx, case)
    for k, (r, w) in enumerate(zip(res[:16], Cc.restate(base))):
        check_against_restatement(r, w, ("full_size", k))
        assert r["n_filed_pt"] > 100 and r["n_filed_seg"] > 30
    for k in range(16, 16 * reps):
        assert same(res[k], res[k % 16]), k
