"""Structure optimiser, path by path, on the CPU: the C oracle (oracle/plsvo_oracle.c: the generic in-place ldlt_solve_n at N = 3, and
plsvo_oracle_structure_optimize) against the restatement that records its path (tests/np_structopt.py), bit for bit, on the directed
inputs of tests/structopt_cases.py -- and a tally, from the restatement's records alone, that those inputs reach every branch they were
written for.  tests/test_gpu_structopt_paths.py then holds the device to the oracle on the same inputs.

Flavour: the device's 3x3 solve implements Eigen 3.2's zero-pivot rule (oracle flavour 320) and no other, so everything here pins 320."""
import numpy as np
import pytest

import np_structopt as ns
import structopt_cases as sc

KEYS = ("pt_iters", "seg_iters", "pt_pos", "seg_spos", "seg_epos")


@pytest.fixture(autouse=True)
def flavour320(ob):
    prev = ob.set_ldlt_flavour(320)
    yield
    ob.set_ldlt_flavour(prev)


@pytest.fixture(scope="module")
def restated():
    """the restatement's results and records of the geometry batch, per (n_iter_pts, n_iter_segs); computed once, never modified"""
    d = sc.geometry_batch()
    return {v: ns.optimize_batch(d, *v) for v in sc.ITER_VARIANTS}


@pytest.mark.parametrize("name,A,b", sc.SOLVER_SYSTEMS, ids=[s[0] for s in sc.SOLVER_SYSTEMS])
def test_oracle_solve3_equals_the_restatement(ob, name, A, b):
    x, rec = ns.solve3(A, b)
    xo = ob.ldlt_solve3(A, b)
    assert np.array_equal(xo, x, equal_nan=True), (name, xo, x, rec)
    # only the lower triangle is read
    U = np.tril(A) + np.triu(np.full((3, 3), 12345.0), 1)
    assert np.array_equal(ob.ldlt_solve3(U, b), xo, equal_nan=True) and np.array_equal(ns.solve3(U, b)[0], x, equal_nan=True)


def test_instrumented_solve_is_the_crosschecked_restatement():
    """np_structopt.solve3 is np_restatement.eigen32_ldlt_solve plus records: same bits wherever the latter does not raise"""
    import np_restatement as npr
    for name, A, b in sc.SOLVER_SYSTEMS:
        with np.errstate(all="ignore"):
            x = npr.eigen32_ldlt_solve(A, b)
        assert np.array_equal(x, ns.solve3(A, b)[0], equal_nan=True), name


@pytest.mark.parametrize("n_iter", sc.ITER_VARIANTS, ids=lambda v: "iters%d_%d" % v)
def test_oracle_optimisation_equals_the_restatement(P, ob, restated, n_iter):
    d, rn = sc.geometry_batch(), restated[n_iter]
    ro = ob.structure_optimize(P.structopt_job_from_batch(d, *n_iter))
    for i, p in enumerate(sc.POINTS):
        assert ro["pt_iters"][i] == rn["pt_iters"][i], (p["name"], rn["pt_rec"][i].exit)
        assert np.array_equal(ro["pt_pos"][i], rn["pt_pos"][i], equal_nan=True), (p["name"], ro["pt_pos"][i], rn["pt_pos"][i])
    for i, g in enumerate(sc.SEGMENTS):
        assert ro["seg_iters"][i] == rn["seg_iters"][i], (g["name"], rn["seg_rec"][i].exit)
        assert np.array_equal(ro["seg_spos"][i], rn["seg_spos"][i], equal_nan=True), (g["name"], ro["seg_spos"][i], rn["seg_spos"][i])
        assert np.array_equal(ro["seg_epos"][i], rn["seg_epos"][i], equal_nan=True), (g["name"], ro["seg_epos"][i], rn["seg_epos"][i])


def test_oracle_results_do_not_depend_on_the_batch(P, ob, restated):
    """every case alone, and the batch under a permutation of landmarks and frames, give the restatement's bits"""
    rn = restated[(5, 5)]
    for i, p in enumerate(sc.POINTS):
        r1 = ob.structure_optimize(P.structopt_job_from_batch(sc.batch([p], [])))
        assert r1["pt_iters"][0] == rn["pt_iters"][i] and np.array_equal(r1["pt_pos"][0], rn["pt_pos"][i], equal_nan=True), p["name"]
    for i, g in enumerate(sc.SEGMENTS):
        r1 = ob.structure_optimize(P.structopt_job_from_batch(sc.batch([], [g])))
        assert r1["seg_iters"][0] == rn["seg_iters"][i] and np.array_equal(r1["seg_spos"][0], rn["seg_spos"][i], equal_nan=True), g["name"]
        assert np.array_equal(r1["seg_epos"][0], rn["seg_epos"][i], equal_nan=True), g["name"]
    dp, po, so = sc.permuted(sc.POINTS, sc.SEGMENTS, 5)
    rp = ob.structure_optimize(P.structopt_job_from_batch(dp))
    assert np.array_equal(rp["pt_iters"], rn["pt_iters"][po]) and np.array_equal(rp["pt_pos"], rn["pt_pos"][po], equal_nan=True)
    assert np.array_equal(rp["seg_iters"], rn["seg_iters"][so]) and np.array_equal(rp["seg_spos"], rn["seg_spos"][so], equal_nan=True)
    assert np.array_equal(rp["seg_epos"], rn["seg_epos"][so], equal_nan=True)


def test_roll_back_restores_the_position_before_the_last_accepted_step(restated):
    """chi2 rising at iteration k undoes the step of iteration k-1 as well (reference src/feature3D_impl.cpp:71, :144-145: old_point is
    assigned before the step, not after): the result of k+1 evaluations is the result of k-1 evaluations of the same landmark"""
    i = sc.POINT_ORDER.index("rough6")
    assert restated[(5, 5)]["pt_rec"][i].exit == "chi2_rose" and restated[(5, 5)]["pt_iters"][i] == 3
    p = sc.NAMED["rough6"]
    one, it, rec = ns.point_optimize(sc.FRAMES, p["pos"], p["frames"], p["f"], 1)
    two = ns.point_optimize(sc.FRAMES, p["pos"], p["frames"], p["f"], 2)[0]
    assert it == 1 and rec.exit == "max_iter"
    assert np.array_equal(restated[(5, 5)]["pt_pos"][i], one) and not np.array_equal(one, two)
    # a segment rolls BOTH ends back when one end's chi2 rises: the healthy end loses its last step too
    k = [g["name"] for g in sc.SEGMENTS].index("rough6+pool0")
    g = sc.SEGMENTS[k]
    s1, e1, _, _ = ns.segment_optimize(sc.FRAMES, g["spos"], g["epos"], g["frames"], g["sf"], g["ef"], 1)
    s2, e2, _, _ = ns.segment_optimize(sc.FRAMES, g["spos"], g["epos"], g["frames"], g["sf"], g["ef"], 2)
    assert restated[(5, 5)]["seg_rec"][k][:2] == ("chi2_rose", "s") and restated[(5, 5)]["seg_iters"][k] == 3
    assert np.array_equal(restated[(5, 5)]["seg_epos"][k], e1) and np.array_equal(restated[(5, 5)]["seg_spos"][k], s1) and not np.array_equal(e1, e2)


def test_inputs_reach_every_path(restated):
    """From the restatement's records alone: the committed inputs reach every branch they were written for."""
    recs = {name: ns.solve3(A, b)[1] for name, A, b in sc.SOLVER_SYSTEMS}
    full = [r for n, r in recs.items() if n.startswith("order")]
    # each of the six pivot orders, on full-rank systems
    assert sorted(r.order for r in full) == [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
    assert all(r.stop_at == 3 and r.scaled == (True, True) and not any(r.zeroed) and not any(r.ties) for r in full)
    # ties: a00 == a11 at step 0, a11 == a22 at step 1, all three; the first maximum wins
    assert recs["tie01"].ties == (True, False, False) and recs["tie01"].order == (0, 1, 2)
    assert recs["tie01_negative"].ties == (True, False, False) and recs["tie02"].ties[0] and recs["tie02"].order == (0, 2, 1)
    assert recs["tie12_step1"].ties == (False, True, False) and recs["tie12_step1"].order == (0, 1, 2)
    assert recs["tie012"].ties == (True, True, False) and recs["tie012"].order == (0, 1, 2)
    for n in ("tie01_rank2", "tie12_step1_rank2", "tie012_rank1"):
        assert any(recs[n].ties) and any(recs[n].zeroed), n
    # rank 2, 1, 0
    assert sum(recs["rank2"].zeroed) == 1 and sum(recs["rank1"].zeroed) == 2 and sum(recs["zero_matrix"].zeroed) == 3
    assert recs["zero_matrix"].scaled == (False, False) and recs["zero_diagonal"].scaled == (False, False) and recs["zero_diagonal"].stop_at == 3
    # early stop at step 1 (column 0 scaled, nothing else touched), step 2 skipped, column 1 unscaled after the elimination
    for n in ("early_stop_step1", "early_stop_step1_dominant_last", "early_stop_step1_inf_a21", "early_stop_step1_nan_a21", "early_stop_step1_huge"):
        assert recs[n].stop_at == 1 and recs[n].scaled == (True, False), n
    assert recs["early_stop_step1_dominant_last"].order[0] == 2
    assert recs["skip_step2"].stop_at == 2 and recs["skip_step2_swapped"].stop_at == 2 and recs["skip_step2_swapped"].order == (0, 2, 1)
    assert recs["skip_step2"].scaled == (True, True) and recs["skip_step2_exactly_at_cutoff_runs"].stop_at == 3
    for n in ("d1_cancels", "d1_below_cutoff"):
        assert recs[n].stop_at == 3 and recs[n].scaled == (True, False) and recs[n].zeroed == (False, True, False), n
    assert recs["d1_below_cutoff"].rel_zeroed == (False, True, False)
    # a non-zero D zeroed by the relative tolerance; the tolerance floor, zeroing and keeping
    assert recs["d2_zeroed_by_relative_tolerance"].rel_zeroed == (False, False, True) and recs["d2_zeroed_by_relative_tolerance"].stop_at == 3
    assert recs["tolerance_floor"].tol_floor and not any(recs["tolerance_floor"].zeroed)
    assert recs["tolerance_floor_zeroes_subnormal_d"].tol_floor and recs["tolerance_floor_zeroes_subnormal_d"].zeroed == (False, False, True)
    assert recs["tolerance_floor_keeps_small_d"].tol_floor and not any(recs["tolerance_floor_keeps_small_d"].zeroed)
    assert not recs["overflow_products"].tol_floor and not np.all(np.isfinite(ns.solve3(*sc.SOLVER_SYSTEMS[[s[0] for s in sc.SOLVER_SYSTEMS].index("overflow_products")][1:])[0]))
    # NaN in every position, Inf on every diagonal
    # (base matrix: pivot order 0, 1, 2).  A NaN pivot is neither scaled by nor kept in D^+; a NaN off-diagonal makes the later pivots NaN
    X = {name: ns.solve3(A, b)[0] for name, A, b in sc.SOLVER_SYSTEMS}
    nan_paths = {"nan_a00": ((False, False), (True, True, True), True), "nan_a10": ((True, False), (False, True, True), False),
                 "nan_a11": ((True, False), (False, True, True), False), "nan_a20": ((True, True), (False, False, True), False),
                 "nan_a21": ((True, True), (False, False, True), False), "nan_a22": ((True, True), (False, False, True), False),
                 "nan_b0": ((True, True), (False, False, False), False), "nan_b1": ((True, True), (False, False, False), False),
                 "nan_b2": ((True, True), (False, False, False), False)}
    for n, (scaled, zeroed, floor) in nan_paths.items():
        assert recs[n].order == (0, 1, 2) and recs[n].stop_at == 3 and (recs[n].scaled, recs[n].zeroed, recs[n].tol_floor) == (scaled, zeroed, floor), (n, recs[n])
    # a NaN diagonal that D^+ zeroes leaves x finite when nothing else carries it; every other position reaches x
    assert np.isfinite(X["nan_a11"]).all() and np.isfinite(X["nan_a22"]).all()
    for n in ("nan_a00", "nan_a10", "nan_a20", "nan_a21"):
        assert np.isnan(X[n][:2]).all() and X[n][2] == 0.0, (n, X[n])
    for n in ("nan_b0", "nan_b1", "nan_b2", "nan_b0_last_pivot", "nan_b2_diagonal_matrix_order210"):
        assert np.isnan(X[n]).all(), (n, X[n])
    assert [recs[n].order[0] for n in ("inf_a00", "minus_inf_a11", "inf_a22")] == [0, 1, 2] and np.array_equal(X["inf_a22"], np.zeros(3))
    for n in ("inf_a00", "minus_inf_a11", "inf_a22"):
        assert recs[n].scaled == (False, False) and recs[n].stop_at == 1, n         # |Inf| > Inf * eps is false; everything else is below Inf * eps
    # the NaN clause of step 1's search: a NaN a11 keeps the factorisation going past a small a22; a NaN a22 does not save a small a11
    assert recs["nan_a11_small_a22"].stop_at == 2 and recs["nan_a11_small_a22_overflowing_l21"].stop_at == 2 and recs["nan_a11_zero_a22"].stop_at == 2
    assert recs["nan_a22_small_a11"].stop_at == 1 and recs["nan_a22_small_a11_overflowing_l21"].stop_at == 1
    x_go = ns.solve3(*[s for s in sc.SOLVER_SYSTEMS if s[0] == "nan_a11_small_a22_overflowing_l21"][0][1:])[0]
    x_stop = ns.solve3(*[s for s in sc.SOLVER_SYSTEMS if s[0] == "nan_a22_small_a11_overflowing_l21"][0][1:])[0]
    assert np.isnan(x_go[0]) and np.isfinite(x_stop).all()          # what going on / stopping does to x: the clause is observable

    # ---- geometry, 5 + 5 iterations ----
    r55 = restated[(5, 5)]
    pt = dict()
    for n, rec, it in zip(sc.POINT_ORDER, r55["pt_rec"], r55["pt_iters"]):
        pt.setdefault(rec.exit, []).append((n, int(it)))
    assert set(pt) == set(ns.EXITS) - {"n_iter_0"}, sorted(pt)
    assert sorted({it for _, it in pt["chi2_rose"]}) == [2, 3, 4, 5]               # chi2 rises at iteration 1, 2, 3 and 4
    assert {it for _, it in pt["nan_0"]} == {1} and {it for _, it in pt["nan_later"]} == {2}
    assert [n for n, _ in pt["no_obs"]].count("no_observations") == 2 and 0 < sc.POINT_ORDER.index("no_observations") < len(sc.POINTS) - 1
    by = dict(zip(sc.POINT_ORDER, r55["pt_rec"]))
    assert by["exact0"].exit == by["exact1"].exit == "converged_0"
    # one observation: the two lateral diagonals are equal (1/z^2) whichever world axis the depth falls on; on the optical axis the
    # third is zero and so are the off-diagonals, off the axis the matrix is full and of rank 2
    assert by["axis_z"].solves[0].order == (0, 1, 2) and by["axis_y"].solves[0].order == (0, 2, 1) and by["axis_x"].solves[0].order == (1, 2, 0)
    assert by["off_axis_z"].solves[0].order == (0, 1, 2) and by["off_axis_y"].solves[0].order == (0, 2, 1) and by["off_axis_x"].solves[0].order == (1, 2, 0)
    for n in ("axis_z", "axis_y", "axis_x"):
        assert by[n].solves[0].ties[0] and by[n].solves[0].zeroed[2], n
    for n in ("off_axis_z", "off_axis_y", "off_axis_x"):
        assert by[n].solves[0].ties[0] and by[n].solves[0].zeroed == (False, False, True) and by[n].solves[0].scaled == (True, True), n
    # depth 1e-9 of the lateral offset: the depth column dominates and the factorisation stops at step 1
    assert by["shallow"].solves[0].stop_at == 1 and by["shallow"].solves[0].order[0] == 2 and by["shallow_y"].solves[0].stop_at == 1 and by["shallow_y"].solves[0].order[0] == 1
    assert by["shallow_two_views"].solves[0].stop_at == 1
    assert by["zero_depth"].exit == by["zero_depth_on_axis"].exit == by["bearing_f2_zero"].exit == by["bearing_f2_zero_inf_inf"].exit == "nan_0"
    assert all(s.tol_floor for s in by["far_1e150"].solves) and all(s.tol_floor for s in by["far_1e150_one_view"].solves)
    assert by["step_to_infinity"].exit == "nan_later" and not by["step_to_infinity"].nan_written
    # an accepted step whose dp[0] is not NaN while another component is: the reference tests dp[0] alone and writes the NaN (here the
    # following iteration rolls it back; with one iteration it is the result)
    assert by["wild9"].nan_written and by["wild22"].nan_written and by["wild9"].exit == "nan_later"
    i9 = sc.POINT_ORDER.index("wild9")
    assert np.isnan(restated[(1, 1)]["pt_pos"][i9]).any() and not np.isnan(restated[(1, 1)]["pt_pos"][i9]).all()
    assert np.isfinite(r55["pt_pos"][i9]).all()
    assert not by["wild9"].nan_written_finite and not by["wild22"].nan_written_finite       # full rank: dp[0] = +-Inf there
    # ... and beside a FINITE dp[0], where D^+ turns the NaN components it zeroes into 0: b all NaN (a bearing with f[2] == 0, or holding a
    # NaN), A finite, the depth column pivoted first and the factorisation stopped at step 1 -- dp is NaN on the depth axis alone.  With
    # the depth on world z or y, dp[0] = 0: the step is accepted, norm_max passes over the NaN, and the landmark is reported at rest at
    # iteration 0 with a NaN written into it -- at every iteration limit.  With the depth on world x the same input is rolled back.
    for n, axis in (("shallow_f2_zero", 2), ("shallow_nan_bearing", 2), ("shallow_y_f2_zero", 1)):
        i, rec = sc.POINT_ORDER.index(n), by[n]
        assert rec.exit == "converged_0" and rec.nan_written and rec.nan_written_finite and len(rec.solves) == 1, (n, rec)
        assert rec.solves[0].stop_at == 1 and rec.solves[0].order[0] == axis and rec.solves[0].zeroed == (False, True, True), (n, rec)
        for v in ((5, 5), (2, 3), (1, 1)):
            pos = restated[v]["pt_pos"][i]
            assert restated[v]["pt_iters"][i] == 1 and np.isnan(pos[axis]) and np.array_equal(np.delete(pos, axis), np.delete(sc.NAMED[n]["pos"], axis)), (n, v, pos)
    ix = sc.POINT_ORDER.index("shallow_x_f2_zero")
    assert by["shallow_x_f2_zero"].exit == "nan_0" and by["shallow_x_f2_zero"].solves[0].order[0] == 0 and np.array_equal(r55["pt_pos"][ix], sc.NAMED["shallow_x_f2_zero"]["pos"])
    assert sorted(n for n, r in by.items() if r.nan_written_finite) == ["shallow_f2_zero", "shallow_nan_bearing", "shallow_y_f2_zero"]
    # the iteration limits: out of iterations at 1, 2, 3 and 5; zero iterations on either side
    assert any(r.exit == "max_iter" for r in restated[(2, 3)]["pt_rec"]) and any(r.exit == "max_iter" for r in restated[(2, 3)]["seg_rec"])
    assert all(r.exit == "n_iter_0" for r in restated[(0, 5)]["pt_rec"]) and all(r.exit == "n_iter_0" for r in restated[(5, 0)]["seg_rec"])
    assert not any(r.exit == "n_iter_0" for r in restated[(0, 5)]["seg_rec"] + restated[(5, 0)]["pt_rec"])

    # ---- segments: every exit, and every trigger on the start point only, the end point only and both ----
    sg = {}
    for g, rec, it in zip(sc.SEGMENTS, r55["seg_rec"], r55["seg_iters"]):
        sg.setdefault((rec.exit, rec.ends), []).append((g["name"], int(it)))
    for ex in ("converged_0", "converged_later", "chi2_rose", "nan_0", "nan_later"):
        for ends in ("s", "e", "both"):
            assert (ex, ends) in sg, (ex, ends)
    assert ("max_iter", "") in sg and ("no_obs", "both") in sg
    # one end at rest while the other still moves: the other end, alone, would have gone on
    for n in ("pool37+pool0", "pool0+pool37"):
        k = [g["name"] for g in sc.SEGMENTS].index(n)
        assert r55["seg_rec"][k][:2] in (("converged_later", "s"), ("converged_later", "e")) and r55["seg_iters"][k] == 4
    assert r55["pt_iters"][sc.POINT_ORDER.index("pool0")] == 5 and r55["pt_iters"][sc.POINT_ORDER.index("pool37")] == 4
    for ends in ("s", "e", "both"):
        assert sorted({it for _, it in sg[("chi2_rose", ends)]}) == [2, 3, 5], ends
    assert sorted(g["name"] for g, r in zip(sc.SEGMENTS, r55["seg_rec"]) if r.nan_written and not r.nan_written_finite) == ["pool2+wild22", "wild7+wild9", "wild9+pool2"]
    # a segment end at rest at iteration 0 with a NaN written into it: the start point only (the other end has moved one step), the end
    # point only, and both
    names = [g["name"] for g in sc.SEGMENTS]
    for n, ends, nan_s, nan_e in (("shallow_f2_zero+off_axis_z", "s", True, False), ("off_axis_z+shallow_f2_zero", "e", False, True),
                                  ("shallow_f2_zero+shallow_nan_bearing", "both", True, True), ("shallow_y_f2_zero+axis_y", "s", True, False)):
        k = names.index(n)
        rec = r55["seg_rec"][k]
        assert (rec.exit, rec.ends, rec.nan_written_finite) == ("converged_0", ends, True) and r55["seg_iters"][k] == 1, (n, rec)
        assert np.isnan(r55["seg_spos"][k]).any() == nan_s and np.isnan(r55["seg_epos"][k]).any() == nan_e, n
        moved = r55["seg_epos"][k] if nan_s and not nan_e else r55["seg_spos"][k] if nan_e and not nan_s else None
        start = sc.SEGMENTS[k]["epos"] if nan_s and not nan_e else sc.SEGMENTS[k]["spos"]
        assert moved is None or (np.isfinite(moved).all() and not np.array_equal(moved, start)), n
    assert sorted(g["name"] for g, r in zip(sc.SEGMENTS, r55["seg_rec"]) if r.nan_written_finite) == sorted(
        ["shallow_f2_zero+off_axis_z", "off_axis_z+shallow_f2_zero", "shallow_f2_zero+shallow_nan_bearing", "shallow_y_f2_zero+axis_y"])


def test_layouts_have_the_sizes_they_claim():
    assert sc.LAYOUT_SIZES == [(a, b) for a in (1, 63, 64, 65) for b in (0, 1, 64, 65)]
    for n_pts, n_seg in sc.LAYOUT_SIZES:
        d = sc.layout(n_pts, n_seg)
        assert d["pt_pos"].shape == (n_pts, 3) and d["seg_spos"].shape == (n_seg, 3) and len(d["pt_obs_off"]) == n_pts + 1 and len(d["seg_obs_off"]) == n_seg + 1
        assert np.all(np.diff(d["pt_obs_off"]) >= 0) and np.all(np.diff(d["seg_obs_off"]) >= 0) and d["pt_obs_off"][-1] == len(d["pt_obs_frame"])
