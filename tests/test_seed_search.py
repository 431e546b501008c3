"""The depth filter's epipolar search on directed inputs, CPU side: the oracle (oracle/plsvo_oracle.c: plsvo_update_seeds, what the HIP
kernel is held to bit for bit in tests/test_gpu_seed_search.py) against the NumPy restatement of tests/np_seeds.py, written from the
reference source, on every seed of every case of tests/seed_search_cases.py -- point seeds AND line seeds, every reference level,
n_pyr_levels 3 and 4, other step / iteration limits, the edgelet filter off -- and the CONDITIONS on those inputs: which exits of the
search, which (reference level, search level) pairs, which byte phases of the scored patch rows, ties, border crossings and statuses
they must keep reaching, from the restatement's path records."""
import collections

import numpy as np
import pytest

import np_seeds as ns
import seed_search_cases as sc
from test_depth_filter import _assert_close

RUNS = [(k, {}) for k in range(sc.N_CASES)] + sc.VARIANTS
POSTERIOR_SEG = ("seg_a", "seg_b", "seg_mu_s", "seg_mu_e", "seg_sigma2_s", "seg_sigma2_e")
SEG_TIGHT = sorted(sc.SEG_ROWS["tight"] + (sc.SEG_ROWS["one_tight"],))


def oracle_of(P, ob, k, over):
    c = sc.case(P, ob, k)
    return c["oracle"] if not over else ob.update_seeds(sc.job_of(P, c, **over), c["frames"])


def assert_close_with_tight_rows(P, rd, ro, seg_tight=SEG_TIGHT):
    """For the DEVICE against the oracle (tests/test_gpu_seed_search.py) only.  test_depth_filter._assert_close (statuses and depths equal, the posterior to its documented tolerances) on every row, except that the
    posterior of the line seeds planted TIGHT (sigma2 = 1e-8) follows the rule tests/test_depth_filter.py::test_hip_update_seeds_edge_cases
    documents for such seeds: their variance is a difference of floats that agree to seven digits, rounding noise on both sides, so it is
    only asked to be either within the usual tolerance or below 1e-6 on both sides; mu and a converged landmark agree to 1e-5"""
    rows = [r for r in seg_tight if r < len(ro["seg_status"])]
    masked = dict(rd)
    for k in POSTERIOR_SEG:
        masked[k] = rd[k].copy()
        masked[k][rows] = ro[k][rows]
    _assert_close(masked, ro)
    for r in rows:
        for k in ("seg_a", "seg_b"):
            assert np.allclose(rd[k][r], ro[k][r], rtol=2e-3, atol=0, equal_nan=True), (k, r, rd[k][r], ro[k][r])
        for k in ("seg_mu_s", "seg_mu_e", "seg_xyz_world_s", "seg_xyz_world_e"):
            assert np.allclose(rd[k][r], ro[k][r], rtol=1e-5, atol=1e-9, equal_nan=True), (k, r, rd[k][r], ro[k][r])
        for k in ("seg_sigma2_s", "seg_sigma2_e"):
            a, b = float(rd[k][r]), float(ro[k][r])
            assert (a < 1e-6 and b < 1e-6) or np.isclose(a, b, rtol=2e-4, atol=0, equal_nan=True), (k, r, a, b)
    conv = ro["seg_status"] == P.abi.SEED_CONVERGED
    assert np.allclose(rd["seg_xyz_world_s"][conv], ro["seg_xyz_world_s"][conv], rtol=1e-5, atol=1e-9)
    assert np.allclose(rd["seg_xyz_world_e"][conv], ro["seg_xyz_world_e"][conv], rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("run", range(len(RUNS)))
def test_oracle_matches_the_numpy_restatement_on_every_seed(P, ob, run):
    """Every point and line seed of the run: the same status (so also the same status class as
    test_depth_filter.py::test_oracle_point_seed_search_matches_numpy_restatement defines it), a search that ends in *_ok exactly where the
    oracle's status is at least UPDATED, a second end-point search exactly where the first succeeded, triangulated depths within 2e-3, the
    position in the current frame within 1e-9 px (measured: 6e-14), the posterior of points and lines within _assert_close's tolerances
    and the landmarks of converged seeds within its 1e-6.
    Matched searches whose depth agrees to 1e-9: all but at most one per run.  Measured: all, in all 24 runs (largest difference
    3.0e-10 -- in the pure-rotation case, where the triangulation is next to singular).  Why one may miss: the restatement's warp
    matrix comes from NumPy's own, differently ordered double products (tests/test_match_warp.py: 1e-12), so a byte of the warped
    patch, and with it the argmin or the alignment, may fall the other way once; the precedent in test_depth_filter.py asks half."""
    k, over = RUNS[run]
    c = sc.case(P, ob, k)
    o = oracle_of(P, ob, k, over)
    r, pt_rec, seg_rec = sc.restated(P, ob, k, **over)
    assert np.array_equal(r["pt_status"], o["pt_status"]), np.flatnonzero(r["pt_status"] != o["pt_status"])
    assert np.array_equal(r["seg_status"], o["seg_status"]), np.flatnonzero(r["seg_status"] != o["seg_status"])
    pairs = []            # (restated depth, oracle depth) of every search that the restatement matched
    for i, rec in enumerate(pt_rec):
        assert rec["exit"] in ns.EXITS
        assert rec["exit"].endswith("_ok") == (o["pt_status"][i] >= 2), (i, rec["exit"], o["pt_status"][i])
        assert (rec["exit"] == "invisible") == (o["pt_status"][i] == 0), (i, rec["exit"])
        if rec["exit"].endswith("_ok"):
            pairs.append((r["pt_depth"][i], o["pt_depth"][i]))
        else:
            assert o["pt_depth"][i] == 0.0, i                   # no depth without a match
    for i, (rs, re) in enumerate(seg_rec):
        both = rs["exit"].endswith("_ok") and re is not None and re["exit"].endswith("_ok")
        assert both == (o["seg_status"][i] >= 2), (i, rs["exit"], re and re["exit"], o["seg_status"][i])
        assert (re is not None) == rs["exit"].endswith("_ok")
        if rs["exit"].endswith("_ok"):
            pairs.append((r["seg_depth_s"][i], o["seg_depth_s"][i]))
        if re is None:
            assert o["seg_depth_e"][i] == 0.0, i               # the second search did not run
        elif re["exit"].endswith("_ok"):
            pairs.append((r["seg_depth_e"][i], o["seg_depth_e"][i]))
    if pairs:
        z, zo = np.array(pairs).T
        rel = np.abs(z - zo) / z
        print(f"run {run}: {len(pairs)} matched searches, {(rel <= 1e-9).sum()} within 1e-9, max {rel.max():.3g}")
        assert rel.max() <= 2e-3, (run, rel.max())
        assert (rel <= 1e-9).sum() >= len(pairs) - 1, (run, (rel <= 1e-9).sum(), len(pairs))
    # the matched position (and, without a match, the position the search stopped at): 1e-9 px
    assert np.allclose(r["pt_px_cur"], o["pt_px_cur"], rtol=0, atol=1e-9), np.abs(r["pt_px_cur"] - o["pt_px_cur"]).max()
    # the posterior, tight line seeds included: _assert_close's tolerances unchanged, with the fields it wants bit for bit taken from the oracle
    r = dict(r, **{f: o[f] for f in ("pt_depth", "pt_px_cur", "seg_depth_s", "seg_depth_e")})
    _assert_close(r, o)
    conv = o["seg_status"] == P.abi.SEED_CONVERGED
    for f in ("seg_xyz_world_s", "seg_xyz_world_e"):
        assert np.allclose(r[f], o[f], rtol=1e-6, atol=1e-9) and o[f][conv].any(axis=1).all(), f
    assert c["frames"][0][0].shape == (sc.H, sc.W)


def test_planted_seeds_do_what_they_were_planted_for(P, ob):
    """the rows of seed_search_cases.PT_ROWS / SEG_ROWS, on the oracle's statuses and the restatement's records"""
    A, R, S = P.abi, sc.PT_ROWS, sc.SEG_ROWS
    n = collections.Counter()
    for k in range(sc.N_CASES):
        c = sc.case(P, ob, k)
        o = c["oracle"]
        r, pt_rec, seg_rec = sc.restated(P, ob, k)
        zoom, kind = sc.CASES[k][2], sc.CASES[k][5]
        if zoom > -1.2:                                         # (a camera that backs away far enough sees them again)
            assert o["pt_status"][R["behind"]] == A.SEED_NOT_VISIBLE and o["pt_status"][R["outside"]] == A.SEED_NOT_VISIBLE, k
            for row in (R["behind"], R["outside"]):
                assert o["pt_mu"][row] == np.float32(c["pt"]["mu"][row]) and o["pt_b"][row] == 10.0
        n["pt_converged"] += o["pt_status"][R["tight"]] == A.SEED_CONVERGED
        if o["pt_status"][R["tight"]] == A.SEED_CONVERGED:
            X = P.synth.se3_act(P.synth.se3_inv(c["frame_T"][0]), c["pt"]["f"][R["tight"]] * c["truth"]["pt_depth"][R["tight"]])
            assert np.linalg.norm(o["pt_xyz_world"][R["tight"]] - X) < 0.05 * c["truth"]["pt_depth"][R["tight"]], k
        assert o["pt_status"][R["nan"]] in (A.SEED_NOT_VISIBLE, A.SEED_NO_MATCH, A.SEED_NAN), k
        if o["pt_status"][R["nan"]] != A.SEED_NOT_VISIBLE:
            assert pt_rec[R["nan"]]["exit"] == "epi_nonfinite" and o["pt_b"][R["nan"]] == 11.0, k
        if pt_rec[R["far"]]["exit"] != "invisible":
            assert pt_rec[R["far"]]["exit"].startswith("short_"), (k, pt_rec[R["far"]]["exit"])
            n["far_short"] += 1
        if kind in ("walk", "tie") and zoom == 0.0:
            for row in R["cross"]:
                n["cross"] += pt_rec[row]["n_out_of_frame_skipped"] > 0 and pt_rec[row]["n_scored"] > 0
            for row in R["all_out"]:
                n["all_out"] += pt_rec[row]["exit"] == "no_score_below_threshold" and pt_rec[row]["n_scored"] == 0
            for row in S["all_out"]:
                n["seg_all_out"] += seg_rec[row][0]["exit"] == "no_score_below_threshold" and seg_rec[row][0]["n_scored"] == 0
        if kind == "rotation":
            ex = collections.Counter(rec["exit"] for rec in pt_rec)
            assert set(ex) <= {"invisible", "epi_nonfinite", "edgelet_reject", "short_ok", "short_align_fail", "short_tri_fail"} and ex["short_tri_fail"] >= 20, ex
        # line seeds
        rs, re = seg_rec[S["nan_s"]]
        if rs["exit"] != "invisible":
            assert rs["exit"] == "nan_bounds" and re is None and o["seg_status"][S["nan_s"]] == A.SEED_NO_MATCH and o["seg_b"][S["nan_s"]] == 11.0, k
            n["seg_nan_s"] += 1
        rs, re = seg_rec[S["nan_e"]]
        if rs["exit"].endswith("_ok"):
            assert re["exit"] == "nan_bounds" and o["seg_status"][S["nan_e"]] == A.SEED_NO_MATCH and o["seg_b"][S["nan_e"]] == 11.0, k
            assert o["seg_depth_s"][S["nan_e"]] > 0 and o["seg_mu_s"][S["nan_e"]] == np.float32(c["seg"]["mu_s"][S["nan_e"]])
            n["seg_nan_e"] += 1
        for row in S["tight"]:
            if o["seg_status"][row] == A.SEED_CONVERGED:
                n["seg_converged"] += 1
                assert o["seg_xyz_world_s"][row].any() and o["seg_xyz_world_e"][row].any()
        assert o["seg_status"][S["one_tight"]] != A.SEED_CONVERGED, k
        n["seg_one_tight_updated"] += o["seg_status"][S["one_tight"]] == A.SEED_UPDATED
        assert not o["seg_xyz_world_s"][o["seg_status"] != A.SEED_CONVERGED].any()
    print(dict(n))
    # (in brackets: what the cases gave when they were written)
    assert n["pt_converged"] >= 10, n             # (13)
    assert n["far_short"] >= 10, n                # (18)
    assert n["cross"] >= 12 and n["all_out"] >= 12 and n["seg_all_out"] >= 4, n      # (16, 15, 7: four cases without a zoom)
    assert n["seg_nan_s"] >= 8 and n["seg_nan_e"] >= 8, n                            # (16, 14)
    assert n["seg_converged"] >= 10 and n["seg_one_tight_updated"] >= 8, n           # (31, 15)


def test_other_settings_do_what_they_say(P, ob):
    """max_epi_search_steps = 5: every search of more than 5 steps ends in too_many_steps and no other one does; the edgelet filter off:
    nothing is rejected, and the edgelets that were are now searched; align_max_iter = 3: fewer alignments converge"""
    for k, over in sc.VARIANTS:
        _, rec0, _ = sc.restated(P, ob, k)
        _, rec1, seg1 = sc.restated(P, ob, k, **over)
        o0, o1 = sc.case(P, ob, k)["oracle"], oracle_of(P, ob, k, over)
        ex0, ex1 = (collections.Counter(r["exit"] for r in rr) for rr in (rec0, rec1))
        if "max_epi_search_steps" in over:
            allr = rec1 + [r for rr in seg1 for r in rr if r]
            assert all((r["exit"] == "too_many_steps") == (r["n_steps"] > 5) for r in allr)
            assert ex1["too_many_steps"] >= 20 and ex1["walk_ok"] + ex1["walk_align_fail"] + ex1["no_score_below_threshold"] < ex0["walk_ok"], (k, ex1)
        elif "edgelet_filtering" in over:
            assert ex0["edgelet_reject"] >= 5 and ex1["edgelet_reject"] == 0, (k, ex0, ex1)
            was = [i for i, r in enumerate(rec0) if r["exit"] == "edgelet_reject"]
            assert (o0["pt_status"][was] == 1).all() and (o1["pt_status"][was] >= 2).sum() >= 3, (k, o1["pt_status"][was])
            rest = [i for i in range(sc.N_PTS) if i not in was]
            assert np.array_equal(o0["pt_depth"][rest], o1["pt_depth"][rest])
        else:
            assert (o1["pt_status"] >= 2).sum() < (o0["pt_status"] >= 2).sum(), k


def test_tie_case_scores_tie_and_the_first_best_wins(P, ob):
    """the edited frame of the tie case: inside a flat rectangle EVERY scored position has the best score; at a repeated texture exactly
    two have it, the alignment succeeds from the first one (the oracle's depth is the restatement's, which keeps the first by
    construction) and would end elsewhere from the second (their pixel columns are 10 apart)"""
    c = sc.case(P, ob, sc.TIE_CASE)
    o = c["oracle"]
    r, pt_rec, _ = sc.restated(P, ob, sc.TIE_CASE)
    assert len(c["edits"]["flat"]) == sc.N_FLAT and len(c["edits"]["repeat"]) >= 4, c["edits"]
    for i in c["edits"]["flat"]:
        rec = pt_rec[i]
        assert rec["n_scored"] >= 20 and rec["n_positions_at_best"] == rec["n_scored"] and rec["search_level"] == 0, (i, rec)
    n_ok = 0
    for i in c["edits"]["repeat"]:
        rec = pt_rec[i]
        assert rec["n_positions_at_best"] == 2 and rec["search_level"] == 0, (i, rec)
        if rec["exit"] == "walk_ok":
            n_ok += 1
            assert o["pt_status"][i] >= 2 and abs(o["pt_depth"][i] - r["pt_depth"][i]) <= 1e-9 * r["pt_depth"][i]
    assert n_ok >= 3, n_ok            # (4)


def test_inputs_reach_every_path(P, ob):
    """CONDITIONS on the inputs, tallied from the restatement's path records over all runs (the 19 cases and the 5 runs with other
    settings).  Not measurements: whoever changes the cases must keep every path populated.  (In brackets: the tally when written.)

    Left out, with the reason:
      * exit `warp_fail` (both variants): needs a NaN inverse of the warp matrix, i.e. det(A) = 0 or a non-finite A -- a depth
        hypothesis of exactly 0 or infinity (mu = inf or 0), not a finite seed;
      * exit `epi_nonfinite` in END-POINT searches: a NaN bound is caught before it (`nan_bounds`), and a finite bound gives a finite
        segment unless the hypothesis lies exactly in the current camera's focal plane.  POINT searches do reach it, through the planted
        NaN sigma2 (a non-finite input, counted below);
      * exit `nan_bounds` in POINT searches: the test exists only in the end-point variant;
      * status NAN (points and lines): `isnan(z_inv_min)` is only looked at after a successful search, and a NaN z_inv_min makes d_min
        and with it the whole segment NaN, which no search survives -- unreachable in the reference, the oracle and the kernel alike.
        Asserted to be absent, so that a change that makes it reachable shows up here.  The other four statuses are held to 4 each."""
    pt_ex, ep_ex, pairs, st_pt, lines = (collections.Counter() for _ in range(5))
    t = collections.Counter()
    first_phase = np.zeros(4, int)
    for k, over in RUNS:
        o = oracle_of(P, ob, k, over)
        _, pt_rec, seg_rec = sc.restated(P, ob, k, **over)
        st_pt.update(int(s) for s in o["pt_status"])
        pt_ex.update(r["exit"] for r in pt_rec)
        ep = [r for rr in seg_rec for r in rr if r is not None]
        ep_ex.update(r["exit"] for r in ep)
        for r in pt_rec + ep:
            walked = r["exit"] in ("no_score_below_threshold", "walk_ok", "walk_align_fail", "walk_tri_fail")
            if walked:
                pairs[(r["ref_level"], r["search_level"])] += 1
            t["search_level_3"] += walked and r["search_level"] == 3
            t["mixed_phase_winners"] += len(r["row_phases_best"]) >= 3
            if r["first_row_phase_best"] >= 0:
                first_phase[r["first_row_phase_best"]] += 1
            t["ties"] += r["n_positions_at_best"] >= 2
            t["border_crossings"] += r["n_out_of_frame_skipped"] > 0 and r["n_scored"] > 0
            t["nothing_scored"] += r["exit"] == "no_score_below_threshold" and r["n_scored"] == 0
            t["repeat_skips"] += r["n_repeat_skipped"] > 0
            t["long_walks"] += walked and r["n_steps"] >= 100
        for i, (rs, re) in enumerate(seg_rec):
            if rs["exit"] == "invisible":
                continue
            lines["first_failed"] += re is None
            lines["first_ok_second_failed"] += re is not None and not re["exit"].endswith("_ok")
            lines["both_ok"] += re is not None and re["exit"].endswith("_ok")
            lines["converged"] += o["seg_status"][i] == P.abi.SEED_CONVERGED
            lines["updated_not_converged"] += o["seg_status"][i] == P.abi.SEED_UPDATED
            lines["nan"] += o["seg_status"][i] == P.abi.SEED_NAN
    print("point exits", dict(pt_ex), "\nend-point exits", dict(ep_ex), "\n(ref level, search level) of walks", sorted(pairs.items()), "\n", dict(t),
          "\nfirst-row phase of winners", first_phase, "\npoint statuses", dict(st_pt), "\nlines", dict(lines))
    for e in ns.EXITS:
        if e not in ("warp_fail", "nan_bounds"):
            assert pt_ex[e] >= 4, (e, pt_ex)      # (least: walk_tri_fail 6, epi_nonfinite 19, short_align_fail 24; too_many_steps 115, 2 of them at the default limit)
        if e not in ("warp_fail", "epi_nonfinite", "edgelet_reject"):
            assert ep_ex[e] >= 2, (e, ep_ex)      # (least: walk_tri_fail 4, short_align_fail 5, no_score_below_threshold 10; too_many_steps 18, all with the limit of 5)
    assert pt_ex["warp_fail"] == 0 and ep_ex["warp_fail"] == 0 and ep_ex["epi_nonfinite"] == 0 and pt_ex["nan_bounds"] == 0 and ep_ex["edgelet_reject"] == 0
    for lv in range(4):
        for sl in range(3):
            assert pairs[(lv, sl)] >= 4, ((lv, sl), sorted(pairs.items()))      # (least: (0, 2) 13, (3, 0) 16)
    assert t["search_level_3"] >= 8, t            # (75) walks at search level 3 (n_pyr_levels = 4)
    assert t["mixed_phase_winners"] >= 20, t      # (585) winning positions whose eight rows have at least 3 distinct byte phases
    assert first_phase.min() >= 20, first_phase   # (382) each byte phase as the phase of a winning position's first row
    assert t["ties"] >= 4, t                      # (25) searches whose best score occurs at two or more positions
    assert t["border_crossings"] >= 4, t          # (193) positions skipped outside the patch margin AND positions scored, in one search
    assert t["nothing_scored"] >= 4, t            # (63) every position outside the margin
    assert t["repeat_skips"] >= 20, t             # (1619) searches that met the same pixel twice in a row
    assert t["long_walks"] >= 4, t                # (10) walks of 100 steps and more (the zoom of 0.75)
    for s in (0, 1, 2, 3):
        assert st_pt[s] >= 4, st_pt               # (421, 615, 1249, 19)
    assert st_pt[4] == 0 and lines["nan"] == 0, (st_pt, lines)
    for key in ("first_failed", "first_ok_second_failed", "both_ok", "converged", "updated_not_converged"):
        assert lines[key] >= 2, lines             # (88, 17, 214, 38, 176)
