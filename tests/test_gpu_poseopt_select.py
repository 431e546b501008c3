"""The medians of the pose optimiser's row kernels (PLSVO_OPT_POSEOPT_SELECT, poseopt_select.hpp): every lane fetches its values once
into registers, the first digit starts at the highest bit in which the row's minimum and maximum differ, and the last (at most 16)
candidates are finished by rank; a wave with a row above 320 values keeps the radix select over memory.  An order statistic has one
value, so everything here is bit for bit: plsvo_poseopt_row_select -- the very device function, four rows per workgroup -- against
np.sort, and the whole pipeline with the option off against on.  tests/test_emu_poseopt_select.py runs this file (less the full-size
case) on the host emulation build."""
import collections

import numpy as np
import pytest

import poseopt_refill_cases as R
import poseopt_select_cases as S

# rows per route over family_rows(bits): 16 sizes x 3 ranks (n = 1 has one distinct rank, n = 2 two) x 13 families = 585 rows, of which 78
# lie above the cap; counted by S.model_path, which the device's path words must equal row by row (the counts are the same for both widths)
ROUTES = {S.EQUAL: 126, S.RANK: 275, S.RANK | S.EXTRA: 16, S.DIGITS: 38, S.DIGITS | S.EXTRA: 52, S.FALLBACK: 78}


@pytest.fixture(scope="module")
def ctx(P):
    c = P.capi.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [32, 64])
def test_row_select_equals_numpy_sort_on_every_family(ctx, bits):
    """n in SIZES x k in {0, n / 2, n - 1} x the value families of poseopt_select_cases.families, one launch per width: the selected
    pattern is np.sort(patterns)[k], and the path word of every row is the route the model predicts -- so each route provably ran, as
    often as ROUTES says"""
    rows = S.family_rows(bits)
    sel, path = rows.run(ctx)
    exp = rows.expected()
    want = [0 if not a else (S.FALLBACK if n > S.CAP else S.model_path(v, k, bits)) for v, n, k, a in zip(rows.vals, rows.n, rows.k, rows.active)]
    bad = [(rows.names[i], hex(int(sel[i])), hex(int(exp[i])), int(path[i]), want[i]) for i in range(len(exp)) if sel[i] != exp[i] or path[i] != want[i]]
    assert not bad, (len(bad), bad[:8])
    counts = collections.Counter(int(p) for p, a in zip(path, rows.active) if a)
    print("routes", bits, dict(counts))
    assert dict(counts) == ROUTES


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [32, 64])
def test_row_select_with_the_option_off_is_the_radix_select(P, bits):
    """PLSVO_OPT_POSEOPT_SELECT = 0: every active row reports the fallback, same patterns"""
    c = P.capi.Context(0)
    try:
        c.set_poseopt_select(False)
        rows = S.family_rows(bits)
        sel, path = rows.run(c)
        assert np.array_equal(sel, rows.expected())
        assert all(int(p) == (S.FALLBACK if a else 0) for p, a in zip(path, rows.active))
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [32, 64])
def test_row_select_waves_of_mixed_rows(P, ctx, bits):
    """rows of a wave share a program counter: an inactive row, a row of one value, a row at the cap and (second workgroup) one above it
    -- there the whole wave reports the fallback; third workgroup: an active flag on an empty row counts as inactive; the last
    workgroup is not full"""
    rng = np.random.default_rng(77 + bits)
    rows = S.Rows(bits)
    d = lambda n: S._distinct(rng, n, bits)
    rows.add("inactive", d(50), 25, False); rows.add("one value", d(1), 0); rows.add("at the cap", d(S.CAP), S.CAP // 2); rows.add("model", S.model_errors(rng, 280, bits), 140)
    rows.add("inactive", d(50), 25, False); rows.add("one value", d(1), 0); rows.add("at the cap", d(S.CAP), S.CAP // 2); rows.add("above the cap", d(S.CAP + 1), 7)
    rows.add("empty but flagged", d(0), 0); rows.add("17 values", d(17), 16); rows.add("inactive above the cap", d(700), 3, False); rows.add("two values", d(2), 1)
    rows.add("last workgroup, one row", S.model_errors(rng, 200, bits), 100)
    sel, path = rows.run(ctx)
    assert np.array_equal(sel, rows.expected()), (sel, rows.expected())
    assert [int(p) for p in path[:4]] == [0, S.EQUAL, S.RANK, S.RANK]
    assert [int(p) for p in path[4:8]] == [0, S.FALLBACK, S.FALLBACK, S.FALLBACK]
    assert int(path[8]) == 0 and int(path[10]) == 0 and not (int(path[9]) | int(path[11]) | int(path[12])) & S.FALLBACK
    assert ctx.poseopt_row_select(np.zeros(0, rows.ut), [], [], [], [])[0].size == 0
    with pytest.raises(P.capi.PlsvoError):
        ctx.poseopt_row_select(d(5), [0], [5], [5], [1])     # k outside [0, n)
    with pytest.raises(P.capi.PlsvoError):
        ctx.poseopt_row_select(d(5), [1], [5], [0], [1])     # the row runs past the patterns


def _select_on_off(ctx, jobs, refill):
    """the staged batch run twice (the second run of a large batch takes the refreshed launch order) with the select off, then on"""
    ctx.set_poseopt_refill(refill)
    runs = {}
    for on in (False, True):
        ctx.set_poseopt_select(on)
        ctx.poseopt_stage(jobs)
        runs[on] = [R.snapshot(ctx, len(jobs)) for _ in range(2)]
    for r in range(2):
        assert runs[False][r]["refill"] == runs[True][r]["refill"]
        R.assert_same_results(runs[False][r], runs[True][r], ("select off / on, refill", refill, "run", r))
    return runs


@pytest.mark.gpu
def test_select_changes_no_result_on_a_mixed_batch(P):
    """mixed_batch (0 .. 3 features, points only, lines only, 200 + 80, a NaN pose, identical points, n_iter = 0; the 500 + 200 frames are
    above the cap and force the fallback in their waves) in the row shape, as one kernel and as the three of the row refill: every
    field of the fetch, the pose records and the work counters equal the radix select's, byte for byte"""
    jobs = R.mixed_batch(P)
    ctx = R.make_ctx(P, PLSVO_POSEOPT_REFILL_MIN=4, PLSVO_POSEOPT_REORDER_MIN=4)
    try:
        ctx.set_launch_shapes(poseopt_threads=16)
        assert _select_on_off(ctx, jobs, False)[True][0]["refill"] == 0
        assert _select_on_off(ctx, jobs, True)[True][0]["refill"] == len(jobs)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_select_changes_no_result_with_a_refinement_job(P):
    """one job of the 10-argument overload (n_iter_ref > 0): its error_init is the median over both loops' entries (2 x 160 values)"""
    jobs = R.mixed_batch(P, 41)
    jobs[17] = P.poseopt_job_from_frame(P.synth.make_poseopt_frame(79, 120, 40), n_iter_ref=5)
    ctx = R.make_ctx(P, PLSVO_POSEOPT_REFILL_MIN=4, PLSVO_POSEOPT_REORDER_MIN=4)
    try:
        ctx.set_launch_shapes(poseopt_threads=16)
        runs = _select_on_off(ctx, jobs, True)
        assert runs[True][0]["refill"] == 0 and runs[True][0]["res"][17].iters_ref > 0
    finally:
        ctx.close()


@pytest.mark.gpu
def test_select_leaves_the_resident_frame_step_unchanged(P):
    """plsvo_frame_step_batch on six streams with the row shape forced: every result equals the run with the option off"""
    ctx = R.make_ctx(P, PLSVO_POSEOPT_REFILL_MIN=4)
    try:
        cam, jobs = R.chain_jobs(P, ctx)
        ctx.set_launch_shapes(poseopt_threads=16)
        out = {}
        for on in (False, True):
            ctx.set_poseopt_select(on)
            out[on] = (ctx.frame_step_batch(jobs, cam, n_pyr_levels=3, cell_size=40, cell_rule=False), ctx.fetch_pose_records(len(jobs)))
        for k, (a, b) in enumerate(zip(out[False][0], out[True][0])):
            for f in R.RESULT_FIELDS:
                assert np.asarray(getattr(a.pose, f)).tobytes() == np.asarray(getattr(b.pose, f)).tobytes(), (k, f)
            assert a.align.T.tobytes() == b.align.T.tobytes() and np.array_equal(a.sel_pt, b.sel_pt) and np.array_equal(a.sel_seg, b.sel_seg), k
        assert out[False][1].tobytes() == out[True][1].tobytes()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_select_changes_no_result_full_size(P):
    """2048 frames of 200 + 80 features drawn from 64 distinct seeds (the benchmark's pose-optimiser frames) in the row shape, one kernel
    and the three of the row refill"""
    pool = [P.poseopt_job_from_frame(P.synth.make_poseopt_frame(1234 + i, 200, 80, 640, 480)) for i in range(64)]
    jobs = [pool[(7 * k) % len(pool)] for k in range(2048)]
    ctx = R.make_ctx(P, PLSVO_POSEOPT_REFILL_MIN=4)
    try:
        ctx.set_launch_shapes(poseopt_threads=16)
        _select_on_off(ctx, jobs, False)
        assert _select_on_off(ctx, jobs, True)[True][0]["refill"] == len(jobs)
    finally:
        ctx.close()
