"""The alignment's 6x6 solve with the static pivot order in every launch shape (PLSVO_OPT_ALIGN_STATIC_SOLVE: the order of Eigen's LDLT
is sorted once from the diagonals, exact ties and NaN diagonals take the per-step search) -- same arithmetic in the same order, so
option on equals option off bit for bit -- and the quotient 1. / Z of the slot's Jacobian in the one-wave-per-frame shape on landmarks
whose depth is 0, NaN, infinite, huge or tiny, against the oracle: the cases any other home for that division has to pass (a slot record
{X, Y, Z, 1. / Z} written once per level was built, measured slower and left out: tools/patches/align_stored_zinv.patch).
tests/test_emu_align_static_solve.py runs this file on the host emulation build."""
import numpy as np
import pytest

import align_static_solve_cases as S
import helpers as Hh
import tail_split_cases as C


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [64, 128, 512])
def test_static_solve_changes_no_result_on_a_mixed_batch(P, threads):
    """twelve 320x240 frames on four-image pyramids (the ten-frame mixed batch of the tail-split tests, a static-camera frame -- an
    infinite diagonal: the NaN route -- and a one-point frame -- rank-deficient: the zero-pivot rule): T, H, chi2, n_meas, iterations per
    level, status, seg_alive, the work and tie counters and the per-iteration trace with the option on equal those with it off, over two
    re-runs.  64 and 128 threads per frame took the search until now; at 512 the option's off side is the new one."""
    imgs, jobs = S.solve_batch(P)
    ctx = P.capi.Context(0)
    try:
        C.load_images(ctx, imgs, S.W, S.H)
        ctx.set_launch_shapes(align_threads=threads)
        runs = S.compare_static_solve_on_off(ctx, jobs)
        # the two frames did take the routes they are here for: a NaN step and the solver's stop at every level of the static cameras,
        # components dropped by the zero-pivot rule in every step of the one-point frame
        trace = runs[True][0]["trace"]
        for k in (7, 10):
            assert len(trace[k]) >= 1 and all(np.isnan(r["x"]).all() and r["stop"] for r in trace[k]), k
        assert len(trace[11]) >= 1 and all((r["x"] == 0.0).sum() >= 3 and not np.isnan(r["x"]).any() for r in trace[11])
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def depth_case(P, ob):
    """the 320x240 case of test_gpu_parity.py's per-iteration parity test ("level0": 60 points, 20 segments, levels 2..0), whose tolerances
    the ordinary-depth frame is held to: they are stated for that test's frames (a frame with fewer points per line is dominated by the
    per-line float sum of |res|, which the device adds in tree order -- 1.3e-6 on H for 40 points and 12 segments, on this tree and on its
    parent alike)"""
    st, ref, cur, _ = Hh.make_case(ob, 14, S.W, S.H, 60, 20, 3, 2, 0)
    return st, ref, cur


@pytest.mark.gpu
@pytest.mark.parametrize("depth", S.DEPTHS, ids=[d[0] for d in S.DEPTHS])
def test_reciprocal_depth_of_the_jacobian_follows_the_oracle(P, ob, depth_case, depth):
    """one-wave-per-frame shape, the depth of five points and two segments set to the value: the same decisions as the oracle (NaN pattern
    of the pose, culled segments, status, measurement counts record by record, accepted steps) and the same pose inside the parity bar,
    as the adversarial cases of test_gpu_parity.py ask; the frame with ordinary depths also record for record against the oracle's
    iteration trace at the per-iteration parity test's tolerances."""
    tag, z = depth
    st, ref, cur = depth_case
    job = S.depth_job(P, st, z)
    ro, lo = ob.sparse_align(job, ref, cur, max_log=S.TRACE)
    ctx = P.capi.Context(0)
    try:
        ctx.config_pyramids(2, S.W, S.H, 3)
        ctx.upload_pyramid(0, ref)
        ctx.upload_pyramid(1, cur)
        ctx.set_launch_shapes(align_threads=64)
        ctx.align_set_trace(S.TRACE)
        rd = ctx.sparse_align(job)
        ld = ctx.align_fetch_trace(0)
    finally:
        ctx.close()
    To, Td = np.asarray(ro.T, float), np.asarray(rd.T, float)
    assert np.array_equal(np.isnan(To), np.isnan(Td)), (tag, To, Td)
    assert np.array_equal(rd.seg_alive, ro.seg_alive), tag
    assert rd.status == ro.status, (tag, rd.status, ro.status)
    n = Hh.common_prefix(lo, ld)
    assert n == min(len(lo), len(ld)) or n >= 1, (tag, n, len(lo), len(ld))
    for a, b in list(zip(lo, ld))[:n]:
        assert a["n_meas"] == b["n_meas"] and a["accepted"] == b["accepted"], (tag, a["level"], a["iter"])
        assert np.array_equal(np.isnan(a["x"]), np.isnan(b["x"])) or not a["accepted"], (tag, a["x"], b["x"])
    assert Hh.same_path(lo, ld), (tag, n, len(lo), len(ld))
    assert (rd.n_meas, rd.n_tracked, rd.iters_per_level) == (ro.n_meas, ro.n_tracked, ro.iters_per_level), tag
    if not np.isnan(To).any():
        assert Hh.pose_close(Td, To)[2], (tag, Hh.pose_close(Td, To))
    if z is None:
        nrec, worst = Hh.compare_align_logs(lo, ld)
        assert nrec == len(lo) >= 1
        assert worst["H"] < 1e-6 and worst["Jres"] < 1e-3 and worst["chi2"] < 1e-4, worst
