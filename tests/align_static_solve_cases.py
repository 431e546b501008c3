"""Cases shared by tests/test_gpu_align_static_solve.py (MI355X) and tests/test_emu_align_static_solve.py (the same file run against the
host emulation build): the alignment's 6x6 solve with the static pivot order on and off (PLSVO_OPT_ALIGN_STATIC_SOLVE,
plsvo_wave.hpp::wave_solve6_core) in every launch shape, and the Jacobian's 1. / Z of the throughput shapes (align_kernels.hip) on
landmarks whose depth leaves the ordinary range."""
import numpy as np

import tail_split_cases as C

W, H = 320, 240
TRACE = 200


def solve_batch(P):
    """the ten-frame mixed batch of tail_split_cases (mixed feature counts and level ranges, a one-level frame, a skipped job, segments
    dead on entry, culls, a solver stop) plus a static-camera frame over levels 2..0 (cur == ref, T = I: a line's mean |res| is 0, the
    diagonal infinite -- the NaN route of the solve) and a one-point frame (rank-deficient: the zero-pivot rule).
    Returns (images [5, 2, H, W], jobs)."""
    imgs, jobs = C.mixed_batch(P, W, H)
    streams = [P.synth.make_align_stream(7100 + i, W, H, 40 + 15 * i, 4 + 4 * i, max_level=3, motion_scale=(4.0 if i == 3 else 0.3 + 0.2 * i)) for i in (0, 1)]
    I = np.array([0, 0, 0, 1, 0, 0, 0.0])
    s = streams[1]
    jobs.append(P.abi.AlignJob(s.cam, 2, 0, 30, 1e-6, I, s.pt_px, s.pt_xyz_ref, s.seg_spx, s.seg_epx, s.seg_len, s.seg_p_ref, s.seg_q_ref,
                               ref_slot=2, cur_slot=2))
    s = streams[0]
    jobs.append(P.abi.AlignJob(s.cam, 3, 1, 30, 1e-6, s.T_init, s.pt_px[:1], s.pt_xyz_ref[:1], s.seg_spx[:0], s.seg_epx[:0], s.seg_len[:0],
                               s.seg_p_ref[:0], s.seg_q_ref[:0], ref_slot=0, cur_slot=1))
    return imgs, jobs


def snapshot(ctx, n):
    """one align_run of the staged (traced) batch: everything the ABI reports about it, the per-iteration trace of every frame included"""
    snap = C.snapshot(ctx, n)
    snap["trace"] = [ctx.align_fetch_trace(k) for k in range(n)]
    return snap


def assert_same_trace(a, b, what):
    assert len(a) == len(b), what
    for k, (la, lb) in enumerate(zip(a, b)):
        assert len(la) == len(lb), (what, k, len(la), len(lb))
        for r, (x, y) in enumerate(zip(la, lb)):
            assert sorted(x) == sorted(y)
            for key in x:
                assert np.asarray(x[key]).tobytes() == np.asarray(y[key]).tobytes(), (what, k, r, key, x[key], y[key])   # (bytes: NaN counts)


def compare_static_solve_on_off(ctx, jobs, reruns=2):
    """the staged batch run `reruns` times with the option off, then on: re-run r of one equals re-run r of the other in every value"""
    n = len(jobs)
    runs = {}
    ctx.align_set_trace(TRACE)
    try:
        for on in (False, True):
            ctx.set_align_static_solve(on)
            ctx.align_stage(jobs)
            runs[on] = [snapshot(ctx, n) for _ in range(reruns)]
    finally:
        ctx.set_align_static_solve(True)
        ctx.align_set_trace(0)
    for r in range(reruns):
        C.assert_same_results(runs[False][r], runs[True][r], ("static solve off / on", r))
        assert_same_trace(runs[False][r]["trace"], runs[True][r]["trace"], ("static solve off / on", r))
    return runs


# depths a landmark can carry: the Jacobian divides by them
DEPTHS = [("ordinary", None), ("zero", 0.0), ("nan", np.nan), ("plus-inf", np.inf), ("minus-inf", -np.inf), ("huge", 1e200), ("tiny", 1e-200)]


def depth_job(P, st, z):
    """the stream's job over levels 2..0 with the depth of its first five points and of both 3-D end points of its first two segments set
    to z (None: the stream as it is)"""
    xyz, p, q = st.pt_xyz_ref.copy(), st.seg_p_ref.copy(), st.seg_q_ref.copy()
    if z is not None:
        xyz[:5, 2] = z
        p[:2, 2] = z
        q[:2, 2] = z
    return P.abi.AlignJob(st.cam, 2, 0, 30, 1e-6, st.T_init, st.pt_px, xyz, st.seg_spx, st.seg_epx, st.seg_len, p, q)
