"""The keyframe stage on the device (plsvo_close_keyframes, plsvo_keyframe_decide; pl-svo_amd/csrc/keyframe_device.hpp) against its
restatement tests/np_keyframe.py on the cases of tests/keyframe_cases.py: batches of nine streams of unequal size.  Every output is
compared bit for bit, except delta_t / delta_r, whose logarithm calls the device's atan and tan."""
import ctypes as C

import numpy as np
import pytest

import keyframe_cases as Kc
import np_keyframe as K

# Worst relative deviation of delta_t / delta_r from the restatement over the cases of this file, measured on the MI355X:
# delta_t 2.377e-16, delta_r 2.729e-16 (the last bit of atan / tan; 0 on the host emulation, where both sides call the host's libm).
# The bound is 16 x the larger of the two, to leave room for other inputs, and in no case above 1e-12.
DELTA_WORST_T, DELTA_WORST_R = 2.377e-16, 2.729e-16
DELTA_REL_TOL = min(16 * max(DELTA_WORST_T, DELTA_WORST_R), 1e-12)


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def check_decide(got, want, tag):
    for f in ("has_depth", "n_depth", "need_new_kf", "blocking", "furthest_kf"):
        assert got[f] == want[f], (tag, f, got[f], want[f])
    for f in ("depth_mean", "depth_min"):
        assert bits(got[f]) == bits(want[f]), (tag, f, got[f], want[f])
    assert np.array_equal(got["key_pts"], want["key_pts"]), (tag, got["key_pts"], want["key_pts"])
    worst = [0.0, 0.0]
    for k, f in enumerate(("delta_t", "delta_r")):
        assert got[f].shape == want[f].shape
        zero = want[f] == 0.0                          # (delta_r of a pure translation: exactly 0 on both sides)
        assert np.array_equal(got[f][zero], want[f][zero]), (tag, f)
        if np.any(~zero):
            worst[k] = float(np.max(np.abs(got[f][~zero] - want[f][~zero]) / np.abs(want[f][~zero])))
            assert np.isfinite(worst[k]), (tag, f)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["depth_counts", "depth_patterns", "key_points", "need_new_kf"])
def test_keyframe_decide_equals_the_restatement(gpu_ctx, name):
    jobs = Kc.decide_batches()[name]
    res = gpu_ctx.keyframe_decide(list(jobs))
    worst_t = worst_r = 0.0
    for k, (j, r) in enumerate(zip(jobs, res)):
        wt, wr = check_decide(r, K.decide(j), (name, k))
        worst_t, worst_r = max(worst_t, wt), max(worst_r, wr)
    print(f"keyframe_decide[{name}]: worst relative deviation delta_t {worst_t:.3e} delta_r {worst_r:.3e}")
    assert worst_t <= DELTA_REL_TOL and worst_r <= DELTA_REL_TOL, (worst_t, worst_r)


@pytest.mark.gpu
def test_keyframe_decide_is_the_same_one_stream_at_a_time(gpu_ctx):
    """a stream's result does not depend on its place in the batch (wave, workgroup) -- deltas included, bit for bit"""
    jobs = list(Kc.decide_batches()["need_new_kf"])
    res = gpu_ctx.keyframe_decide(jobs)
    for k in (0, 3, 6, 8):
        one = gpu_ctx.keyframe_decide([jobs[k]])[0]
        for f in one:
            assert np.asarray(one[f]).tobytes() == np.asarray(res[k][f]).tobytes(), (k, f)


@pytest.mark.gpu
def test_close_keyframes_equal_the_restatement(gpu_ctx):
    jobs = Kc.close_batch()
    res = gpu_ctx.close_keyframes(list(jobs))
    for k, (j, r) in enumerate(zip(jobs, res)):
        w = K.close(j)
        assert (r["n_close"], r["n_overlap"]) == (w["n_close"], w["n_overlap"]), k
        assert np.array_equal(r["close_idx"], w["close_idx"]), (k, r["close_idx"], w["close_idx"])
        assert np.array_equal(bits(r["close_dist"]), bits(w["close_dist"])), k


@pytest.mark.gpu
def test_close_keyframes_project_like_plsvo_reproject(gpu_ctx, P):
    """isVisible uses the T * p and world2cam of plsvo_reproject: the keyframes whose first valid key point reprojects inside the image
    (z >= 0) are exactly the ones the call reports for a table with one valid key point per keyframe"""
    rng = np.random.default_rng(77)
    T = Kc.rand_pose(rng)
    kf_T, kp, kv = Kc._table(rng, T, 40, p_valid=1.0)
    kv[:, 1:] = 0
    r = gpu_ctx.close_keyframes([P.abi.CloseKeyframesJob(Kc.CAM, T, kf_T, kp, kv)])[0]
    pr = gpu_ctx.reproject(P.abi.ReprojectJob(Kc.CAM, [T], np.zeros(40, np.int32), kp[:, 0], cell_size=30, boundary=0))
    z = np.array([K.se3_act(T, p)[2] for p in kp[:, 0]])
    px = pr["px"]
    vis = (z >= 0) & (px[:, 0] >= 0) & (px[:, 1] >= 0) & (px[:, 0] < Kc.CAM.width) & (px[:, 1] < Kc.CAM.height)
    assert 0 < vis.sum() < 40 and sorted(r["close_idx"]) == list(np.nonzero(vis)[0])


@pytest.mark.gpu
def test_keyframe_decide_reads_the_resident_poses(P):
    """d_T_new = plsvo_chain_poses_dev after a small frame step: the same results as with the fetched poses, bit for bit"""
    import poseopt_refill_cases as R
    ctx = P.capi.Context(0)
    try:
        cam, cj = R.chain_jobs(P, ctx, n_streams=5)
        res = ctx.frame_step_batch(cj, cam, n_pyr_levels=3, cell_size=40, cell_rule=False)
        rng = np.random.default_rng(5)
        jobs_host, jobs_dev = [], []
        for r in res:
            T = np.array(r.pose.T, float)
            base = Kc.rand_decide_job(rng, 70, 12, 6, blocking_at=None, T_new=T)
            args = (Kc.CAM, None, list(base.c.T_last_w), base.pt_px, base.pt_pos, None, base.seg_spos, base.seg_epos, None, base.kf_T, base.overlap_idx,
                    list(base.c.key_pts_prev))
            jobs_host.append(P.abi.KeyframeDecideJob(args[0], T, *args[2:]))
            jobs_dev.append(P.abi.KeyframeDecideJob(args[0], [0, 0, 0, 1, 0, 0, 0], *args[2:]))     # T_new_w must not be looked at
        a = ctx.keyframe_decide(jobs_host)
        b = ctx.keyframe_decide(jobs_dev, poses_dev=ctx.chain_poses_dev())
        c = ctx.keyframe_decide(jobs_dev)
        for k in range(len(res)):
            for f in a[k]:
                assert np.asarray(a[k][f]).tobytes() == np.asarray(b[k][f]).tobytes(), (k, f)
        assert any(a[k]["depth_mean"] != c[k]["depth_mean"] for k in range(len(res)))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_keyframe_error_paths(gpu_ctx, P):
    L, h, A = gpu_ctx.L, gpu_ctx.h, P.abi
    inv = A.E_INVALID
    assert L.plsvo_close_keyframes(h, -1, None, None) == inv and L.plsvo_keyframe_decide(h, -1, None, None) == inv
    assert L.plsvo_close_keyframes(h, 1, None, None) == inv and L.plsvo_keyframe_decide(h, 1, None, None) == inv
    assert L.plsvo_close_keyframes(h, 0, None, None) == 0 and L.plsvo_keyframe_decide(h, 0, None, None) == 0
    ci, co = A.CloseKfIn(), A.CloseKfOut()
    ci.cam = Kc.CAM
    ci.n_kf = 2                                       # NULL table with a non-zero count
    assert L.plsvo_close_keyframes(h, 1, C.byref(ci), C.byref(co)) == inv
    ci.n_kf = -1
    assert L.plsvo_close_keyframes(h, 1, C.byref(ci), C.byref(co)) == inv
    ci.n_kf, ci.max_n_kfs = 0, -1
    assert L.plsvo_close_keyframes(h, 1, C.byref(ci), C.byref(co)) == inv
    good = Kc.decide_batches()["need_new_kf"][1]
    do = A.KfDecideOut()
    for field, value in (("n_pt", -1), ("n_seg", -1), ("n_kf", -1), ("n_overlap", -1), ("pt_px", None), ("pt_pos", None), ("seg_spos", None),
                         ("seg_epos", None), ("kf_T", None), ("overlap_idx", None)):
        di = A.KfDecideIn.from_buffer_copy(good.c)
        setattr(di, field, value)                      # (None: a NULL pointer)
        assert L.plsvo_keyframe_decide(h, 1, C.byref(di), C.byref(do)) == inv, field
    di = A.KfDecideIn.from_buffer_copy(good.c)
    di.key_pts_prev[2] = good.n_pt                     # a holder outside the points
    assert L.plsvo_keyframe_decide(h, 1, C.byref(di), C.byref(do)) == inv
    bad = np.array(good.overlap_idx); bad[0] = good.kf_T.shape[0]
    di = A.KfDecideIn.from_buffer_copy(good.c)
    di.overlap_idx = bad.ctypes.data_as(A.c_i32_p)
    assert L.plsvo_keyframe_decide(h, 1, C.byref(di), C.byref(do)) == inv
    di = A.KfDecideIn.from_buffer_copy(good.c)         # and the untouched copy passes
    assert L.plsvo_keyframe_decide(h, 1, C.byref(di), C.byref(do)) == 0 and do.blocking == 0
