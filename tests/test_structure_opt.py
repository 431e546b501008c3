"""Structure optimisation (hot-path contract row (f) "next" #3): plsvo::Point::optimize / LineSeg::optimize,
src/feature3D_impl.cpp:36-174.  CPU: the C oracle against a NumPy restatement and known answers.
GPU: the HIP kernel is compiled without fma contraction and must reproduce the oracle BIT FOR BIT."""
import numpy as np
import pytest

import np_structopt as nso


def test_oracle_points_match_numpy_restatement(P, ob):
    """the oracle against tests/np_structopt.py (term by term in the reference's order, its own pivoted LDLT -- singular systems
    included): bit for bit"""
    d = P.synth.make_structure_batch(1, n_pts=12, n_seg=0)
    res = ob.structure_optimize(P.structopt_job_from_batch(d))
    for i in range(12):
        o0, o1 = d["pt_obs_off"][i], d["pt_obs_off"][i + 1]
        pos, iters, _ = nso.point_optimize(d["frame_T"], d["pt_pos"][i], d["pt_obs_frame"][o0:o1], d["pt_obs_f"][o0:o1], 5)
        assert iters == res["pt_iters"][i]
        assert np.array_equal(pos, res["pt_pos"][i])
    # one observation each: singular (rank-2) normal equations
    d["pt_obs_off"] = np.arange(13, dtype=np.int32)
    res = ob.structure_optimize(P.structopt_job_from_batch(d))
    for i in range(12):
        pos, iters, rec = nso.point_optimize(d["frame_T"], d["pt_pos"][i], d["pt_obs_frame"][i:i + 1], d["pt_obs_f"][i:i + 1], 5)
        assert any(rec.solves[0].zeroed) and iters == res["pt_iters"][i] and np.array_equal(pos, res["pt_pos"][i])


def test_oracle_segments_are_two_coupled_point_problems(P, ob):
    """LineSeg::optimize runs the point update on both end points but breaks / rolls back jointly (:139-146, :169): the oracle equals
    the restatement of the joint loop bit for bit on every segment, and the joint exits are not those of the two ends alone"""
    d = P.synth.make_structure_batch(2, n_pts=0, n_seg=10)
    res = ob.structure_optimize(P.structopt_job_from_batch(d))
    coupled = 0
    for i in range(10):
        o0, o1 = d["seg_obs_off"][i], d["seg_obs_off"][i + 1]
        fr, sf, ef = d["seg_obs_frame"][o0:o1], d["seg_obs_sf"][o0:o1], d["seg_obs_ef"][o0:o1]
        sp, ep, iters, rec = nso.segment_optimize(d["frame_T"], d["seg_spos"][i], d["seg_epos"][i], fr, sf, ef, 5)
        assert iters == res["seg_iters"][i], rec
        assert np.array_equal(sp, res["seg_spos"][i]) and np.array_equal(ep, res["seg_epos"][i]), rec
        ps, its, _ = nso.point_optimize(d["frame_T"], d["seg_spos"][i], fr, sf, 5)
        pe, ite, _ = nso.point_optimize(d["frame_T"], d["seg_epos"][i], fr, ef, 5)
        assert iters == min(its, ite)                    # whichever end stops or fails first ends both
        coupled += int(not (np.array_equal(ps, sp) and np.array_equal(pe, ep)))
    assert coupled >= 3                                  # ... so a segment is not two independent point problems


def test_known_answer_triangulation(P, ob):
    """noise-free bearings from >= 3 views: the landmark must move (close) to its true position"""
    d = P.synth.make_structure_batch(3, n_pts=20, n_seg=20, noise_px=0.0, pert=0.05, obs_range=(3, 6))
    res = ob.structure_optimize(P.structopt_job_from_batch(d, 10, 10))
    e0 = np.linalg.norm(d["pt_pos"] - d["pt_true"], axis=1)
    e1 = np.linalg.norm(res["pt_pos"] - d["pt_true"], axis=1)
    assert np.median(e1) < 1e-6 and np.all(e1 < e0 + 1e-12)
    es = np.linalg.norm(res["seg_spos"] - d["seg_s_true"], axis=1)
    assert np.median(es) < 1e-6


def test_edge_cases(P, ob):
    # a landmark without observations: A = 0 -> dp = 0 -> unchanged after one evaluation
    d = P.synth.make_structure_batch(4, n_pts=3, n_seg=0)
    d["pt_obs_off"] = np.array([0, 0, 0, 0], np.int32)
    res = ob.structure_optimize(P.structopt_job_from_batch(d))
    assert np.array_equal(res["pt_pos"], d["pt_pos"]) and list(res["pt_iters"]) == [1, 1, 1]
    # zero iterations: untouched
    d = P.synth.make_structure_batch(5, n_pts=4, n_seg=4)
    res = ob.structure_optimize(P.structopt_job_from_batch(d, 0, 0))
    assert np.array_equal(res["pt_pos"], d["pt_pos"]) and np.array_equal(res["seg_epos"], d["seg_epos"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(11, 20, 20, 6), (12, 500, 300, 12), (13, 64, 0, 4), (14, 0, 33, 5), (15, 5000, 5000, 40)])
def test_hip_structure_optimize_is_bit_exact(P, ob, gpu_ctx, case):
    seed, npts, nseg, nfr = case
    d = P.synth.make_structure_batch(seed, npts, nseg, nfr)
    job = P.structopt_job_from_batch(d)
    ro = ob.structure_optimize(job)
    rd = gpu_ctx.structure_optimize(job)
    assert np.array_equal(rd["pt_iters"], ro["pt_iters"]) and np.array_equal(rd["seg_iters"], ro["seg_iters"])
    assert np.array_equal(rd["pt_pos"], ro["pt_pos"]), np.abs(rd["pt_pos"] - ro["pt_pos"]).max()
    assert np.array_equal(rd["seg_spos"], ro["seg_spos"]) and np.array_equal(rd["seg_epos"], ro["seg_epos"])


@pytest.mark.gpu
def test_hip_structure_optimize_edge_cases(P, ob, gpu_ctx):
    d = P.synth.make_structure_batch(21, n_pts=3, n_seg=2)
    d["pt_obs_off"] = np.array([0, 0, 0, 0], np.int32)
    job = P.structopt_job_from_batch(d)
    ro, rd = ob.structure_optimize(job), gpu_ctx.structure_optimize(job)
    assert np.array_equal(rd["pt_pos"], ro["pt_pos"]) and np.array_equal(rd["seg_spos"], ro["seg_spos"])
    # landmarks with ONE observation: rank-2 3x3 normal equations -- A.ldlt().solve(b) returns a zero component for the depth
    # direction (Eigen 3.2's zero-pivot rule, oracle flavour 320) and the device must return the same bits
    d = P.synth.make_structure_batch(23, n_pts=6, n_seg=0)
    d["pt_obs_off"] = np.arange(7, dtype=np.int32)
    job1 = P.structopt_job_from_batch(d)
    ro, rd = ob.structure_optimize(job1), gpu_ctx.structure_optimize(job1)
    assert np.all(np.isfinite(ro["pt_pos"]))
    assert np.array_equal(rd["pt_pos"], ro["pt_pos"]) and np.array_equal(rd["pt_iters"], ro["pt_iters"])
    job0 = P.structopt_job_from_batch(P.synth.make_structure_batch(22, 4, 4), 0, 0)
    rd = gpu_ctx.structure_optimize(job0)
    assert np.array_equal(rd["pt_pos"], job0.pt_pos)
