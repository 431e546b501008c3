"""Cases shared by tests/test_gpu_poseopt_refill.py (MI355X) and tests/test_emu_poseopt_refill.py (the same file run against the host
emulation build): the row shape of the pose optimiser as three launches whose Gauss-Newton rows take their next frame from a queue
(PLSVO_OPT_POSEOPT_REFILL, poseopt_kernels.hip) against the one launch with four frames of a wave in lock step.  Scheduling only: every
comparison here is bit for bit."""
import copy

import numpy as np

from tail_split_cases import make_ctx  # noqa: F401  (a context created under a given environment)

RESULT_FIELDS = ("T", "cov", "pt_keep", "seg_keep", "iters", "iters_ref", "num_obs_pt", "num_obs_ls", "estimated_scale", "error_init", "error_final", "status")


def _bytes(v):
    return np.asarray(v).tobytes()   # (bytes: NaN payloads and signed zeros count)


def snapshot(ctx, n):
    """one poseopt_run of the staged batch: everything the ABI reports about it"""
    ctx.poseopt_run()
    return dict(res=ctx.poseopt_fetch(), recs=ctx.fetch_pose_records(n), work=ctx.poseopt_work(), refill=ctx.poseopt_refill_frames())


def assert_same_results(a, b, what):
    assert len(a["res"]) == len(b["res"])
    for k, (x, y) in enumerate(zip(a["res"], b["res"])):
        for f in RESULT_FIELDS:
            assert _bytes(getattr(x, f)) == _bytes(getattr(y, f)), (what, k, f, getattr(x, f), getattr(y, f))
    assert a["recs"].tobytes() == b["recs"].tobytes(), what
    assert a["work"] == b["work"], (what, a["work"], b["work"])


def compare_refill_on_off(ctx, jobs, expect_refill, reruns=2):
    """the batch staged and run `reruns` times (from the second run on a large batch takes the refreshed launch order) with the refill
    off, then on: run r of one equals run r of the other in every reported value, and the query says which path ran"""
    n = len(jobs)
    runs = {}
    for on in (False, True):
        ctx.set_poseopt_refill(on)
        ctx.poseopt_stage(jobs)
        runs[on] = [snapshot(ctx, n) for _ in range(reruns)]
    ctx.set_poseopt_refill(True)
    for r in range(reruns):
        assert runs[False][r]["refill"] == 0 and runs[True][r]["refill"] == (n if expect_refill else 0), (r, runs[True][r]["refill"])
        assert_same_results(runs[False][r], runs[True][r], ("run", r))
    assert_same_results(runs[True][0], runs[True][-1], "first against last re-run")   # a frame's result does not depend on its place in the launch
    return runs


def mixed_batch(P, n=211):
    """n frames (not a multiple of four) of mixed size in no particular order: 0, 1, 2, 3 features, points only, lines only, a few dozen
    of each, 200 + 80 and 500 + 200; and the special frames of test_pose_optimizer_row_per_frame_shape_on_a_mixed_batch: noise-free at the
    true pose, far outliers, a NaN pose, identical points, n_iter = 0 -- so that the rows of a wave hold frames of different feature and
    iteration counts and refill at different times."""
    mk = P.synth.make_poseopt_frame
    sizes = [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (2, 2), (40, 0), (0, 25), (60, 20), (17, 9), (33, 5), (7, 3), (25, 12)]
    frames = []
    for i in range(n):
        npts, nseg = sizes[(5 * i) % len(sizes)]
        frames.append((mk(4000 + i, npts, nseg), {"n_iter": 3 + i % 8} if i % 6 == 5 else {}))
    for k, i in enumerate(range(9, n, 50)):
        frames[i] = (mk(4500 + i, 200, 80), {})
    frames[30] = (mk(4601, 500, 200), {})
    frames[n - 2] = (mk(4602, 500, 200), {})
    fr = mk(96, 60, 20)
    f3 = copy.copy(fr); f3.pt_pos = fr.pt_pos.copy(); f3.pt_pos[:5] = 1e6
    f4 = copy.copy(fr); f4.T_init = fr.T_init.copy(); f4.T_init[6] = np.nan
    f5 = copy.copy(fr); f5.pt_pos = np.repeat(fr.pt_pos[:1], len(fr.pt_pos), 0); f5.pt_f = np.repeat(fr.pt_f[:1], len(fr.pt_f), 0)
    special = [(mk(95, 60, 20, noise_px=0.0, outlier_frac=0.0, pert_t=0.0, pert_r=0.0), {}), (f3, {}), (f4, {}), (f5, {}), (fr, {"n_iter": 0}),
               (fr, {"n_iter": 0, "n_iter_ref": 0}), (fr, {"n_iter_ref": 0}), (f4, {"n_iter": 1})]
    for k, s in enumerate(special):
        frames[(3 + 23 * k) % n] = s
    return [P.poseopt_job_from_frame(f, **kw) for f, kw in frames]


def chain_jobs(P, ctx, n_streams=6):
    """a small resident frame step: n_streams streams of 320x240 (the set-up of test_resident_chain_applies_the_reprojection_grid_rule)"""
    import importlib
    seqm = importlib.import_module("pl-svo_amd.sequence")
    abi, synth = P.abi, P.synth
    seqs = [seqm.make_sequence(8 + s, n_frames=2, W=320, H=240, n_pts=60 + 20 * (s % 3), n_seg=10) for s in range(n_streams)]
    cam = seqs[0]["cam"]
    ctx.config_pyramids(2 * n_streams, 320, 240, 4)
    jobs = []
    for s, seq in enumerate(seqs):
        ctx.build_pyramid(2 * s, seq["images"][0], 0)
        ctx.build_pyramid(2 * s + 1, seq["images"][1], 0)
        T0 = seq["poses_true"][0]
        ref_pos = synth.se3_inv(T0)[4:]
        scaled = lambda px, pos: seqm._bearing(cam, px) * np.linalg.norm(pos - ref_pos, axis=1)[:, None]
        aj = abi.AlignJob(cam, 3, 1, 30, 1e-6, [0, 0, 0, 1, 0, 0, 0], seq["pt_px0"], scaled(seq["pt_px0"], seq["pt_pos"]), seq["seg_spx0"], seq["seg_epx0"],
                          np.linalg.norm(seq["seg_epx0"] - seq["seg_spx0"], axis=1), scaled(seq["seg_spx0"], seq["seg_spos"]),
                          scaled(seq["seg_epx0"], seq["seg_epos"]), ref_slot=2 * s, cur_slot=2 * s + 1)
        n_pts, n_seg = len(seq["pt_pos"]), len(seq["seg_spos"])
        pos_all = np.concatenate([seq["pt_pos"], seq["seg_spos"], seq["seg_epos"]])
        jobs.append(abi.ChainJob(aj, T0, T0, 2 * s, n_pts, n_seg, pos_all, np.concatenate([seq["pt_px0"], seq["seg_spx0"], seq["seg_epx0"]]),
                                 np.concatenate([seq["pt_f0"], seq["seg_sf0"], seq["seg_ef0"]])))
    return cam, jobs
