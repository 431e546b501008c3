"""Cases shared by tests/test_gpu_tail_split.py (MI355X) and tests/test_emu_tail_split.py (the same file run against the host emulation
build): the alignment launch with its tail split (PLSVO_OPT_ALIGN_TAIL_SPLIT: the frames at the end of the launch order run as a coarse
and a fine workgroup of one launch, align_kernels.hip) against the same launch with one workgroup per frame.  Scheduling only: every
comparison here is bit for bit."""
import os

import numpy as np


def make_ctx(P, **env):
    """a context created under the given environment (the library reads its switches once, at create)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return P.capi.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def snapshot(ctx, n):
    """one align_run of the staged batch: everything the ABI reports about it"""
    ctx.align_run()
    res = ctx.align_fetch()
    return dict(res=res, work=ctx.align_work(), work_pt=ctx.align_work_points(), ties=ctx.align_chi2_ties(),
                order_next=ctx.align_launch_order(n), tail=ctx.align_tail_frames())


def assert_same_results(a, b, what):
    assert len(a["res"]) == len(b["res"])
    for k, (x, y) in enumerate(zip(a["res"], b["res"])):
        w = (what, k)
        assert x.T.tobytes() == y.T.tobytes(), w                    # (bytes: NaN payloads and signed zeros count)
        assert x.H.tobytes() == y.H.tobytes(), w
        assert np.float64(x.chi2).tobytes() == np.float64(y.chi2).tobytes(), w
        assert x.n_meas == y.n_meas and x.n_tracked == y.n_tracked, w
        assert x.iters_per_level == y.iters_per_level and x.status == y.status, w
        assert np.array_equal(x.seg_alive, y.seg_alive), w
    assert a["work"] == b["work"] and a["work_pt"] == b["work_pt"] and a["ties"] == b["ties"], (what, a["work"], b["work"], a["ties"], b["ties"])
    # the sort key of a split frame is the cost of both its parts: the refreshed order is the unsplit launch's
    assert np.array_equal(a["order_next"], b["order_next"]), what


def compare_split_on_off(ctx, jobs, tail_expected, reruns=3, refresh_modes=(True, False)):
    """the staged batch run `reruns` times with the split off, then on -- with the launch-order refresh and without --: re-run r of one
    equals re-run r of the other in every reported value, and the split took the frames it was asked to take"""
    n = len(jobs)
    for refresh in refresh_modes:
        runs = {}
        for split in (False, True):
            ctx.set_align_tail_split(split)
            ctx.set_launch_order_refresh(align=True)   # (False below: set_option puts the stage order back at once)
            ctx.align_stage(jobs)                      # staging resets the launch order to the stage call's
            if not refresh:
                ctx.set_launch_order_refresh(align=False)
            runs[split] = [snapshot(ctx, n) for _ in range(reruns)]
        for r in range(reruns):
            assert runs[False][r]["tail"] == 0 and runs[True][r]["tail"] == tail_expected, (refresh, r, runs[True][r]["tail"])
            assert_same_results(runs[False][r], runs[True][r], ("refresh" if refresh else "staged", r))
        if not refresh:   # the same order every time: the same launch every time
            assert_same_results(runs[True][0], runs[True][-1], "first against last re-run")
    ctx.set_launch_order_refresh(align=True)
    ctx.set_align_tail_split(True)
    return runs


def mixed_batch(P, W=320, H=240):
    """ten frames on five scenes: feature counts 40 .. 100 / 4 .. 20, level ranges 3..1, 2..0, 3..0, 2..1, ONE level (3..3 and 1..1), a job
    without features (skipped), segments dead on entry, a violent motion (lines culled on the way), a static camera (solver stop at
    every level).  Returns (images [5, 2, H, W], jobs)."""
    streams = [P.synth.make_align_stream(7100 + i, W, H, 40 + 15 * i, 4 + 4 * i, max_level=3, motion_scale=(4.0 if i == 3 else 0.3 + 0.2 * i)) for i in range(5)]
    imgs = P.synth.render_streams(streams).numpy()
    I = np.array([0, 0, 0, 1, 0, 0, 0.0])

    def job(i, hi, lo, T=None, pts=slice(None), segs=slice(None), alive_in=None, same_image=False):
        s = streams[i]
        return P.abi.AlignJob(s.cam, hi, lo, 30, 1e-6, s.T_init if T is None else T, s.pt_px[pts], s.pt_xyz_ref[pts], s.seg_spx[segs], s.seg_epx[segs],
                              s.seg_len[segs], s.seg_p_ref[segs], s.seg_q_ref[segs], seg_alive_in=alive_in, ref_slot=2 * i, cur_slot=2 * i + (0 if same_image else 1))
    dead = np.ones(streams[4].seg_spx.shape[0], np.uint8)
    dead[::3] = 0
    jobs = [job(0, 3, 1), job(1, 2, 0), job(2, 3, 3), job(3, 3, 0), job(4, 2, 1, alive_in=dead),
            job(0, 3, 1, pts=slice(0, 0), segs=slice(0, 0)),   # no features: skipped
            job(1, 1, 1), job(2, 3, 1, T=I, same_image=True), job(3, 2, 1), job(4, 3, 0)]
    return imgs, jobs


def load_images(ctx, imgs, W, H, n_levels=4):
    ctx.config_pyramids(2 * imgs.shape[0], W, H, n_levels)
    for i in range(imgs.shape[0]):
        ctx.build_pyramid(2 * i, imgs[i, 0], 0)
        ctx.build_pyramid(2 * i + 1, imgs[i, 1], 0)
