"""Tail split of the large-batch alignment launch (PLSVO_OPT_ALIGN_TAIL_SPLIT, align_kernels.hip): the frames at the end of the launch
order run as two workgroups of ONE launch -- coarse levels first of all, finest level last of all -- and hand the solver state over in
HBM behind a per-frame flag.  Scheduling only: with the split on, every value the ABI reports equals the unsplit launch's bit for bit.
tests/test_emu_tail_split.py runs the small cases of this file on the host emulation build."""
import numpy as np
import pytest

import helpers as Hh
import tail_split_cases as C


@pytest.mark.gpu
@pytest.mark.parametrize("tail", [3, 5, 10])
def test_tail_split_changes_no_result_on_a_mixed_batch(P, tail):
    """ten frames (mixed feature counts and level ranges, a one-level frame, a skipped job, segments dead on entry, culls on the way, a
    solver stop) with the threshold lowered to four frames and the tail set at 3 (S < n), 5 (S = n / 2) and 10 (every frame) of them:
    T, H, chi2, n_meas, iterations per level, status, seg_alive, the work counters, the tie counters and the refreshed launch order
    equal the unsplit launch's over three re-runs, with the launch-order refresh and without."""
    W, H = 320, 240
    imgs, jobs = C.mixed_batch(P, W, H)
    ctx = C.make_ctx(P, PLSVO_ALIGN_REORDER_MIN=4, PLSVO_ALIGN_TAIL_MIN=4, PLSVO_ALIGN_TAIL_FRAMES=tail)
    try:
        C.load_images(ctx, imgs, W, H)
        ctx.set_launch_shapes(align_threads=64)
        C.compare_split_on_off(ctx, jobs, tail)
        # below the threshold nothing is split, and the other launch shapes never are
        ctx.align_stage(jobs[:3])
        ctx.align_run()
        assert ctx.align_tail_frames() == 0
        ctx.set_launch_shapes(align_threads=128)
        ctx.align_stage(jobs)
        ctx.align_run()
        assert ctx.align_tail_frames() == 0
    finally:
        ctx.close()


@pytest.mark.gpu
def test_tail_split_on_two_pass_levels(P, ob):
    """1920x1080 frames with lines of more than 64 samples at level 0 (a two-pass level, as the fine part of a split frame and -- levels
    1..0 of a job whose range starts lower -- as its only level), S = n / 2 and S = n"""
    st, ref, cur, job = Hh.make_case(ob, 41, 1920, 1080, 30, 6, 3, 1, 0, n_iter=10, seg_len_range=(1150.0, 1800.0))
    assert P.capi.align_slot_layout(job, 0)[3], "the case must contain a level that runs in two passes"
    jobs = [job, P.align_job_from_stream(st, 2, 0, n_iter=10), P.align_job_from_stream(st, 0, 0, n_iter=10), P.align_job_from_stream(st, 2, 1, n_iter=10)]
    for tail in (2, 4):
        ctx = C.make_ctx(P, PLSVO_ALIGN_REORDER_MIN=2, PLSVO_ALIGN_TAIL_MIN=4, PLSVO_ALIGN_TAIL_FRAMES=tail)
        try:
            ctx.config_pyramids(2, 1920, 1080, 3)
            ctx.upload_pyramid(0, ref)
            ctx.upload_pyramid(1, cur)
            ctx.set_launch_shapes(align_threads=64)
            C.compare_split_on_off(ctx, jobs, tail, reruns=2)
        finally:
            ctx.close()


@pytest.mark.gpu
def test_tail_split_engages_by_itself_full_size(P):
    """the smallest batch that takes the split on its own: the one-wave-per-frame shape starts at 64 frames per CU, which is eight rounds
    of resident workgroups (the split asks for four); 320x240 frames with 60 .. 100 features cycling through 128 scenes.  The tail set is
    two rounds; every frame's result equals the unsplit launch's."""
    W, H, scenes = 320, 240, 128
    streams = [P.synth.make_align_stream(9000 + i, W, H, 60 + 10 * (i % 5), 12 + 2 * (i % 4), max_level=3, motion_scale=0.3 + 0.2 * (i % 5)) for i in range(scenes)]
    imgs = P.synth.render_streams(streams).numpy()
    ctx = P.capi.Context(0)
    try:
        cus = ctx.device_info()[1]
        n = 64 * cus + 8
        C.load_images(ctx, imgs, W, H)
        pool = [P.align_job_from_stream(s, 3, 1, ref_slot=2 * i, cur_slot=2 * i + 1) for i, s in enumerate(streams)]
        jobs = [pool[(7 * k) % scenes] for k in range(n)]
        C.compare_split_on_off(ctx, jobs, 2 * cus * 8, reruns=2, refresh_modes=(False,))
    finally:
        ctx.close()
