"""Row refill of the large-batch pose-optimiser launch (PLSVO_OPT_POSEOPT_REFILL, poseopt_kernels.hip): the row shape runs as three
kernels -- prologue, a persistent Gauss-Newton kernel whose 16-lane rows take their next frame from a queue as soon as their frame
stops, epilogue -- instead of one whose four frames per wave iterate until the last of them stops.  Scheduling only: with the refill
on, every value the ABI reports equals the one launch's bit for bit.  tests/test_emu_poseopt_refill.py runs the small cases of this
file on the host emulation build, where the first workgroup of the persistent kernel drains the whole queue."""
import numpy as np
import pytest

import poseopt_refill_cases as C


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 2, 0], ids=["one-workgroup", "two-workgroups", "all-resident"])
def test_refill_changes_no_result_on_a_mixed_batch(P, waves):
    """211 frames of mixed size (0 .. 3 features, points only, lines only, 200 + 80, 500 + 200, a NaN pose, far outliers, identical
    points, n_iter = 0, n_iter from 3 to 10) with the threshold lowered to four frames and the persistent kernel at one workgroup (every
    row refills some fifty times), two, and as many as the device holds; run twice, so that the second run takes the launch order
    refreshed from the first: every field of the fetch, the pose records and the work counters equal the one launch's."""
    jobs = C.mixed_batch(P)
    assert len(jobs) % 4 != 0
    ctx = C.make_ctx(P, PLSVO_POSEOPT_REFILL_MIN=4, PLSVO_POSEOPT_REFILL_WAVES=waves, PLSVO_POSEOPT_REORDER_MIN=4)
    try:
        ctx.set_launch_shapes(poseopt_threads=16)
        C.compare_refill_on_off(ctx, jobs, True)
        # below the threshold the one launch runs, and the other launch shapes never take the queue
        ctx.poseopt_stage(jobs[:3])
        ctx.poseopt_run()
        assert ctx.poseopt_refill_frames() == 0
        ctx.set_launch_shapes(poseopt_threads=64)
        ctx.poseopt_stage(jobs)
        ctx.poseopt_run()
        assert ctx.poseopt_refill_frames() == 0
    finally:
        ctx.close()


@pytest.mark.gpu
def test_refill_leaves_refinement_and_traced_batches_to_the_one_launch(P):
    """a batch with ONE job of the 10-argument overload (n_iter_ref > 0), and a batch with the iteration trace on: the query reports 0
    and the results equal the run with the option off"""
    jobs = C.mixed_batch(P, 41)
    ref = list(jobs)
    ref[17] = P.poseopt_job_from_frame(P.synth.make_poseopt_frame(79, 120, 40), n_iter_ref=5)
    ctx = C.make_ctx(P, PLSVO_POSEOPT_REFILL_MIN=4, PLSVO_POSEOPT_REORDER_MIN=4)
    try:
        ctx.set_launch_shapes(poseopt_threads=16)
        runs = C.compare_refill_on_off(ctx, ref, False)
        assert runs[True][0]["res"][17].iters_ref > 0
        ctx.poseopt_set_trace(12)
        try:
            C.compare_refill_on_off(ctx, jobs, False)
            assert len(ctx.poseopt_fetch_trace(9)) > 0
        finally:
            ctx.poseopt_set_trace(0)
        C.compare_refill_on_off(ctx, jobs, True)   # (the same context, trace off again: the queue)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_refill_leaves_the_resident_frame_step_unchanged(P):
    """plsvo_chain_run on six streams with the row shape forced and the threshold lowered: its pose-optimiser jobs are written on the
    device (the host cannot see whether one has a refinement loop), so the frame step keeps the one launch -- the query reports 0 -- and
    every result equals the run with the option off"""
    ctx = C.make_ctx(P, PLSVO_POSEOPT_REFILL_MIN=4)
    try:
        cam, jobs = C.chain_jobs(P, ctx)
        ctx.set_launch_shapes(poseopt_threads=16)
        out = {}
        for on in (False, True):
            ctx.set_poseopt_refill(on)
            res = ctx.frame_step_batch(jobs, cam, n_pyr_levels=3, cell_size=40, cell_rule=False)
            out[on] = (res, ctx.fetch_pose_records(len(jobs)))
            assert ctx.poseopt_refill_frames() == 0
        for k, (a, b) in enumerate(zip(out[False][0], out[True][0])):
            for f in C.RESULT_FIELDS:
                assert np.asarray(getattr(a.pose, f)).tobytes() == np.asarray(getattr(b.pose, f)).tobytes(), (k, f)
            assert a.align.T.tobytes() == b.align.T.tobytes() and np.array_equal(a.sel_pt, b.sel_pt) and np.array_equal(a.sel_seg, b.sel_seg), k
        assert out[False][1].tobytes() == out[True][1].tobytes()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_refill_engages_by_itself_full_size(P):
    """32768 frames of 200 + 80 features (512 distinct ones in seed order, the benchmark's pose-optimiser frames) -- or, on a device with
    more than 512 CUs, the smallest batch above two frames per resident row: the row shape and the refill engage on their own, staged
    order and refreshed order; every frame's result equals the one launch's."""
    pool = [P.poseopt_job_from_frame(P.synth.make_poseopt_frame(1234 + i, 200, 80, 640, 480)) for i in range(512)]
    ctx = P.capi.Context(0)
    try:
        cus = ctx.device_info()[1]
        n = max(32768, 64 * cus + 4)
        jobs = [pool[k % len(pool)] for k in range(n)]
        runs = C.compare_refill_on_off(ctx, jobs, True)
        its = np.array([r.iters for r in runs[True][0]["res"]])
        assert its.min() >= 1 and its.max() == 10 and len(np.unique(its)) > 3   # (the bimodal iteration counts the refill exists for)
    finally:
        ctx.close()
