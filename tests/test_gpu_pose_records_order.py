"""plsvo_fetch_pose_records behind a resident frame step that is still staged: a pose-optimisation batch staged and run AFTER the step is
"the one that ran last" and is what the records describe.  The order was found by the suite itself -- a frame-step test and the mixed
pose-optimiser batch one after the other on one context -- so this runs exactly that: the two existing tests, in that order, on a context
of its own (before the fix the second one was refused with "n does not match the resident batch")."""
import importlib

import pytest

import test_gpu_parity
import test_sequence


@pytest.mark.gpu
def test_a_pose_batch_that_ran_after_a_staged_frame_step_is_the_records_source(P, ob):
    seqm = importlib.import_module("pl-svo_amd.sequence")
    ctx = P.capi.Context(0)
    try:
        test_sequence.test_resident_chain_applies_the_segment_grid_rule(P, ob, ctx, seqm)       # leaves its frame step staged
        test_gpu_parity.test_pose_optimizer_row_per_frame_shape_on_a_mixed_batch(P, ob, ctx)    # stages, runs and fetches the records of 19 frames
        # and the step, staged and run again, is the source again
        test_sequence.test_resident_chain_applies_the_reprojection_grid_rule(P, ob, ctx, seqm)
    finally:
        ctx.close()
