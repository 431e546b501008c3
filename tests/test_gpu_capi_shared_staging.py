"""The one-shot calls of the C ABI share one staging allocation and one output allocation (s_d_in / s_d_out, laid out per call by
Blob / Carver of pl-svo_amd/csrc/capi_transfer.hpp) and one pinned readback buffer: a stale offset or a view read after the next fetch
shows only when calls FOLLOW each other.  Here they do, on one context, and every output must equal -- bit for bit -- the output of
the same call made alone on a fresh context.  The inputs are the directed cases of match_warp_cases, structopt_cases, seed_search_cases
and keyframe_cases, whose own tests hold each call to the oracle."""
import ctypes as C

import numpy as np
import pytest

import keyframe_cases as kc
import match_warp_cases as mc
import poseopt_refill_cases as rc
import seed_search_cases as sc
import structopt_cases as stc


def _same(a, b, what):
    assert type(a) is type(b), what
    if isinstance(a, dict):
        assert list(a) == list(b), what
        for k in a:
            _same(a[k], b[k], (what, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for k, (x, y) in enumerate(zip(a, b)):
            _same(x, y, (what, k))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), what
    else:
        assert np.array([a]).tobytes() == np.array([b]).tobytes(), what


def _match_subset(P, c, rows):
    d = dict(c["d"])
    for key in ("cur_frame", "ref_frame", "ref_px", "ref_f", "ref_level", "ref_type", "ref_grad", "pos", "px_cur"):
        d[key] = c["d"][key][rows]
    return P.match_job_from_batch(d, c["n_pyr_levels"])


def _calls(P, ob):
    """[(name, call(ctx) -> result)] in an order that changes every section size from call to call: each call stages into the shared buffers"""
    m = mc.case(P, ob, 5)
    ty = m["d"]["ref_type"][:65]
    assert (ty == P.abi.FTR_CORNER).any() and (ty == P.abi.FTR_EDGELET).any()
    match65, match1 = _match_subset(P, m, slice(0, 65)), _match_subset(P, m, slice(70, 71))

    def match(job):
        def call(ctx):
            mc.load_frames(ctx, m["frames"])
            return ctx.match_direct(job)
        return call

    reproj = P.abi.ReprojectJob(m["d"]["cam"], m["d"]["frame_T"], m["d"]["cur_frame"][:3], m["d"]["pos"][:3])
    so_pts = P.structopt_job_from_batch(stc.batch(stc.POINTS[:9], []))
    so_segs = P.structopt_job_from_batch(stc.batch([], stc.SEGMENTS[:5]))
    so_both = P.structopt_job_from_batch(stc.layout(65, 3))
    s = sc.case(P, ob, 0)
    corner = [r for r in sc.PT_ROWS["wide"] if s["pt"]["type"][r] == P.abi.FTR_CORNER][0]
    pt, seg = sc.select(s, [corner], [sc.SEG_ROWS["wide"][0], sc.SEG_ROWS["wide"][1]])
    seeds = P.abi.SeedsJob(s["st"].cam, s["frame_T"], np.array([0, 1]), pt, seg, **sc.options(s))
    seeds.c.pt_grad = C.cast(None, P.abi.c_double_p)            # no gradient array at all: the kernel is told so

    def seeds_call(ctx):
        sc.load_frames(ctx, s["frames"])
        return ctx.update_seeds(seeds)

    decide = list(kc.need_new_kf_batch()[1:3])
    return [("match65", match(match65)), ("reproject3", lambda ctx: ctx.reproject(reproj)), ("structopt_points", lambda ctx: ctx.structure_optimize(so_pts)),
            ("structopt_segments", lambda ctx: ctx.structure_optimize(so_segs)), ("structopt_both", lambda ctx: ctx.structure_optimize(so_both)),
            ("update_seeds", seeds_call), ("keyframe_decide2", lambda ctx: ctx.keyframe_decide(decide)), ("match1", match(match1)),
            ("match65_again", match(match65))]


@pytest.mark.gpu
def test_one_shot_calls_in_a_row_equal_each_call_alone(P, ob):
    calls = _calls(P, ob)
    shared = P.capi.Context(0)
    try:
        in_a_row = [(name, call(shared)) for name, call in calls]
    finally:
        shared.close()
    for name, got in in_a_row:
        alone = P.capi.Context(0)
        try:
            want = dict(calls)[name](alone)
        finally:
            alone.close()
        _same(got, want, name)
    assert in_a_row[0][1]["found"].sum() > 30 and in_a_row[5][1]["pt_status"].size == 1 and in_a_row[5][1]["seg_status"].size == 2


def _chain_fields(r):
    return dict(T=r.align.T, H=r.align.H, chi2=r.align.chi2, n_meas=r.align.n_meas, seg_alive=r.align.seg_alive, T_f_w=r.pose.T,
                cov=r.pose.cov, pt_keep=r.pose.pt_keep, seg_keep=r.pose.seg_keep, found=r.found, px=r.px, search_level=r.search_level,
                sel_pt=r.sel_pt, sel_seg=r.sel_seg)


@pytest.mark.gpu
def test_chain_fetch_with_a_stream_without_candidates_equals_each_stream_alone(P):
    """two streams, the second without a single candidate: nine ranges come back, three of them shorter than their neighbours expect"""
    abi = P.abi
    ctx = P.capi.Context(0)
    try:
        cam, jobs = rc.chain_jobs(P, ctx, n_streams=2)
        z3 = np.zeros((0, 3))
        jobs[1] = abi.ChainJob(jobs[1].align_job, jobs[1].c.T_prev_w[:], jobs[1].c.T_kf_w[:], jobs[1].c.kf_slot, 0, 0, z3, np.zeros((0, 2)), z3)
        both = [_chain_fields(r) for r in ctx.frame_step_batch(jobs, cam)]
        assert both[0]["found"].sum() > 20 and both[1]["found"].size == 0 and both[1]["sel_pt"].size == 0 and np.isfinite(both[1]["T"]).all()
    finally:
        ctx.close()
    for k in range(2):
        alone = P.capi.Context(0)
        try:
            rc.chain_jobs(P, alone, n_streams=2)                 # (configures and fills the same four pyramid slots)
            _same(_chain_fields(alone.frame_step_batch([jobs[k]], cam)[0]), both[k], ("stream", k))
        finally:
            alone.close()
