"""The next frame's alignment job built on the device from the resident selection (plsvo_candidates_align_reserve / _build / _compose ..;
pl-svo_amd/csrc/alignjob_device.hpp) against its restatement tests/np_alignjob.py on the cases of tests/alignjob_cases.py.  Per case:
  * the fetched job (feature arrays, T0, the per-level slot codes, the launch-order key) and the report are byte for byte the
    restatement's, whose inputs are what the device holds at build time -- the fetched selection, the keep masks, the landmarks' types
    and positions as plsvo_candidates_fetch_quality / _fetch_map report them -- and the reference pose;
  * the codes, n_slots and long_lines are those of plsvo_align_slot_layout on the restatement's job wherever the two lay out alike (the
    host helper starts the segments right behind the points; a batch of at most cu_count / 2 streams starts them at a multiple of 64:
    every directed case therefore also runs inside a batch of cu_count / 2 + 1 streams);
  * plsvo_align_run + _fetch on the built batch equal plsvo_sparse_align_batch on the restatement's jobs bit for bit;
  * the composed pose equals the restated product.
The frames are driven with constructed match results (plsvo_candidates_set_match) and, where the pose optimiser would not produce the
pattern, with constructed keep masks."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import alignjob_cases as A
import candidates_cases as Cc
import insert_cases as Ic
import np_alignjob as NA
import select_cases as Sc

JOB_ARRAYS = ("T0", "T_ref", "n_slots", "pt_px", "pt_xyz_ref", "seg_spx", "seg_epx", "seg_len", "seg_p_ref", "seg_q_ref", "seg_alive_in", "seg_code")
JOB_INTS = ("n_pts", "n_seg", "skip", "long_mask", "n_patches")
RESULT = ("T", "H", "chi2", "n_meas", "n_tracked", "iters_per_level", "status")
N_SLOTS = 4


def same_bytes(got, want, tag):
    g = np.asarray(got)
    w = np.asarray(want, dtype=g.dtype)
    assert g.size == w.size and g.tobytes() == w.reshape(g.shape).tobytes(), (tag, g, w)


def make_ctx(P, geo):
    c = P.capi.Context(0)
    cam = geo["cam_t"]
    c.config_pyramids(N_SLOTS, cam[4], cam[5], A.N_PYR)
    for s, img in enumerate(A.images(cam, N_SLOTS)):
        c.build_pyramid(s, img)
    return c


@pytest.fixture(scope="module")
def ctx(P):
    c = make_ctx(P, A.SMALL)
    yield c
    c.close()


@pytest.fixture(scope="module")
def wide_ctx(P):
    c = make_ctx(P, A.WIDE)
    yield c
    c.close()


def stage(ctx, streams, reserve=None):
    geo = streams[0]["geo"] if "geo" in streams[0] else A.SMALL
    sts = [copy.deepcopy(s["st"]) for s in streams]
    ctx.candidates_reserve(**(reserve or {}))
    try:
        ctx.candidates_stage([Cc.to_job(st) for st in sts], Cc.abi.Pinhole(*geo["cam_t"]), geo["cell"], geo["seg_cell"], geo["boundary"])
    finally:
        ctx.candidates_reserve()
    ctx.candidates_set_quality([dict(pt_n_failed=st["pt_nfail"], pt_n_succeeded=st["pt_nsucc"], seg_n_failed=st["seg_nfail"], seg_n_succeeded=st["seg_nsucc"]) for st in sts])
    return geo


def frame(ctx, P, streams, outliers=False, params=None):
    """candidates -> constructed match -> selection on the device; the fetched selection (each stage has tests of its own)"""
    ctx.candidates_run([P.abi.CandidateFrameJob(s["T"], s["overlap"], cur_slot=1) for s in streams])
    matches = [Sc.match_of(s, r) for s, r in zip(streams, ctx.candidates_fetch())]
    if outliers:                                                      # every seventh match lands six pixels off: the pose optimiser rejects it
        for m in matches:
            m["px"][::7] += 6.0
    ctx.candidates_set_match(matches)
    ctx.candidates_select(**(params or A.PARAMS))
    return ctx.candidates_select_fetch()


def ones(sel):
    return np.ones(len(sel["pt_lm"]), np.uint8), np.ones(len(sel["seg_lm"]), np.uint8)


def seg_align_of(ctx, n):
    return 64 if 2 * n <= ctx.device_info()[1] else 32


def restate(ctx, geo, sels, masks, poses, cfg, active=None, prev=None):
    """the restatement of a build on what the device holds now: the types and positions of the tables"""
    n = len(sels)
    quality, maps = ctx.candidates_fetch_quality(), ctx.candidates_fetch_map()
    out = []
    for k in range(n):
        if active is not None and not active[k]:
            out.append(prev[k] if prev else NA.empty_job(cfg))
            continue
        q, m = quality[k], maps[k]
        out.append(NA.align_job(sels[k], masks[k][0], masks[k][1], q["pt_type"], q["seg_type"], np.asarray(m["pt_pos"]).reshape(-1, 3), np.asarray(m["seg_spos"]).reshape(-1, 3),
                                np.asarray(m["seg_epos"]).reshape(-1, 3), poses[k], geo["cam_t"], cfg, seg_align_of(ctx, n)))
    return out


def host_job(P, geo, cfg, w, ref_slot=0, cur_slot=1):
    return P.abi.AlignJob(geo["cam_t"], cfg["max_level"], cfg["min_level"], cfg.get("n_iter", 30), 1e-6, w["T0"], w["pt_px"], w["pt_xyz_ref"], w["seg_spx"], w["seg_epx"],
                          w["seg_len"], w["seg_p_ref"], w["seg_q_ref"], w["seg_alive_in"], ref_slot=ref_slot, cur_slot=cur_slot)


def check_jobs(ctx, P, geo, cfg, wants, tag, n=None):
    """the fetched jobs and reports against the restatement (the first len(wants) streams of a batch of n); the layout against
    plsvo_align_slot_layout where the two lay out alike"""
    align = seg_align_of(ctx, len(wants) if n is None else n)
    reports = ctx.candidates_align_fetch()
    for k, w in enumerate(wants):
        g = ctx.candidates_align_fetch_job(k)
        assert {f: reports[k][f] for f in w["report"]} == w["report"], (tag, k, reports[k], w["report"])
        assert {f: g[f] for f in JOB_INTS} == {f: w[f] for f in JOB_INTS}, (tag, k, {f: g[f] for f in JOB_INTS}, {f: w[f] for f in JOB_INTS})
        for f in JOB_ARRAYS:
            same_bytes(g[f], w[f], (tag, "job", k, f))
        if align == 32 or w["n_pts"] % 64 == 0 or w["n_seg"] == 0:
            job, patches = host_job(P, geo, cfg, w), 0
            for level in range(cfg["min_level"], cfg["max_level"] + 1):
                first, N, n_slots, long_lines, n_patches = P.capi.align_slot_layout(job, level)
                same_bytes(w["seg_code"][level - cfg["min_level"]], np.where(first >= 0, (N << 20) | first, -1), (tag, "slot_layout", k, level))
                assert (n_slots, int(long_lines)) == (int(w["n_slots"][level]), (w["long_mask"] >> level) & 1), (tag, k, level)
                patches += n_patches
            assert w["skip"] or patches == w["n_patches"], (tag, k)


def check_run(ctx, P, geo, cfg, wants, tag, slots=None):
    """plsvo_align_run + _fetch + _compose on the built batch against plsvo_sparse_align_batch on the restatement's jobs"""
    slots = [(0, 1)] * len(wants) if slots is None else slots
    ctx.align_run()
    got = ctx.align_fetch()
    ctx.candidates_align_compose()
    assert ctx.candidates_align_poses_dev()
    composed = [ctx.candidates_align_fetch_job(k)["T_f_w"] for k in range(len(wants))]
    want = ctx.sparse_align_batch([host_job(P, geo, cfg, w, *s) for w, s in zip(wants, slots)])
    for k, (g, r, w) in enumerate(zip(got, want, wants)):
        for f in RESULT:
            same_bytes(np.asarray(getattr(g, f)), np.asarray(getattr(r, f)), (tag, "run", k, f))
        same_bytes(g.seg_alive[:w["n_seg"]], r.seg_alive, (tag, "run", k, "seg_alive"))
        same_bytes(composed[k], NA.compose(r.T, w["T_ref"]), (tag, "composed", k))
    return want


def build(ctx, sels, masks, poses, active=None, slots=None, resident=()):
    """masks / poses per stream; `resident`: the streams whose masks the device reads from the pose optimiser"""
    jobs = []
    for k, (m, T) in enumerate(zip(masks, poses)):
        if active is not None and not active[k]:
            jobs.append(None)
            continue
        j = dict(ref_slot=slots[k][0] if slots else 0, cur_slot=slots[k][1] if slots else 1)
        if k not in resident:
            j.update(pt_keep=m[0], seg_keep=m[1])
        if isinstance(T, dict):
            j.update(T)                                               # poses_dev=.., or nothing: the resident pose
        else:
            j["T_f_w"] = T
        jobs.append(j)
    ctx.candidates_align_build(jobs)


def levels_n(w, cfg, level):
    """samples per segment feature at a level (0: no slots)"""
    code = w["seg_code"][level - cfg["min_level"]]
    return [int(c) >> 20 if c >= 0 else 0 for c in code]


def padded(streams, geo, n):
    """the streams at the head of a batch of n: the rest have no map at all"""
    return tuple(streams) + tuple(A.Builder(geo, 0).done() for _ in range(n - len(streams)))


def large_n(ctx):
    return ctx.device_info()[1] // 2 + 1


@pytest.mark.gpu
def test_keep_masks_a_doubly_won_segment_and_the_rounds_of_64(ctx, P):
    """80 point features and 14 segment features (two segments won both their cells): points and segments culled in the middle of the
    lists, the second instance of a doubly won segment among them; 70 kept points, whose kept set straddles a round of 64 in the
    ballot prefix; exactly 64 kept points; all kept"""
    streams = (A.eighty(),)
    geo, cfg = stage(ctx, streams), A.cfg()
    ctx.candidates_align_reserve(**cfg)
    sels = frame(ctx, P, streams)
    sel = sels[0]
    assert len(sel["pt_lm"]) == 80 and len(sel["seg_lm"]) == 14
    seg_lm = [int(v) for v in sel["seg_lm"]]
    twice = [i for i, lm in enumerate(seg_lm) if seg_lm.index(lm) != i]
    assert len(twice) == 2
    pk70, sk = ones(sel)
    pk70[[3, 9, 20, 31, 40, 41, 55, 62, 66, 77]] = 0
    sk[[2, 5, twice[0]]] = 0
    pk64 = np.ones(80, np.uint8)
    pk64[:8] = 0; pk64[60:68] = 0
    for n, (pk, run) in enumerate(((pk70, True), (pk64, True), (np.ones(80, np.uint8), False))):
        build(ctx, sels, [(pk, sk)], [A.T_REF])
        wants = restate(ctx, geo, sels, [(pk, sk)], [A.T_REF], cfg)
        assert wants[0]["n_pts"] == (70, 64, 80)[n] and wants[0]["report"]["n_seg_alive"] == 11 and wants[0]["n_seg"] == 14
        assert not np.array_equal(wants[0]["T0"], [0, 0, 0, 1, 0, 0, 0])               # cur.T_f_w * ref.T_f_w^-1: not the literal identity
        check_jobs(ctx, P, geo, cfg, wants, ("masks", n))
        if run:
            check_run(ctx, P, geo, cfg, wants, ("masks", n))


@pytest.mark.gpu
def test_a_landmark_deleted_by_the_insertions_keyframe_removal(ctx, P):
    """the insertion removes keyframe 3 (Map::safeDeleteFrame): landmarks with two observations or fewer are deleted and cut loose from the
    new keyframe's features -- their rows read TYPE_DELETED at build time and count as feat3D == NULL although their keep byte is set"""
    streams = (Ic.directed_stream(),)
    geo, cfg = stage(ctx, streams, Ic.RESERVE), A.cfg()
    ctx.candidates_align_reserve(**cfg)
    sels = frame(ctx, P, streams)
    masks = [Ic.keep_masks(streams[0], sels[0])]
    before = ctx.candidates_fetch_quality()[0]
    ctx.candidates_insert_keyframe([dict(remove_kf=3, kf_slot=1, T_f_w=Ic.T_NEW, pt_keep=masks[0][0], seg_keep=masks[0][1])])
    after = ctx.candidates_fetch_quality()[0]
    cut = [i for i, lm in enumerate(sels[0]["pt_lm"]) if masks[0][0][i] and before["pt_type"][lm] != NA.TYPE_DELETED and after["pt_type"][lm] == NA.TYPE_DELETED]
    cut_seg = [i for i, lm in enumerate(sels[0]["seg_lm"]) if masks[0][1][i] and before["seg_type"][lm] != NA.TYPE_DELETED and after["seg_type"][lm] == NA.TYPE_DELETED]
    assert cut and cut_seg
    build(ctx, sels, masks, [Ic.T_NEW])
    wants = restate(ctx, geo, sels, masks, [Ic.T_NEW], cfg)
    assert wants[0]["n_pts"] == int(masks[0][0].sum()) - len(cut) and not wants[0]["seg_alive_in"][cut_seg].any()
    check_jobs(ctx, P, geo, cfg, wants, "removal")
    check_run(ctx, P, geo, cfg, wants, "removal")


@pytest.mark.gpu
def test_empty_lists_a_skipped_and_an_inactive_stream(ctx, P):
    """0 points; 0 segments; nothing at all (skip), with and without a map; then a second build in which two streams sit out: their jobs,
    poses and reports are what the first build left"""
    streams = (A.only_points(), A.only_segments(), A.nothing_found(), A.no_map(), A.border())
    geo, cfg = stage(ctx, streams), A.cfg(cap_pts=16, cap_seg=8, slot_cap=256)
    ctx.candidates_align_reserve(**cfg)
    sels = frame(ctx, P, streams)
    masks = [ones(s) for s in sels]
    poses = [A.T_REF, Cc.IDENT, A.T_REF, Ic.T_NEW, Ic.T_NEW]
    active = [True, True, True, True, False]
    build(ctx, sels, masks, poses, active)
    first = restate(ctx, geo, sels, masks, poses, cfg, active)
    assert [(w["n_pts"], w["n_seg"], w["skip"]) for w in first] == [(9, 0, 0), (0, 6, 0), (0, 0, 1), (0, 0, 1), (0, 0, 1)]
    check_jobs(ctx, P, geo, cfg, first, "empty 1")
    check_run(ctx, P, geo, cfg, first, "empty 1")
    masks[0][0][4] = 0
    active = [True, False, False, True, True]
    build(ctx, sels, masks, poses, active)
    second = restate(ctx, geo, sels, masks, poses, cfg, active, prev=first)
    assert second[0]["n_pts"] == 8 and second[1] is first[1] and second[4]["n_pts"] == 5
    check_jobs(ctx, P, geo, cfg, second, "empty 2")
    check_run(ctx, P, geo, cfg, second, "empty 2")


@pytest.mark.gpu
def test_an_end_point_inside_the_border_at_level_3_only(ctx, P):
    streams = (A.border(),)
    geo, cfg = stage(ctx, streams), A.cfg(cap_pts=8, cap_seg=8, slot_cap=256)
    ctx.candidates_align_reserve(**cfg)
    sels = frame(ctx, P, streams)
    masks = [ones(sels[0])]
    build(ctx, sels, masks, [A.T_REF])
    wants = restate(ctx, geo, sels, masks, [A.T_REF], cfg)
    at = [i for i, p in enumerate(sels[0]["seg_px"]) if p[0] == 20.0]
    assert at and all(levels_n(wants[0], cfg, 3)[i] == 0 and levels_n(wants[0], cfg, 2)[i] > 0 and levels_n(wants[0], cfg, 1)[i] > 0 for i in at)
    assert sum(1 for v in levels_n(wants[0], cfg, 3) if v) == len(sels[0]["seg_lm"]) - len(at)
    check_jobs(ctx, P, geo, cfg, wants, "border")
    check_run(ctx, P, geo, cfg, wants, "border")


@pytest.mark.gpu
def test_a_stream_beyond_a_capacity_is_dropped_and_its_neighbours_are_intact(ctx, P):
    """cap_pts, cap_seg and slot_cap each exceeded by one stream of a batch of four"""
    streams = A.overflow_batch()
    geo, cfg = stage(ctx, streams), A.cfg(**A.OVERFLOW_CFG)
    ctx.candidates_align_reserve(**cfg)
    sels = frame(ctx, P, streams)
    masks = [ones(s) for s in sels]
    poses = [A.T_REF] * 4
    build(ctx, sels, masks, poses)
    wants = restate(ctx, geo, sels, masks, poses, cfg)
    rep = [w["report"] for w in wants]
    assert [r["status"] for r in rep] == [NA.NO_ROOM, NA.NO_ROOM, NA.NO_ROOM, NA.OK]
    assert rep[0]["n_pts"] == 30 and rep[0]["n_slots"] == 0                                   # the layout is not reached
    assert rep[1]["n_seg"] == 24 and rep[1]["n_pts"] <= 20
    assert rep[2]["n_pts"] == 10 and rep[2]["n_seg"] == 16 and rep[2]["n_slots"] > 80          # what the stream would have needed
    assert rep[3]["n_slots"] == 76 and [(w["skip"], w["n_pts"], w["n_seg"]) for w in wants] == [(1, 0, 0)] * 3 + [(0, 10, 2)]
    check_jobs(ctx, P, geo, cfg, wants, "overflow")
    check_run(ctx, P, geo, cfg, wants, "overflow")


@pytest.mark.gpu
def test_the_three_pose_sources_and_the_resident_masks(ctx, P):
    """a host pose, a device pointer and the resident optimised pose; NULL masks: the build reads the keep masks
    plsvo_candidates_pose_optimize left on the device (every seventh match is six pixels off and is culled)"""
    streams = (A.eighty(), A.border(), A.only_points())
    geo, cfg = stage(ctx, streams), A.cfg()
    ctx.candidates_align_reserve(**cfg)
    sels = frame(ctx, P, streams, outliers=True)
    ctx.candidates_pose_optimize()
    po = ctx.candidates_pose_fetch([(s["n_matches"], s["n_ls_matches"]) for s in sels])
    masks = [(p.pt_keep, p.seg_keep) for p in po]
    assert any(0 in m[0] for m in masks) and sum(int(m[0].sum()) for m in masks) > 30
    dev = ctx.candidates_poses_dev()
    build(ctx, sels, masks, [A.T_REF, dict(poses_dev=dev + 56), dict()], resident=(0, 1, 2))
    wants = restate(ctx, geo, sels, masks, [A.T_REF, po[1].T, po[2].T], cfg)
    check_jobs(ctx, P, geo, cfg, wants, "poses")
    check_run(ctx, P, geo, cfg, wants, "poses")


def packing_wants(wide_ctx, P, streams, tag, run=True):
    geo, cfg = stage(wide_ctx, streams), A.cfg(cap_pts=16, cap_seg=16, slot_cap=640)
    wide_ctx.candidates_align_reserve(**cfg)
    sels = frame(wide_ctx, P, streams)
    masks = [ones(s) for s in sels]
    poses = [A.T_REF] * len(streams)
    build(wide_ctx, sels, masks, poses)
    wants = restate(wide_ctx, geo, sels, masks, poses, cfg)
    check_jobs(wide_ctx, P, geo, cfg, wants, tag)
    if run:
        check_run(wide_ctx, P, geo, cfg, wants, tag)
    return cfg, wants


@pytest.mark.gpu
def test_segment_packing(wide_ctx, P):
    """N = 64 and N = 65 (a two-pass level, long_mask); a segment long at level 1 and short at level 2; equal N (tie order); enough shorts
    for four rounds, filled first-fit in decreasing N; a level with long segments only"""
    cfg, wants = packing_wants(wide_ctx, P, (A.sixty_four_and_five(), A.third_round(), A.equal_n(), A.long_only()), "packing")
    a, b, c, d = wants
    assert levels_n(a, cfg, 1) == [64, 64, 65, 65] and levels_n(a, cfg, 2) == [32, 32, 33, 33] and a["long_mask"] == 2
    first = [int(v) & 0xfffff for v in a["seg_code"][0]]
    assert first == [64, 128, 192, 257] and a["n_slots"][1] == 322                          # (two workgroups per frame: the segments start at 64)
    assert sorted(levels_n(b, cfg, 1)) == [10, 10, 20, 20, 30, 30, 40, 40] and b["long_mask"] == 0
    rounds = {}
    for code in b["seg_code"][0]:
        rounds.setdefault((int(code) & 0xfffff) // 64, []).append(int(code) >> 20)
    assert sorted(sorted(v) for v in rounds.values()) == [[10, 10], [20, 40], [20, 40], [30, 30]]
    assert levels_n(c, cfg, 1) == [13] * 6 + [5, 5] and [int(v) & 0xfffff for v in c["seg_code"][0]] == [64, 77, 90, 103, 128, 141, 116, 121]
    assert levels_n(d, cfg, 1) == [65, 65, 66, 66] and [int(v) & 0xfffff for v in d["seg_code"][0]] == [64, 129, 194, 260] and d["long_mask"] == 2


@pytest.mark.gpu
def test_the_directed_cases_in_a_large_batch_lay_out_like_the_host(ctx, wide_ctx, P):
    """a batch of cu_count / 2 + 1 streams starts the segments right behind the points (seg_align 32), as plsvo_align_slot_layout does:
    every directed case against the host helper, level by level; the same streams in a batch of two start them at a multiple of 64"""
    n = large_n(ctx)
    for c, head, kw in ((ctx, (A.eighty(), A.border(), A.only_segments(), A.small_lines(10, [(50, 200, 30.125 + 25 * k) for k in range(8)])), dict()),
                        (wide_ctx, (A.sixty_four_and_five(), A.third_round(), A.equal_n(), A.long_only()), dict(cap_pts=16, cap_seg=16, slot_cap=640))):
        streams = padded(head, head[0]["geo"], n)
        geo, cfg = stage(c, streams), A.cfg(n_iter=2, **kw)
        c.candidates_align_reserve(**cfg)
        sels = frame(c, P, streams)
        masks = [ones(s) for s in sels]
        poses = [A.T_REF] * n
        build(c, sels, masks, poses)
        assert seg_align_of(c, n) == 32
        wants = restate(c, geo, sels, masks, poses, cfg)
        check_jobs(c, P, geo, cfg, wants[:len(head) + 1], ("large", geo["cam_t"][4]), n=n)
        assert all(w["skip"] for w in wants[len(head):])
    # the small camera's batch again, run: a few features per stream
    streams = tuple(A.tiny(k % 30) for k in range(n))
    geo, cfg = stage(ctx, streams), A.cfg(cap_pts=8, cap_seg=8, slot_cap=96, n_iter=2)
    ctx.candidates_align_reserve(**cfg)
    sels = frame(ctx, P, streams)
    masks = [ones(s) for s in sels]
    build(ctx, sels, masks, [A.T_REF] * n)
    wants = restate(ctx, geo, sels, masks, [A.T_REF] * n, cfg)
    check_jobs(ctx, P, geo, cfg, wants, "tiny, large batch")
    order = ctx.align_launch_order(n)                                 # most patches first, in the sort's bins of four
    assert sorted(order) == list(range(n)) and all(wants[a]["n_patches"] >> 2 >= wants[b]["n_patches"] >> 2 for a, b in zip(order[:-1], order[1:]))
    check_run(ctx, P, geo, cfg, wants, "tiny, large batch")
    assert wants[1]["n_pts"] == 3 and [int(v) & 0xfffff for v in wants[1]["seg_code"][0]][0] == 3
    two = streams[:2]
    stage(ctx, two)
    ctx.candidates_align_reserve(**cfg)
    sels = frame(ctx, P, two)
    build(ctx, sels, masks[:2], [A.T_REF] * 2)
    assert seg_align_of(ctx, 2) == 64
    wants2 = restate(ctx, geo, sels, masks[:2], [A.T_REF] * 2, cfg)
    check_jobs(ctx, P, geo, cfg, wants2, "tiny, two")
    check_run(ctx, P, geo, cfg, wants2, "tiny, two")
    assert [int(v) & 0xfffff for v in wants2[1]["seg_code"][0]][0] == 64
    for f in ("pt_px", "pt_xyz_ref", "seg_p_ref", "seg_len"):
        same_bytes(wants2[1][f], wants[1][f], ("two", f))


def one_wave_ctx(P, geo):
    """a context whose alignment launches take the throughput shape (64 threads per frame) whatever the batch size"""
    old = os.environ.get("PLSVO_ALIGN_THREADS")
    os.environ["PLSVO_ALIGN_THREADS"] = "64"
    try:
        return make_ctx(P, geo)
    finally:
        if old is None:
            del os.environ["PLSVO_ALIGN_THREADS"]
        else:
            os.environ["PLSVO_ALIGN_THREADS"] = old


@pytest.mark.gpu
def test_more_than_64_rounds_of_shorts_and_a_level_beyond_the_bins(P):
    """70 features of more than 32 samples at level 1 open 68 rounds: the second bin group of the first-fit walk, with two shorts that fit
    nowhere in the first group; 136 such features need more rounds than the bins hold: the level cannot be laid out, the stream is
    dropped, its neighbour intact.  4480 slots fit a workgroup's LDS in the one-wave shape only (the reserve refuses them otherwise)"""
    cfg = A.cfg(cap_pts=8, cap_seg=140, slot_cap=4480)
    streams = (A.seventy_rounds(), A.beyond_the_bins())
    small = make_ctx(P, A.WIDE)
    try:
        stage(small, streams)
        with pytest.raises(P.capi.PlsvoError) as e:                   # two streams launch with 512 threads per frame: 44 bytes of LDS per slot
            small.candidates_align_reserve(**cfg)
        assert e.value.code == P.abi.E_CAPACITY
    finally:
        small.close()
    c = one_wave_ctx(P, A.WIDE)
    try:
        geo = stage(c, streams)
        c.candidates_align_reserve(**cfg)
        sels = frame(c, P, streams, params=dict(A.PARAMS, max_fts_segs=200))
        assert [len(s["seg_lm"]) for s in sels] == [70, 136]
        masks = [ones(s) for s in sels]
        build(c, sels, masks, [A.T_REF] * 2)
        wants = restate(c, geo, sels, masks, [A.T_REF] * 2, cfg)
        a, b = wants
        assert sorted(levels_n(a, cfg, 1)) == [30, 30] + [33] * 4 + [40] * 64 and a["n_slots"][1] == 68 * 64 - 31 and a["long_mask"] == 0
        rounds = {}
        for code in a["seg_code"][0]:
            rounds.setdefault((int(code) & 0xfffff) // 64, []).append(int(code) >> 20)
        assert len(rounds) == 68 and sorted(rounds[64]) == sorted(rounds[65]) == [30, 33] and rounds[66] == rounds[67] == [33]
        assert b["report"] == dict(n_pts=0, n_seg=136, n_seg_alive=136, n_slots=0, long_mask=0, status=NA.NO_ROOM) and (b["skip"], b["n_seg"]) == (1, 0)
        check_jobs(c, P, geo, cfg, wants, "bin groups")
        assert c.align_launch_shape()[0] == 64
        check_run(c, P, geo, cfg, wants, "bin groups")
    finally:
        c.close()


@pytest.mark.gpu
def test_one_wave_per_frame_reads_the_tiled_mirror_of_the_built_slots(P):
    """the throughput shape (64 threads per frame, forced here) reads the tiled mirror: plsvo_align_run refreshes the tiles of the slots
    the build named, which it knows from the records alone"""
    c = one_wave_ctx(P, A.SMALL)
    try:
        streams = (A.border(), A.only_points(), A.eighty())
        geo, cfg = stage(c, streams), A.cfg()
        c.candidates_align_reserve(**cfg)
        sels = frame(c, P, streams)
        masks = [ones(s) for s in sels]
        slots = [(2, 3), (0, 1), (1, 2)]
        build(c, sels, masks, [A.T_REF] * 3, slots=slots)
        wants = restate(c, geo, sels, masks, [A.T_REF] * 3, cfg)
        check_jobs(c, P, geo, cfg, wants, "one wave")
        got = c.candidates_align_fetch_job(0)
        assert (got["ref_slot"], got["cur_slot"]) == (2, 3)
        res = check_run(c, P, geo, cfg, wants, "one wave", slots=slots)
        assert all(r.n_tracked > 0 for r in res)
    finally:
        c.close()


@pytest.fixture
def own_ctx(P):
    c = make_ctx(P, A.SMALL)
    yield c
    c.close()


@pytest.mark.gpu
def test_alignjob_error_paths(own_ctx, P):
    ctx = own_ctx
    L, h, Ab = ctx.L, ctx.h, P.abi
    streams = (A.border(), A.only_points())
    g = Ab.CandAlignCfg(3, 1, 30, 16, 8, 256, 1e-6)
    # -- reserve
    fresh = P.capi.Context(0)
    try:
        assert fresh.L.plsvo_candidates_align_reserve(fresh.h, C.byref(g)) == Ab.E_STATE                 # no staged tables
        assert fresh.L.plsvo_candidates_align_build(fresh.h, 0, None) == Ab.E_STATE
        assert fresh.L.plsvo_candidates_align_fetch(fresh.h, 0, None) == Ab.E_STATE and fresh.L.plsvo_candidates_align_compose(fresh.h) == Ab.E_STATE
        assert fresh.L.plsvo_candidates_align_fetch_job(fresh.h, 0, C.byref(Ab.CandAlignJobOut())) == Ab.E_STATE and not fresh.candidates_align_poses_dev()
    finally:
        fresh.close()
    stage(ctx, streams)
    assert L.plsvo_candidates_align_reserve(h, None) == Ab.E_INVALID
    for field, bad in (("max_level", 4), ("min_level", 4), ("min_level", -1), ("n_iter", -1), ("cap_pts", 0), ("cap_seg", 0), ("slot_cap", 0), ("cap_pts", -3)):
        b = Ab.CandAlignCfg(3, 1, 30, 16, 8, 256, 1e-6)
        setattr(b, field, bad)
        assert L.plsvo_candidates_align_reserve(h, C.byref(b)) == Ab.E_INVALID, field
    assert L.plsvo_candidates_align_reserve(h, C.byref(Ab.CandAlignCfg(3, 1, 30, 16, 8, 8065, 1e-6))) == Ab.E_CAPACITY
    assert L.plsvo_candidates_align_reserve(h, C.byref(Ab.CandAlignCfg(3, 1, 30, 16, 8, 3500, 1e-6))) == Ab.E_CAPACITY          # two streams launch with 512 threads: beyond a workgroup's LDS
    jobs = (Ab.CandAlignJob * 2)()
    keep = np.ones(200, np.uint8)
    for j in jobs:
        j.active, j.ref_slot, j.cur_slot, j.pose_source, j.pt_keep, j.seg_keep = 1, 0, 1, Ab.INSERT_POSE_HOST, keep.ctypes.data_as(Ab.c_u8_p), keep.ctypes.data_as(Ab.c_u8_p)
        j.T_f_w[:] = A.T_REF
    ctx.candidates_run([Ab.CandidateFrameJob(s["T"], s["overlap"], cur_slot=1) for s in streams])
    ctx.candidates_set_match([Sc.match_of(s, r) for s, r in zip(streams, ctx.candidates_fetch())])
    ctx.candidates_select(**A.PARAMS)
    assert L.plsvo_candidates_align_build(h, 2, jobs) == Ab.E_STATE                                      # the stage dropped nothing, but nothing is reserved yet
    assert L.plsvo_candidates_align_reserve(h, C.byref(g)) == Ab.OK
    assert L.plsvo_candidates_align_compose(h) == Ab.E_STATE and not ctx.candidates_align_poses_dev()    # nothing built
    # -- build: state
    ctx.candidates_run([Ab.CandidateFrameJob(s["T"], s["overlap"], cur_slot=1) for s in streams])
    assert L.plsvo_candidates_align_build(h, 2, jobs) == Ab.E_STATE                                      # no selection on the last run
    ctx.candidates_set_match([Sc.match_of(s, r) for s, r in zip(streams, ctx.candidates_fetch())])
    ctx.candidates_select(**A.PARAMS)
    # -- build: arguments
    assert L.plsvo_candidates_align_build(h, 1, jobs) == Ab.E_INVALID and L.plsvo_candidates_align_build(h, 3, jobs) == Ab.E_INVALID
    assert L.plsvo_candidates_align_build(h, 2, None) == Ab.E_INVALID
    for field, bad in (("ref_slot", N_SLOTS), ("cur_slot", -1), ("pose_source", 3), ("pose_source", -1), ("pose_source", Ab.INSERT_POSE_DEV)):
        ok = getattr(jobs[1], field)
        setattr(jobs[1], field, bad)
        assert L.plsvo_candidates_align_build(h, 2, jobs) == Ab.E_INVALID, field
        setattr(jobs[1], field, ok)
    jobs[0].pt_keep = None
    assert L.plsvo_candidates_align_build(h, 2, jobs) == Ab.E_STATE                                      # NULL masks, no resident pose optimisation
    jobs[0].pt_keep = keep.ctypes.data_as(Ab.c_u8_p)
    jobs[1].pose_source = Ab.INSERT_POSE_RESIDENT
    assert L.plsvo_candidates_align_build(h, 2, jobs) == Ab.E_STATE                                      # ... for the pose
    jobs[1].pose_source = Ab.INSERT_POSE_HOST
    jobs[1].active, jobs[1].ref_slot = 0, 99                                                             # (an inactive stream's record is not looked at)
    assert L.plsvo_candidates_align_build(h, 2, jobs) == Ab.OK
    jobs[1].active, jobs[1].ref_slot = 1, 0
    # -- the built batch is the staged alignment batch; fetches
    assert L.plsvo_candidates_align_compose(h) == Ab.E_STATE                                             # it has not run
    reps = (Ab.CandAlignReport * 3)()
    assert L.plsvo_candidates_align_fetch(h, 1, reps) == Ab.E_INVALID and L.plsvo_candidates_align_fetch(h, 2, None) == Ab.E_INVALID
    assert L.plsvo_candidates_align_fetch(h, 2, reps) == Ab.OK and (reps[0].n_pts, reps[0].status, reps[1].n_pts) == (5, Ab.ALIGN_JOB_OK, 0)
    out = Ab.CandAlignJobOut()
    assert L.plsvo_candidates_align_fetch_job(h, 2, C.byref(out)) == Ab.E_INVALID and L.plsvo_candidates_align_fetch_job(h, -1, C.byref(out)) == Ab.E_INVALID
    assert L.plsvo_candidates_align_fetch_job(h, 0, None) == Ab.E_INVALID
    assert L.plsvo_candidates_align_fetch_job(h, 0, C.byref(out)) == Ab.OK and (out.n_pts, out.skip) == (5, 0)       # NULL buffers: the counts and poses alone
    assert L.plsvo_align_run(h) == Ab.OK and L.plsvo_candidates_align_compose(h) == Ab.OK and ctx.candidates_align_poses_dev()
    outs = (Ab.AlignOut * 2)()
    assert L.plsvo_align_fetch(h, 3, outs) == Ab.E_INVALID and L.plsvo_align_fetch(h, 2, outs) == Ab.OK
    # a host-staged batch replaces the built one: nothing to compose until the next build
    ctx.align_stage([P.abi.AlignJob(A.SMALL["cam_t"], 3, 1, 30, 1e-6, Cc.IDENT, np.zeros((0, 2)), np.zeros((0, 3)), np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(0),
                                    np.zeros((0, 3)), np.zeros((0, 3)))])
    assert L.plsvo_candidates_align_compose(h) == Ab.E_STATE
    assert L.plsvo_candidates_align_build(h, 2, jobs) == Ab.OK and L.plsvo_align_run(h) == Ab.OK and L.plsvo_candidates_align_compose(h) == Ab.OK
    # -- behind an insertion or an add the build is still in place (it reads the tables as they are); behind the compaction it is refused
    ins = (Ab.CandInsert * 2)()
    stage(ctx, streams, Ic.RESERVE)
    assert L.plsvo_candidates_align_build(h, 2, jobs) == Ab.E_STATE                                      # a new stage: no run
    ctx.candidates_run([Ab.CandidateFrameJob(s["T"], s["overlap"], cur_slot=1) for s in streams])
    ctx.candidates_set_match([Sc.match_of(s, r) for s, r in zip(streams, ctx.candidates_fetch())])
    ctx.candidates_select(**A.PARAMS)
    for a in ins:
        a.is_kf, a.remove_kf, a.kf_slot, a.pt_keep, a.seg_keep = 1, -1, 1, keep.ctypes.data_as(Ab.c_u8_p), keep.ctypes.data_as(Ab.c_u8_p)
    assert L.plsvo_candidates_insert_keyframe(h, 2, ins) == Ab.OK
    assert L.plsvo_candidates_align_build(h, 2, jobs) == Ab.OK
    assert L.plsvo_candidates_compact(h, 2, (Ab.CandCompact * 2)()) == Ab.OK
    assert L.plsvo_candidates_align_build(h, 2, jobs) == Ab.E_STATE
    ctx.candidates_stage([Cc.to_job(copy.deepcopy(streams[0]["st"]))], Sc.CAM, Sc.CELL, Sc.SEG_CELL, Sc.BOUNDARY)
    assert L.plsvo_candidates_align_build(h, 1, jobs) == Ab.E_STATE                                      # reserved for two streams


@pytest.mark.gpu
def test_an_unfetched_seed_update_refuses_the_build(P):
    """between plsvo_seeds_update (here: the diagnostic commit of constructed rows) and plsvo_seeds_update_fetch the tables' sizes are the
    device's alone: the build returns PLSVO_E_STATE; behind the fetch it goes through (the update appended rows; the selection's stand)"""
    import np_seedlist as SL
    import seedlist_cases as Sl
    from test_gpu_seedlist import N_SLOTS as SEED_SLOTS, fresh as fresh_seeds, stage as stage_seeds
    Ab = P.abi
    c = P.capi.Context(0)
    try:
        c.config_pyramids(SEED_SLOTS, Sc.CAM_T[4], Sc.CAM_T[5], 3)
        for s in range(SEED_SLOTS):
            c.build_pyramid(s, np.zeros((Sc.CAM_T[5], Sc.CAM_T[4]), np.uint8))
        L, h = c.L, c.h
        cases = Sl.batch()[4:7]
        sts, seeds = fresh_seeds(cases)
        stage_seeds(c, sts, seeds)
        c.candidates_align_reserve(2, 1, 200, 100, 1024)
        c.candidates_run([Ab.CandidateFrameJob(s["T"], s["overlap"], cur_slot=0) for s in cases])
        c.candidates_set_match([Ic.frame(s, st)[1] for s, st in zip(cases, sts)])
        c.candidates_select(**Ic.PARAMS)
        c.seeds_commit_rows([SL.rows_of(k["rows"]) for k in cases])
        keep = np.ones(400, np.uint8)
        jobs = (Ab.CandAlignJob * 3)()
        for j in jobs:
            j.active, j.cur_slot, j.pt_keep, j.seg_keep = 1, 1, keep.ctypes.data_as(Ab.c_u8_p), keep.ctypes.data_as(Ab.c_u8_p)
            j.T_f_w[:] = A.T_REF
        assert L.plsvo_candidates_align_build(h, 3, jobs) == Ab.E_STATE
        c.seeds_update_fetch()
        assert L.plsvo_candidates_align_build(h, 3, jobs) == Ab.OK
        assert sum(r["n_pts"] + r["n_seg"] for r in c.candidates_align_fetch()) > 0
    finally:
        c.close()
