"""The cell selection of the map candidates on the device (plsvo_candidates_select ..; pl-svo_amd/csrc/select_device.hpp) against its
restatement tests/np_select.py on the cases of tests/select_cases.py.  Everything is compared byte for byte: the stage has no
transcendental call and copies the matcher's own pixels.  The directed cases drive the kernel with constructed match results
(plsvo_candidates_set_match); the pose optimiser's test runs the real matcher on textured frames."""
import copy
import ctypes as C

import numpy as np
import pytest

import candidates_cases as Cc
import np_candidates as N
import np_select as S
import select_cases as Sc
from test_gpu_candidates import _texture

CAND_FIELDS = ("pt_lm", "pt_px", "pt_cell", "pt_obs", "pt_has_view", "pt_active", "seg_lm", "seg_px", "seg_cell", "seg_obs", "seg_has_view", "seg_active", "kf_count")
SEL_FIELDS = ("pt_lm", "pt_px", "pt_level", "pt_type", "pt_grad", "seg_lm", "seg_px", "seg_level")


@pytest.fixture(scope="module")
def ctx(P):
    """a context of its own: the matcher's diagnostic view (for A_cur_ref) wants pyramids of the small camera's size"""
    c = P.capi.Context(0)
    c.config_pyramids(4, Sc.CAM_T[4], Sc.CAM_T[5], 3)
    for s in range(4):
        c.build_pyramid(s, np.zeros((Sc.CAM_T[5], Sc.CAM_T[4]), np.uint8))
    yield c
    c.close()


def same_bytes(got, want, tag):
    g = np.asarray(got)
    w = np.asarray(want, dtype=g.dtype).reshape(g.shape if g.size else (-1,) + g.shape[1:])
    assert g.shape == w.shape and g.tobytes() == w.tobytes(), (tag, g, w)


def stage(ctx, streams, sts):
    ctx.candidates_stage([Cc.to_job(st) for st in sts], Sc.CAM, Sc.CELL, Sc.SEG_CELL, Sc.BOUNDARY)
    ctx.candidates_set_quality([dict(pt_n_failed=st["pt_nfail"], pt_n_succeeded=st["pt_nsucc"], seg_n_failed=st["seg_nfail"], seg_n_succeeded=st["seg_nsucc"]) for st in sts])


def device_A(ctx, P, st, T, r):
    """Matcher::A_cur_ref_ of the filed points whose reference observation is an edgelet, from the matcher's own diagnostic view"""
    rows = [(i, st["pt_obs"][lm][o]) for i, (lm, o) in enumerate(zip(r["pt_lm"], r["pt_obs"])) if o >= 0 and st["pt_obs"][lm][o]["type"] == 1]
    if not rows:
        return {}
    n_kf = len(st["kf_T"])
    job = P.abi.MatchJob(Sc.CAM, list(st["kf_T"]) + [T], [0] * (n_kf + 1), [n_kf] * len(rows), [ob["kf"] for _, ob in rows], [ob["px"] for _, ob in rows],
                         [ob["f"] for _, ob in rows], [ob["level"] for _, ob in rows], [1] * len(rows), [ob["grad"] for _, ob in rows],
                         [st["pt_pos"][r["pt_lm"][i]] for i, _ in rows], [r["pt_px"][i] for i, _ in rows], n_pyr_levels=3, align_max_iter=10)
    w = ctx.match_warp_patches(job, fields=("A", "search_level"))
    assert np.all(w["search_level"] >= 0)                              # none rejected by the border test: A is the warp's
    return {i: [float(v) for v in w["A"][k]] for k, (i, _) in enumerate(rows)}


def frame(ctx, P, streams, sts, params, Ts=None, tag=""):
    """one frame on the device and in the restatement (which mutates sts): candidates -> constructed match -> selection, all compared"""
    Ts = [s["T"] for s in streams] if Ts is None else Ts
    ctx.candidates_run([P.abi.CandidateFrameJob(T, s["overlap"], cur_slot=0) for s, T in zip(streams, Ts)])
    got_c = ctx.candidates_fetch()
    want_c = [N.candidates(st, T, s["overlap"], Sc.CAM_T, Sc.CELL, Sc.SEG_CELL, Sc.BOUNDARY) for s, st, T in zip(streams, sts, Ts)]
    for k, (g, w) in enumerate(zip(got_c, want_c)):
        assert (g["n_filed_pt"], g["n_filed_seg"]) == (w["n_filed_pt"], w["n_filed_seg"]), (tag, k)
        for f in CAND_FIELDS:
            same_bytes(g[f], w[f], (tag, "candidates", k, f))
        for f in ("pt_cand_failed", "seg_cand_failed"):               # the lists may have closed up since they were staged
            same_bytes(g[f][:len(w[f])], w[f], (tag, "candidates", k, f))
    matches = [Sc.match_of(s, r) for s, r in zip(streams, want_c)]
    ctx.candidates_set_match(matches)
    ctx.candidates_select(**params)
    got = ctx.candidates_select_fetch()
    quality = ctx.candidates_fetch_quality()
    want = []
    for k, (s, st, T, r, m) in enumerate(zip(streams, sts, Ts, want_c, matches)):
        A = device_A(ctx, P, st, T, r)
        w = S.select(st, r, m, Sc.CAM_T, Sc.CELL, Sc.SEG_CELL, params["max_fts"], params["max_fts_segs"], params["cell_order"], params["seg_cell_order"], A=A)
        want.append(w)
        g, q = got[k], quality[k]
        assert (g["n_matches"], g["n_ls_matches"], g["n_trials"]) == (w["n_matches"], w["n_ls_matches"], w["n_trials"]), (tag, k)
        for f in SEL_FIELDS:
            same_bytes(g[f], w[f], (tag, "select", k, f))
        for f, key in (("pt_n_failed", "pt_nfail"), ("pt_n_succeeded", "pt_nsucc"), ("pt_type", "pt_type"), ("seg_n_failed", "seg_nfail"), ("seg_n_succeeded", "seg_nsucc"),
                       ("seg_type", "seg_type"), ("pt_cand", "pt_cand"), ("seg_cand", "seg_cand")):
            same_bytes(q[f], st[key], (tag, "quality", k, f))
        same_bytes(q["pt_event"], w["pt_event"], (tag, "quality", k, "pt_event"))
        same_bytes(q["seg_event"], w["seg_event"], (tag, "quality", k, "seg_event"))
    return got, quality, want


@pytest.mark.gpu
@pytest.mark.parametrize("params", sorted(Sc.PARAMS))
def test_selection_equals_the_restatement_over_two_frames(ctx, P, params):
    """the batch of ten unequal streams; the second frame runs on the tables the first one left: its candidates equal np_candidates on
    the restatement's mutated map (a promoted type re-orders a cell, a deleted landmark is gone from the keyframe lists, an erased candidate
    from its list), and its selection starts from the first frame's counters"""
    streams = Sc.batch()
    sts = [copy.deepcopy(s["st"]) for s in streams]
    stage(ctx, streams, sts)
    p = Sc.PARAMS[params]
    _, q1, w1 = frame(ctx, P, streams, sts, p, tag=(params, 1))
    assert any(e for w in w1 for e in w["pt_event"] + w["seg_event"])
    assert any(len(st[f]) < len(s["st"][f]) for s, st in zip(streams, sts) for f in ("pt_cand", "seg_cand"))
    if params == "default":
        assert any(st["kf_pt"] != s["st"]["kf_pt"] for s, st in zip(streams, sts)) and any(st["kf_seg"] != s["st"]["kf_seg"] for s, st in zip(streams, sts))
        assert any(1 in w["pt_event"] for w in w1) and any(1 in w["seg_event"] for w in w1)
    rng = np.random.default_rng(77)
    T2 = [[float(v) for v in P.synth.se3_exp(np.concatenate([rng.uniform(-0.02, 0.02, 3), rng.uniform(-0.01, 0.01, 3)]))] if s["names"] else s["T"] for s in streams]
    frame(ctx, P, streams, sts, p, Ts=T2, tag=(params, 2))


@pytest.mark.gpu
def test_one_stream_at_a_time_equals_its_place_in_the_batch(ctx, P):
    streams = Sc.batch()
    p = Sc.PARAMS["shuffled"]
    sts = [copy.deepcopy(s["st"]) for s in streams]
    stage(ctx, streams, sts)
    got, quality, _ = frame(ctx, P, streams, sts, p, tag="batch")
    for k in (0, 3, 6, 8):
        one = [copy.deepcopy(streams[k]["st"])]
        stage(ctx, streams[k:k + 1], one)
        g, q, _ = frame(ctx, P, streams[k:k + 1], one, p, tag=("alone", k))
        for f in g[0]:
            same_bytes(g[0][f], got[k][f], ("alone", k, f))
        for f in q[0]:
            same_bytes(q[0][f], quality[k][f], ("alone", k, f))


@pytest.mark.gpu
def test_quality_is_zero_after_staging_and_set_quality_leaves_the_rest(ctx, P):
    streams = Sc.batch()[5:6]
    st = copy.deepcopy(streams[0]["st"])
    ctx.candidates_stage([Cc.to_job(st)], Sc.CAM, Sc.CELL, Sc.SEG_CELL, Sc.BOUNDARY)
    q = ctx.candidates_fetch_quality()[0]
    assert not q["pt_n_failed"].any() and not q["pt_n_succeeded"].any() and not q["pt_event"].any() and not q["seg_event"].any()
    same_bytes(q["pt_type"], st["pt_type"], "types"); same_bytes(q["pt_cand"], st["pt_cand"], "list")
    ctx.candidates_set_quality([dict(pt_n_failed=st["pt_nfail"])])
    q = ctx.candidates_fetch_quality()[0]
    same_bytes(q["pt_n_failed"], st["pt_nfail"], "set")
    assert not q["pt_n_succeeded"].any() and not q["seg_n_failed"].any()


@pytest.mark.gpu
def test_select_error_paths(ctx, P):
    L, h, A = ctx.L, ctx.h, P.abi
    streams = Sc.batch()[:3]
    sts = [copy.deepcopy(s["st"]) for s in streams]
    stage(ctx, streams, sts)
    pr = A.CandSelectParams()
    pr.max_fts, pr.max_fts_segs, pr.poseopt_n_iter, pr.reproj_thresh = 120, 100, 10, 2.0
    # no run, no match: state errors
    assert L.plsvo_candidates_select(h, C.byref(pr)) == A.E_STATE
    assert L.plsvo_candidates_select_fetch(h, 3, (A.CandSelectOut * 3)()) == A.E_STATE
    assert L.plsvo_candidates_pose_optimize(h) == A.E_STATE and L.plsvo_candidates_pose_fetch(h, 3, (A.PoseOptOut * 3)()) == A.E_STATE
    assert L.plsvo_candidates_set_match(h, 3, (A.CandMatchOut * 3)()) == A.E_STATE
    ctx.candidates_run([A.CandidateFrameJob(s["T"], s["overlap"], cur_slot=0) for s in streams])
    assert L.plsvo_candidates_select(h, C.byref(pr)) == A.E_STATE                      # run, but no match
    want_c = [Sc.restate_candidates(s, st) for s, st in zip(streams, sts)]
    assert L.plsvo_candidates_set_match(h, 2, (A.CandMatchOut * 3)()) == A.E_INVALID and L.plsvo_candidates_set_match(h, 3, None) == A.E_INVALID
    assert L.plsvo_candidates_set_match(h, 3, (A.CandMatchOut * 3)()) == A.E_INVALID   # null arrays
    ctx.candidates_set_match([Sc.match_of(s, r) for s, r in zip(streams, want_c)])
    before = ctx.candidates_fetch_quality()
    # bad parameters: nothing is written
    assert L.plsvo_candidates_select(h, None) == A.E_INVALID
    for field in ("max_fts", "max_fts_segs", "poseopt_n_iter"):
        p2 = A.CandSelectParams.from_buffer_copy(pr)
        setattr(p2, field, -1)
        assert L.plsvo_candidates_select(h, C.byref(p2)) == A.E_INVALID, field
    for field, n in (("cell_order", Sc.N_CELLS), ("seg_cell_order", Sc.SEG_N_CELLS)):
        for bad in ([0] * n, list(range(1, n + 1)), [-1] + list(range(1, n)), list(range(n - 2)) + [n - 3, n - 1]):
            o = np.array(bad, np.int32)
            p2 = A.CandSelectParams.from_buffer_copy(pr)
            setattr(p2, field, o.ctypes.data_as(A.c_i32_p))
            assert L.plsvo_candidates_select(h, C.byref(p2)) == A.E_INVALID, (field, bad[:3])
    assert L.plsvo_candidates_set_quality(h, 2, (A.CandQualityIn * 3)()) == A.E_INVALID and L.plsvo_candidates_fetch_quality(h, 3, None) == A.E_INVALID
    neg = np.full(len(sts[0]["pt_nfail"]), -1, np.int32)
    qi = (A.CandQualityIn * 3)()
    qi[0].pt_n_failed = neg.ctypes.data_as(A.c_i32_p)
    assert L.plsvo_candidates_set_quality(h, 3, qi) == A.E_INVALID
    after = ctx.candidates_fetch_quality()
    for a, b in zip(before, after):
        for f in a:
            same_bytes(a[f], b[f], ("unchanged", f))
    # the selection itself, once; a second one on the same run is refused (the tables have moved on)
    ctx.candidates_select(**Sc.PARAMS["default"])
    assert L.plsvo_candidates_select(h, C.byref(pr)) == A.E_STATE
    assert L.plsvo_candidates_select_fetch(h, 2, (A.CandSelectOut * 3)()) == A.E_INVALID and L.plsvo_candidates_select_fetch(h, 3, None) == A.E_INVALID
    assert L.plsvo_candidates_pose_fetch(h, 3, (A.PoseOptOut * 3)()) == A.E_STATE and not ctx.candidates_poses_dev()
    got = ctx.candidates_select_fetch()
    for k, (s, st, r) in enumerate(zip(streams, sts, want_c)):
        w = S.select(st, r, Sc.match_of(s, r), Sc.CAM_T, Sc.CELL, Sc.SEG_CELL, 120, 100, A=device_A(ctx, P, st, s["T"], r))
        assert (got[k]["n_matches"], got[k]["n_ls_matches"], got[k]["n_trials"]) == (w["n_matches"], w["n_ls_matches"], w["n_trials"])


def _bearing(px, cam):
    x, y = (px[..., 0] - cam[2]) / cam[0], (px[..., 1] - cam[3]) / cam[1]
    n = np.sqrt((x * x + y * y) + 1.0)
    return np.stack([x / n, y / n, 1.0 / n], -1)


def check_pose(ctx, P, sts, Ts, cam, sel, got):
    """plsvo_pose_optimize on host arrays built from the fetched selection against the resident result `got`"""
    jobs = []
    for st, T, s in zip(sts, Ts, sel):
        pt_f = _bearing(s["pt_px"], cam) if s["n_matches"] else np.zeros((0, 3))
        if s["n_ls_matches"]:
            sf, ef = _bearing(s["seg_px"][:, 0:2], cam), _bearing(s["seg_px"][:, 2:4], cam)
            l = np.stack([sf[:, 1] * ef[:, 2] - sf[:, 2] * ef[:, 1], sf[:, 2] * ef[:, 0] - sf[:, 0] * ef[:, 2], sf[:, 0] * ef[:, 1] - sf[:, 1] * ef[:, 0]], -1)
            line = l / np.sqrt(l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1])[:, None]
        else:
            line = np.zeros((0, 3))
        jobs.append(P.abi.PoseOptJob(T, abs(cam[0]), 2.0, 10, pt_f, np.array(st["pt_pos"]).reshape(-1, 3)[s["pt_lm"]], np.maximum(s["pt_level"], 0), line,
                                     np.array(st["seg_spos"]).reshape(-1, 3)[s["seg_lm"]], np.array(st["seg_epos"]).reshape(-1, 3)[s["seg_lm"]], np.maximum(s["seg_level"], 0)))
    want = ctx.pose_optimize_batch(jobs)
    n_feat = n_iters = 0
    for k, (g, w) in enumerate(zip(got, want)):
        for f in ("T", "cov", "pt_keep", "seg_keep"):
            same_bytes(getattr(g, f), getattr(w, f), (k, f))
        for f in ("estimated_scale", "error_init", "error_final", "num_obs_pt", "num_obs_ls", "iters", "status"):
            assert np.float64(getattr(g, f)).tobytes() == np.float64(getattr(w, f)).tobytes(), (k, f, getattr(g, f), getattr(w, f))
        n_feat += sel[k]["n_matches"] + sel[k]["n_ls_matches"]
        n_iters += g.iters
    return n_feat, n_iters


@pytest.mark.gpu
def test_the_resident_pose_optimiser_on_the_directed_batch(ctx, P):
    """the constructed matches of the batch: points and segments (one of them twice), an empty stream -- the device-written bearings, line
    equations, positions, levels and jobs give what plsvo_pose_optimize gives on host arrays built from the fetched selection; the poses
    on the device are the fetched ones"""
    streams = Sc.batch()
    sts = [copy.deepcopy(s["st"]) for s in streams]
    stage(ctx, streams, sts)
    sel, _, _ = frame(ctx, P, streams, sts, Sc.PARAMS["default"], tag="pose")
    ctx.candidates_pose_optimize()
    got = ctx.candidates_pose_fetch([(s["n_matches"], s["n_ls_matches"]) for s in sel])
    assert ctx.candidates_poses_dev()
    n_feat, n_iters = check_pose(ctx, P, [s["st"] for s in streams], [s["T"] for s in streams], Sc.CAM_T, sel, got)
    assert sum(s["n_ls_matches"] for s in sel) > 10 and sum(s["n_matches"] for s in sel) >= 40 and n_iters > 0
    assert got[4].status & 1 and sel[4]["n_matches"] == 0          # the empty stream: optimizeGaussNewton returns early


@pytest.mark.gpu
def test_the_resident_pose_optimiser_equals_plsvo_pose_optimize_on_the_fetched_selection(P):
    """the real matcher on textured frames (the setup of the candidates' own match test), the selection, then the pose optimiser on the
    features the selection wrote on the device: pose, covariance, keep masks and the medians equal plsvo_pose_optimize on host arrays
    built from the FETCHED selection -- bearings, line equations and positions restated here in float64.  (These streams list a landmark
    both as a candidate and in a keyframe, outside the selection's preconditions: only the features and the poses are looked at.)"""
    case = Cc.edge_batch_case()
    ctx = P.capi.Context(0)
    try:
        n_slots = max(len(st["kf_T"]) for st in case["streams"]) + 1
        ctx.config_pyramids(n_slots, 320, 240, 3)
        rng = np.random.default_rng(31)
        for s in range(n_slots):
            ctx.build_pyramid(s, _texture(rng))
        ctx.candidates_stage([Cc.to_job(st) for st in case["streams"]], Cc.CAM, Cc.CELL, Cc.SEG_CELL, Cc.BOUNDARY, n_pyr_levels=3, align_max_iter=10)
        ctx.candidates_run(Cc.frames_of(case))
        ctx.candidates_match()
        ctx.candidates_select(max_fts=120, max_fts_segs=100)
        ctx.candidates_pose_optimize()
        sel = ctx.candidates_select_fetch()
        got = ctx.candidates_pose_fetch([(s["n_matches"], s["n_ls_matches"]) for s in sel])
        poses = ctx.candidates_poses_dev()
        assert poses
        n_feat, n_iters = check_pose(ctx, P, case["streams"], case["T"], Cc.CAM_T, sel, got)
        assert n_feat >= len(sel) and n_iters > 0, (n_feat, n_iters)      # the optimiser had something to do
    finally:
        ctx.close()


@pytest.mark.gpu
def test_select_full_size_replicas(ctx, P):
    """1024 streams: 16 distinct tables x 64 replicas.  Every replica equals the first sixteen, and those equal the restatement"""
    rng = np.random.default_rng(5301)
    base = [Sc.random_stream(rng, [(60, 30)] * 4, 220, 90, 6, 4) for _ in range(16)]
    reps = 64
    streams = base * reps
    sts = [copy.deepcopy(s["st"]) for s in base]
    jobs = [Cc.to_job(st) for st in sts]
    ctx.candidates_stage(jobs * reps, Sc.CAM, Sc.CELL, Sc.SEG_CELL, Sc.BOUNDARY)
    ctx.candidates_set_quality([dict(pt_n_failed=st["pt_nfail"], pt_n_succeeded=st["pt_nsucc"], seg_n_failed=st["seg_nfail"], seg_n_succeeded=st["seg_nsucc"]) for st in sts] * reps)
    ctx.candidates_run([P.abi.CandidateFrameJob(s["T"], s["overlap"], cur_slot=0) for s in streams])
    want_c = [Sc.restate_candidates(s, st) for s, st in zip(base, sts)]
    matches = [Sc.match_of(s, r) for s, r in zip(base, want_c)]
    ctx.candidates_set_match(matches * reps)
    p = Sc.PARAMS["shuffled"]
    ctx.candidates_select(**p)
    got, quality = ctx.candidates_select_fetch(), ctx.candidates_fetch_quality()
    for k, (s, st, r, m) in enumerate(zip(base, sts, want_c, matches)):
        w = S.select(st, r, m, Sc.CAM_T, Sc.CELL, Sc.SEG_CELL, p["max_fts"], p["max_fts_segs"], p["cell_order"], p["seg_cell_order"], A=device_A(ctx, P, s["st"], s["T"], r))
        for f in SEL_FIELDS:
            same_bytes(got[k][f], w[f], ("full_size", k, f))
        same_bytes(quality[k]["pt_type"], st["pt_type"], ("full_size", k)); same_bytes(quality[k]["seg_n_failed"], st["seg_nfail"], ("full_size", k))
        assert got[k]["n_matches"] == p["max_fts"] + 1 and got[k]["n_ls_matches"] > 0
    for k in range(16, 16 * reps):
        for f in got[k]:
            same_bytes(got[k][f], got[k % 16][f], (k, f))
        for f in quality[k]:
            same_bytes(quality[k][f], quality[k % 16][f], (k, f))
