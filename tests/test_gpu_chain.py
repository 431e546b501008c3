"""The resident frame step (plsvo_chain_stage / _run / _fetch, plsvo_frame_step_batch) on the directed batches of tests/chain_cases.py:
the glue kernels of pl-svo_amd/csrc/chain_kernels.hip -- chain_pose_kernel, chain_active_kernel, chain_select_kernel with its wave
compaction, pack_pose_records_kernel -- and the staging / readback around them, held to tests/np_chain.py.

EXACT LAYER (nothing depends on a float tie).  A step run with poseopt_n_iter = 0 hands back the pose it composed on the device
(poseopt_kernels.hip: T0 is stored and no iteration runs, iters == 0).  With the frame table [T_kf_w, that pose] the per-call
plsvo_reproject and plsvo_match_direct must reproduce the step's found / px / search_level bit for bit on the candidates the NumPy
active rule keeps; on the rest found == 0 and px is the projection itself.  The selection must equal np_chain on those arrays for
every limit, every case and every stream, and the rule must change no match result.

POSE-OPTIMISER INPUT.  np_chain.features of the fetched px / search_level / selection, with T0 = the composed pose, run through the
per-call plsvo_poseopt_* must give the step's pt_keep, seg_keep, num_obs_pt, num_obs_ls and iters, and its pose within POSE_BAR: the
bar tests/test_sequence.py::test_hip_resident_chain_equals_the_per_call_chain holds this very pair to.  It is not zero because
chain_kernels.hip is compiled with fma contraction, so a bearing's norm may round differently from NumPy's.  Largest difference seen
over all runs of this file: none at all on the host-emulated build (no contraction there); 4.7e-16 rad and 2.9e-15 on the MI355X,
four orders of magnitude inside the bar."""
import numpy as np
import pytest

import chain_cases as CC
import np_chain

pytestmark = pytest.mark.gpu

POSE_BAR = 1e-11


def run(ctx, jobs, case, **kw):
    return ctx.frame_step_batch(jobs, case["cam"], n_pyr_levels=case["n_pyr_levels"], **kw)


def exact_layer(P, ctx, case, cell_size):
    """loads the case, runs it once without iterations and without the rule, and holds it to the per-call entry points.  Returns
    (jobs, that run's results, per stream the per-call arrays + `T_k`)"""
    syn = P.synth
    CC.load_frames(ctx, case)
    jobs = CC.chain_jobs(P, case)
    r0 = run(ctx, jobs, case, cell_size=cell_size, cell_rule=False, poseopt_n_iter=0)
    pcs = []
    for s, (r, st) in enumerate(zip(r0, case["streams"])):
        n_pt, n_seg = st["n_pt"], st["n_seg"]
        assert r.pose.iters == 0, s
        T_k = r.pose.T.copy()
        ang, dist = syn.se3_log_angle_dist(T_k, syn.se3_mul(r.align.T, np.asarray(st["T_prev_w"], float)))      # chain_pose_kernel: T_cur_from_ref * T_prev_w
        assert ang < 1e-12 and dist < 1e-12, (s, ang, dist)
        pc = CC.per_call(P, ctx, case, s, T_k, cell_size)
        a = pc["active"]
        assert np.array_equal(r.found[a], pc["found"][a]), s
        assert np.array_equal(r.px[a], pc["px_cur"][a]), s
        assert np.array_equal(r.search_level[a], pc["search_level"][a]), s
        assert not r.found[~a].any() and np.array_equal(r.px[~a], pc["px"][~a]), s
        assert np.array_equal(r.sel_pt, np_chain.select_points(r.found, a, pc["cell"], n_pt)), s
        assert np.array_equal(r.sel_seg, np_chain.select_segments(r.found, a, pc["px"], n_pt, n_seg)), s
        pc["T_k"] = T_k
        pcs.append(pc)
    return jobs, r0, pcs


def same_matches(results, r0):
    for s, (r, b) in enumerate(zip(results, r0)):
        assert np.array_equal(r.found, b.found) and np.array_equal(r.px, b.px) and np.array_equal(r.search_level, b.search_level), s
        assert np.array_equal(r.align.T, b.align.T), s


def follows_the_rule(case, results, pcs, g, max_fts, max_fts_segs):
    for s, (r, pc, st) in enumerate(zip(results, pcs, case["streams"])):
        n_pt, n_seg = st["n_pt"], st["n_seg"]
        e_pt = np_chain.select_points(r.found, pc["active"], pc["cell"], n_pt, g["cell_order"], max_fts, g["n_cells"])
        assert np.array_equal(r.sel_pt, e_pt), (s, max_fts, r.sel_pt[:8], e_pt[:8], len(r.sel_pt), len(e_pt))
        if g["seg_cell_size"] > 0:
            e_seg = np_chain.select_segments(r.found, pc["active"], pc["px"], n_pt, n_seg, g["seg_cell_size"], g["seg_n_cols"], g["seg_cell_order"], max_fts_segs, g["seg_n_cells"])
        else:
            e_seg = np_chain.select_segments(r.found, pc["active"], pc["px"], n_pt, n_seg)
        assert np.array_equal(r.sel_seg, e_seg), (s, max_fts_segs, r.sel_seg, e_seg)


worst = dict(ang=0.0, dist=0.0)


def pose_input(P, ctx, case, results, pcs, n_iter=10, reproj_thresh=2.0):
    """the step's pose against the per-call pose optimiser on np_chain.features of the step's own matches and selection"""
    abi, cam = P.abi, case["cam"]
    jobs = []
    for r, pc, st in zip(results, pcs, case["streams"]):
        f = np_chain.features(cam, r.px, r.search_level, st["pos"], st["n_pt"], st["n_seg"], r.sel_pt, r.sel_seg)
        jobs.append(abi.PoseOptJob(pc["T_k"], abs(cam[0]), reproj_thresh, n_iter, f["pt_f"], f["pt_pos"], f["pt_level"], f["seg_line"], f["seg_spos"], f["seg_epos"], f["seg_level"]))
    for s, (r, p) in enumerate(zip(results, ctx.pose_optimize_batch(jobs))):
        assert len(r.pose.pt_keep) == len(r.sel_pt) and len(r.pose.seg_keep) == len(r.sel_seg), s
        assert np.array_equal(r.pose.pt_keep, p.pt_keep) and np.array_equal(r.pose.seg_keep, p.seg_keep), s
        assert (r.pose.num_obs_pt, r.pose.num_obs_ls, r.pose.iters, r.pose.status) == (p.num_obs_pt, p.num_obs_ls, p.iters, p.status), s
        ang, dist = P.synth.se3_log_angle_dist(r.pose.T, p.T)
        worst["ang"], worst["dist"] = max(worst["ang"], ang), max(worst["dist"], dist)
        print(f"chain vs per-call pose, stream {s}: {ang:.3e} rad {dist:.3e}  (largest so far {worst['ang']:.3e} {worst['dist']:.3e})")
        assert ang < POSE_BAR and dist < POSE_BAR, (s, ang, dist)


@pytest.mark.parametrize("cell_size", [20, 10])
def test_many_cell_selection_stops_at_every_place_of_the_chunks(P, gpu_ctx, cell_size):
    """192 point cells (three chunks) / 768 (twelve chunks, three trips of the 256-stride loops), 88 segment cells (two chunks), 300
    points (a second trip of the vote loop): the stop at the first winner, on the last winner of chunk 0, on the first of chunk 1, inside
    the last chunk, on the last winner overall, beyond the winners -- limits from the device's own winners"""
    case = CC.many_cell(P)
    st = case["streams"][0]
    jobs, r0, pcs = exact_layer(P, gpu_ctx, case, cell_size)
    g = CC.grid(case, cell_size, 30, order_seed=cell_size)
    dev = dict(pcs[0], found=r0[0].found)
    pos_pt, pos_seg = CC.winning_positions(dev, st, g), CC.winning_positions(dev, st, g, True)
    (lim_pt, where_pt), (lim_seg, where_seg) = CC.stop_limits(pos_pt, g["n_cells"]), CC.stop_limits(pos_seg, g["seg_n_cells"])
    last = (g["n_cells"] - 1) // 64
    assert where_pt == dict(first_winner=0, chunk0_last=0, chunk1_first=1, last_chunk_inside=last, last_winner=last, beyond=None)
    assert where_seg == dict(first_winner=0, chunk0_last=0, chunk1_first=1, last_chunk_inside=1, last_winner=1, beyond=None)
    assert set(pos_pt // 64) == set(range(last + 1)) and last + 1 == (3 if cell_size == 20 else 12)
    free = run(gpu_ctx, jobs, case, cell_size=cell_size, cell_rule=False)
    same_matches(free, r0)
    follows_the_rule(case, free, pcs, dict(g, n_cells=None, seg_cell_size=0), None, None)
    pose_input(P, gpu_ctx, case, free, pcs)
    twice = 0
    for kind in CC.STOP_KINDS:
        res = run(gpu_ctx, jobs, case, **CC.rule_kwargs(g, lim_pt[kind], lim_seg[kind]))
        same_matches(res, r0)                                                       # the rule selects, it does not change the matching
        follows_the_rule(case, res, pcs, g, lim_pt[kind], lim_seg[kind])
        assert len(res[0].sel_pt) == min(lim_pt[kind] + 1, len(pos_pt)) and len(res[0].sel_seg) == min(lim_seg[kind] + 1, len(pos_seg)), kind
        twice = max(twice, len(res[0].sel_seg) - len(set(res[0].sel_seg.tolist())))
        pose_input(P, gpu_ctx, case, res, pcs)
    assert twice >= 3                                                               # segments that won both of their cells: a feature twice


def test_border_candidates_follow_the_in_frame_rule_for_both_ends(P, gpu_ctx):
    """candidates up to 16 px on either side of the 8-pixel border on all four sides; segments with the start, the end, both ends out of
    frame; segments in frame with one end masked; candidates behind the camera"""
    case = CC.border(P)
    st, kinds = case["streams"][0], case["kinds"]
    n_pt, n_seg = st["n_pt"], st["n_seg"]
    jobs, r0, pcs = exact_layer(P, gpu_ctx, case, 40)
    cell, act = pcs[0]["cell"], pcs[0]["active"]
    b = kinds["border_pts"]
    assert (cell[b] < 0).sum() >= 4 and (cell[b] >= 0).sum() >= 4
    s_in, e_in = cell[n_pt:n_pt + n_seg] >= 0, cell[n_pt + n_seg:] >= 0
    assert (~s_in & e_in)[kinds["seg_start_out"]].all() and (s_in & ~e_in)[kinds["seg_end_out"]].all() and (~s_in & ~e_in)[kinds["seg_both_out"]].all()
    assert (s_in & e_in)[kinds["seg_start_masked"]].all() and (s_in & e_in)[kinds["seg_end_masked"]].all()
    dropped = np.concatenate([kinds[k] for k in ("seg_start_out", "seg_end_out", "seg_both_out", "seg_start_masked", "seg_end_masked")])
    assert not r0[0].found[n_pt + dropped].any() and not r0[0].found[n_pt + n_seg + dropped].any()
    assert not np.isin(r0[0].sel_seg, dropped).any()
    # ... although one end alone matches when it is asked for on its own (the per-call matcher knows no segments)
    alone = pcs[0]["found"]
    assert alone[n_pt + n_seg + kinds["seg_start_out"]].any() and alone[n_pt + kinds["seg_end_out"]].any()
    assert alone[n_pt + n_seg + kinds["seg_start_masked"]].any() and alone[n_pt + kinds["seg_end_masked"]].any()
    assert (cell[kinds["behind_pts"]] >= 0).all() and act[n_pt + kinds["behind_seg"]].all()
    free = run(gpu_ctx, jobs, case, cell_size=40, cell_rule=False)
    same_matches(free, r0)
    pose_input(P, gpu_ctx, case, free, pcs)
    g = CC.grid(case, 40, 60, order_seed=6)
    res = run(gpu_ctx, jobs, case, **CC.rule_kwargs(g, 500, 500))
    same_matches(res, r0)
    follows_the_rule(case, res, pcs, g, 500, 500)
    pose_input(P, gpu_ctx, case, res, pcs)


def test_keyframe_apart_from_the_previous_frame_with_levels_and_edgelets(P, gpu_ctx):
    """three slots, T_prev_w != T_kf_w, a zoom that brings search levels 1 and 2, ref_level 0..3, edgelets among the points, and
    ref_type / ref_grad entries beyond the points that must not be read"""
    case = CC.zoom(P)
    st = case["streams"][0]
    n_pt, n_seg = st["n_pt"], st["n_seg"]
    jobs, r0, pcs = exact_layer(P, gpu_ctx, case, 30)
    r = r0[0]
    ok, lv = r.found, r.search_level
    assert (lv[ok] == 1).sum() >= 5 and (lv[ok] == 2).sum() >= 5 and (ok[:n_pt] & (st["ref_type"][:n_pt] == 1)).sum() >= 3
    differ = [int(s) for s in r.sel_seg if lv[n_pt + s] != lv[n_pt + n_seg + s]]
    assert differ, "no selected segment whose end points take different search levels"
    free = run(gpu_ctx, jobs, case, cell_size=30, cell_rule=False)
    same_matches(free, r0)
    pose_input(P, gpu_ctx, case, free, pcs)
    g = CC.grid(case, 30, 40, order_seed=7)
    for max_fts, max_segs in ((500, 500), (12, 2)):
        res = run(gpu_ctx, jobs, case, **CC.rule_kwargs(g, max_fts, max_segs))
        same_matches(res, r0)
        follows_the_rule(case, res, pcs, g, max_fts, max_segs)
        pose_input(P, gpu_ctx, case, res, pcs)
    assert set(differ) & set(res[0].sel_seg.tolist()) or set(differ) & set(free[0].sel_seg.tolist())


def check_records(P, ctx, case, results, pcs):
    abi = P.abi
    recs = ctx.fetch_pose_records(len(results))
    for s, (r, pc, st) in enumerate(zip(results, pcs, case["streams"])):
        n_pt, n_seg = st["n_pt"], st["n_seg"]
        assert np.array_equal(recs[s]["T_f_w"], r.pose.T) and int(recs[s]["n_tracked"]) == int(r.align.n_tracked) > 0, s
        assert (int(recs[s]["num_obs_pt"]), int(recs[s]["num_obs_ls"]), int(recs[s]["stream"])) == (r.pose.num_obs_pt, r.pose.num_obs_ls, s), s
        assert float(recs[s]["error_final"]) == r.pose.error_final, s
        empty = len(r.sel_pt) + len(r.sel_seg) == 0
        assert int(recs[s]["status"]) == (abi.REC_ALIGN | abi.REC_POSEOPT | (abi.REC_POSEOPT_EMPTY if empty else 0)), (s, int(recs[s]["status"]))
        if empty:
            assert np.array_equal(r.pose.T, pc["T_k"]) and (r.pose.num_obs_pt, r.pose.num_obs_ls) == (0, 0), s
        # the active rule's counts: what the matcher was asked for, and what of it became a match
        a = pc["active"]
        assert int(r.found.sum()) == int((pc["found"] & a).sum()) and int(r.found[:n_pt].sum()) == int((pc["found"] & a)[:n_pt].sum()), s
    return recs


def test_mixed_batch_keeps_every_stream_in_its_own_rows(P, gpu_ctx):
    """six streams of different sizes in one plsvo_frame_step_batch with a segment grid (the segment rows of the pose optimiser's input
    are doubled): full, no points, no segments, no candidates at all, everything masked out, more than 256 points"""
    case = CC.mixed(P)
    names = case["names"]
    jobs, r0, pcs = exact_layer(P, gpu_ctx, case, 20)
    nothing = {names.index("no_candidates"), names.index("all_masked")}
    free = run(gpu_ctx, jobs, case, cell_size=20, cell_rule=False)
    check_records(P, gpu_ctx, case, free, pcs)
    same_matches(free, r0)
    pose_input(P, gpu_ctx, case, free, pcs)
    g = CC.grid(case, 20, 30, order_seed=3)
    for max_fts, max_segs in ((500, 500), (20, 3)):
        res = run(gpu_ctx, jobs, case, **CC.rule_kwargs(g, max_fts, max_segs))
        recs = check_records(P, gpu_ctx, case, res, pcs)
        assert {s for s in range(len(res)) if int(recs[s]["status"]) & P.abi.REC_POSEOPT_EMPTY} == nothing
        same_matches(res, r0)
        follows_the_rule(case, res, pcs, g, max_fts, max_segs)
        pose_input(P, gpu_ctx, case, res, pcs)
    for s, name in enumerate(names):        # (the limits of the last run bite on the streams that have enough winners)
        want_pt = 0 if name in ("no_points", "no_candidates", "all_masked") else 21
        want_seg = 0 if name in ("no_segments", "no_candidates", "all_masked") else 4
        assert (len(res[s].sel_pt), len(res[s].sel_seg)) == (want_pt, want_seg), name
    assert len(res[names.index("many_points")].pose.pt_keep) == 21


def test_selection_at_the_edge_of_its_lds(P, gpu_ctx):
    """12288 + 2596 cells: 59536 of the 60000 bytes of dynamic LDS the guard of plsvo_chain_stage allows; a finer grid is refused with
    PLSVO_E_CAPACITY, leaves no staged step behind, and the context goes on working"""
    abi = P.abi
    case = CC.lds_edge(P)
    jobs, r0, pcs = exact_layer(P, gpu_ctx, case, CC.LDS_GRID[0])
    g = CC.grid(case, *CC.LDS_GRID, order_seed=9)
    assert (g["n_cells"] + g["seg_n_cells"]) * 4 == 59536
    res = run(gpu_ctx, jobs, case, **CC.rule_kwargs(g, 5000, 5000))
    same_matches(res, r0)
    follows_the_rule(case, res, pcs, g, 5000, 5000)
    assert len(res[0].sel_pt) > 60 and len(res[0].sel_seg) > 8
    pose_input(P, gpu_ctx, case, res, pcs)
    for cell_size, seg_cell_size in CC.LDS_REFUSED:
        with pytest.raises(P.capi.PlsvoError) as e:
            gpu_ctx.chain_stage(jobs, case["cam"], n_pyr_levels=3, cell_size=cell_size, cell_rule=True, max_fts=5000, seg_cell_size=seg_cell_size, max_fts_segs=5000)
        assert e.value.code == abi.E_CAPACITY, (cell_size, seg_cell_size)
        with pytest.raises(P.capi.PlsvoError) as e:        # refused before anything was staged for launch
            gpu_ctx.chain_run()
        assert e.value.code == abi.E_STATE
    # without the rule the selection needs no LDS: the finest of the refused grids is fine
    again = run(gpu_ctx, jobs, case, cell_size=CC.LDS_REFUSED[0][0], cell_rule=False)
    assert np.array_equal(again[0].found, r0[0].found) and np.array_equal(again[0].px, r0[0].px)
    res2 = run(gpu_ctx, jobs, case, **CC.rule_kwargs(g, 5000, 5000))
    assert np.array_equal(res2[0].sel_pt, res[0].sel_pt) and np.array_equal(res2[0].sel_seg, res[0].sel_seg) and np.array_equal(res2[0].pose.T, res[0].pose.T)
