"""CPU side of the resident frame step's test kit: tests/np_chain.py (the reference's sequential selection) against an independent
brute-force statement of the same rule, and the CONDITIONS of tests/chain_cases.py -- on the oracle alone (sparse_align -> composed
pose -> reproject -> match_direct) every directed case reaches what it is named for.  The device tests of tests/test_gpu_chain.py run
the same cases; without these conditions a case could quietly stop reaching its path."""
import numpy as np

import chain_cases as CC
import np_chain


def test_sequential_selection_equals_the_brute_force_form():
    """random found / active / cell / order arrays, more cells than candidates and fewer, every limit from 0 to past the winners;
    segments that win both of their cells, and segments whose two end points share a cell"""
    rng = np.random.default_rng(12)
    twice = same_cell = 0
    for trial in range(60):
        n_pt, n_seg = int(rng.integers(0, 90)), int(rng.integers(0, 30))
        n_cols, n_rows = int(rng.integers(1, 9)), int(rng.integers(1, 7))
        n_cells, size = n_cols * n_rows, 10
        nc = n_pt + 2 * n_seg
        found, active = rng.uniform(size=nc) < 0.6, rng.uniform(size=nc) < 0.8
        px = np.stack([rng.uniform(0, n_cols * size, nc), rng.uniform(0, n_rows * size, nc)], axis=1)
        near = rng.uniform(size=n_seg) < 0.3            # short segments: both end points in one cell
        px[n_pt + n_seg:][near] = np.minimum(px[n_pt:n_pt + n_seg][near] + 0.5, [n_cols * size - 0.01, n_rows * size - 0.01])
        cell = (px[:, 1] / size).astype(int) * n_cols + (px[:, 0] / size).astype(int)
        order = rng.permutation(n_cells).astype(np.int32)
        seg_active = active.copy()
        seg_active[n_pt:n_pt + n_seg] = seg_active[n_pt + n_seg:] = active[n_pt:n_pt + n_seg] & active[n_pt + n_seg:]
        sk, ek = np_chain.segment_cells(px, n_pt, n_seg, size, n_cols)
        assert np.array_equal(sk, cell[n_pt:n_pt + n_seg]) and np.array_equal(ek, cell[n_pt + n_seg:])
        same_cell += int((sk == ek).sum())
        for limit in list(range(0, n_cells + 2)):
            a = np_chain.select_points(found, active, cell, n_pt, order, limit, n_cells)
            b = np_chain.brute_force_selection(found, active, cell, n_pt, order, limit)
            assert np.array_equal(a, b), (trial, limit, a, b)
            a = np_chain.select_segments(found, seg_active, px, n_pt, n_seg, size, n_cols, order, limit, n_cells)
            b = np_chain.brute_force_selection(found, seg_active, cell, n_pt, order, limit, n_seg, (sk, ek))
            assert np.array_equal(a, b), (trial, limit, a, b)
            assert len(a) <= limit + 1
        twice += len(a) - len(set(a.tolist()))
        # without the grids: every match of a filed candidate, in candidate order
        assert np.array_equal(np_chain.select_points(found, active, cell, n_pt), np.nonzero((found & active)[:n_pt])[0])
        both = (found & seg_active)[n_pt:n_pt + n_seg] & (found & seg_active)[n_pt + n_seg:]
        assert np.array_equal(np_chain.select_segments(found, seg_active, px, n_pt, n_seg), np.nonzero(both)[0])
    assert twice > 20 and same_cell > 20


def test_active_rule_needs_both_ends_of_a_segment():
    cell = np.array([3, -1, 5, 5, -1, 5, 5, 5, 5, -1])          # 2 points, 4 segments: starts 2..5, ends 6..9
    want = np.array([1, 1, 1, 0, 1, 1, 1, 1, 0, 1], np.uint8)
    #                 segment 0: both fine; 1: start masked; 2: start out of frame and end masked; 3: end out of frame
    assert np_chain.active_rule(want, cell, 2, 4).tolist() == [True, False, True, False, False, False, True, False, False, False]
    assert np_chain.active_rule(None, cell, 2, 4).tolist() == [True, False, True, True, False, False, True, True, False, False]


def test_features_take_the_segment_level_from_the_end_point():
    cam = (200.0, 210.0, 160.0, 120.0, 320, 240)
    px = np.array([[100.0, 50.0], [20.0, 30.0], [300.0, 200.0]])
    pos = np.arange(9.0).reshape(3, 3)
    f = np_chain.features(cam, px, np.array([-1, 1, 2]), pos, 1, 1, [0], [0, 0])
    assert f["pt_level"].tolist() == [0] and f["seg_level"].tolist() == [2, 2]
    assert np.allclose(np.linalg.norm(f["pt_f"], axis=1), 1.0) and np.allclose(np.hypot(f["seg_line"][:, 0], f["seg_line"][:, 1]), 1.0)
    sf, ef = np_chain.bearing(cam, px[1]), np_chain.bearing(cam, px[2])
    assert abs(f["seg_line"][0] @ sf) < 1e-15 and abs(f["seg_line"][0] @ ef) < 1e-15
    assert np.array_equal(f["seg_spos"], pos[[1, 1]]) and np.array_equal(f["seg_epos"], pos[[2, 2]])


# ---- conditions: each case reaches what it is named for ------------------------------------------------------------------------------

def test_many_cell_case_has_winners_in_every_chunk_and_a_stop_of_each_kind(P, ob):
    case = CC.many_cell(P)
    st = case["streams"][0]
    for cell_size, n_chunks in ((20, 3), (10, 12)):
        g = CC.grid(case, cell_size, 30, order_seed=cell_size)
        pc = CC.oracle_step(P, ob, case, 0, cell_size)
        for segments, cells in ((False, g["n_cells"]), (True, g["seg_n_cells"])):
            pos = CC.winning_positions(pc, st, g, segments)
            lim, where = CC.stop_limits(pos, cells)
            last = (cells - 1) // 64
            assert last + 1 == (2 if segments else n_chunks)
            assert set(pos // 64) == set(range(last + 1)), (cell_size, segments)                 # winners in each chunk
            assert where == dict(first_winner=0, chunk0_last=0, chunk1_first=1, last_chunk_inside=last, last_winner=last, beyond=None)
            assert lim["chunk0_last"] > 0 and lim["last_chunk_inside"] < lim["last_winner"] and len(set(lim.values())) == len(lim)
        sel = np_chain.select_segments(pc["found"], pc["active"], pc["px"], st["n_pt"], st["n_seg"], 30, g["seg_n_cols"], g["seg_cell_order"], 1000, g["seg_n_cells"])
        assert len(sel) > len(set(sel.tolist())) >= 10                                            # a segment that wins both of its cells
        assert 0 < (~pc["active"]).sum() and (pc["found"] & ~pc["active"]).sum() > 10            # the mask drops candidates that would match
    assert st["n_pt"] > 256


def test_border_case_has_every_kind_of_candidate(P, ob):
    case = CC.border(P)
    st, kinds = case["streams"][0], case["kinds"]
    n_pt, n_seg, W, H = st["n_pt"], st["n_seg"], case["W"], case["H"]
    pc = CC.oracle_step(P, ob, case, 0, 40)
    px, cell, act = pc["px"], pc["cell"], pc["active"]
    b = kinds["border_pts"]
    ix, iy = px[:, 0].astype(int), px[:, 1].astype(int)
    for side, out in enumerate((ix < 8, ix >= W - 8, iy < 8, iy >= H - 8)):
        assert (out[b] & (cell[b] < 0)).any() and (~out[b] & (cell[b] >= 0))[side::4].any(), side      # out of frame and in frame on each side
    s_in, e_in = cell[n_pt:n_pt + n_seg] >= 0, cell[n_pt + n_seg:] >= 0
    assert (~s_in & e_in)[kinds["seg_start_out"]].all() and (s_in & ~e_in)[kinds["seg_end_out"]].all() and (~s_in & ~e_in)[kinds["seg_both_out"]].all()
    for k in ("seg_start_masked", "seg_end_masked"):
        assert (s_in & e_in)[kinds[k]].all() and not act[n_pt + kinds[k]].any() and not act[n_pt + n_seg + kinds[k]].any()
    for k in ("seg_start_out", "seg_end_out", "seg_both_out"):
        assert not act[n_pt + kinds[k]].any() and not act[n_pt + n_seg + kinds[k]].any()
    # one end alone would have matched: the rule, not the matcher, keeps these segments out
    assert pc["found"][n_pt + n_seg + kinds["seg_start_out"]].any() and pc["found"][n_pt + kinds["seg_end_out"]].any()
    assert pc["found"][n_pt + n_seg + kinds["seg_start_masked"]].any() and pc["found"][n_pt + kinds["seg_end_masked"]].any()
    # behind the camera, projected into the frame all the same
    z = P.synth.se3_act(pc["T_k"], st["pos"])[:, 2]
    assert (z[kinds["behind_pts"]] < 0).all() and (cell[kinds["behind_pts"]] >= 0).all()
    assert (z[n_pt + n_seg + kinds["behind_seg"]] < 0).all() and act[n_pt + kinds["behind_seg"]].all()
    assert act[:80].all() and act.sum() > 100


def test_zoom_case_reaches_search_levels_1_and_2_and_edgelets(P, ob):
    case = CC.zoom(P)
    st = case["streams"][0]
    n_pt, n_seg = st["n_pt"], st["n_seg"]
    assert not np.array_equal(st["T_prev_w"], st["T_kf_w"]) and len({st["kf_slot"], st["cur_slot"], st["align"]["ref_slot"]}) == 3
    assert set(st["ref_level"].tolist()) == {0, 1, 2, 3} and (st["ref_type"][n_pt:] == 1).all() and np.abs(st["ref_grad"][n_pt:]).max() > 0.5
    pc = CC.oracle_step(P, ob, case, 0, 30)
    ang, dist = P.synth.se3_log_angle_dist(pc["T_k"], case["T_cur_w_true"])
    assert ang < 5e-3, (ang, dist)                                                               # the alignment prev -> new did its job
    ok = pc["found"] & pc["active"]
    lv = pc["search_level"]
    assert (lv[ok] == 1).sum() >= 5 and (lv[ok] == 2).sum() >= 5                                  # search levels 1 and 2 among the matches
    assert (ok[:n_pt] & (st["ref_type"][:n_pt] == 1)).sum() >= 3 and (ok[:n_pt] & (st["ref_type"][:n_pt] == 0)).sum() >= 3      # found edgelets
    both = ok[n_pt:n_pt + n_seg] & ok[n_pt + n_seg:]
    assert both.sum() >= 3
    # a matched segment whose two end points take different search levels: the feature's level is the END point's
    assert (both & (lv[n_pt:n_pt + n_seg] != lv[n_pt + n_seg:])).any()
    assert (~pc["active"]).sum() >= 10                                                            # the zoom pushes candidates out of the frame


def test_mixed_case_has_the_streams_it_names(P, ob):
    case = CC.mixed(P)
    shape = {n: (s["n_pt"], s["n_seg"]) for n, s in zip(case["names"], case["streams"])}
    assert shape["no_points"][0] == 0 < shape["no_points"][1] and shape["no_segments"][1] == 0 < shape["no_segments"][0]
    assert shape["no_candidates"] == (0, 0) and shape["many_points"][0] > 256 and len(case["streams"]) >= 5
    assert len({(s["n_pt"], s["n_seg"]) for s in case["streams"]}) == len(case["streams"])         # streams of different sizes: every offset differs
    masked = case["streams"][case["names"].index("all_masked")]
    assert masked["n_pt"] > 0 and masked["n_seg"] > 0 and not masked["active"].any()
    g = CC.grid(case, 20, 30, order_seed=3)
    for s in (0, 5):
        pc = CC.oracle_step(P, ob, case, s, 20)
        assert len(CC.winning_positions(pc, case["streams"][s], g)) > 21 and len(CC.winning_positions(pc, case["streams"][s], g, True)) > 3
    pc = CC.oracle_step(P, ob, case, case["names"].index("all_masked"), 20)
    assert pc["found"].sum() > 20 and not pc["active"].any()                                      # everything would match; nothing is wanted


def test_lds_edge_grids_stand_on_either_side_of_the_guard():
    lds = lambda W, H, c, s: (-(-W // c) * -(-H // c) + (-(-W // s) * -(-H // s) if s else 0)) * 4
    assert lds(640, 480, *CC.LDS_GRID) == 59536 <= 60000
    assert all(lds(640, 480, c, s) > 60000 for c, s in CC.LDS_REFUSED)
    assert -(-640 // 5) * -(-480 // 5) == 12288
