"""The bookkeeping classes of the sequence harness (pl-svo_amd/sequence.py: _MapTables, _SeedRows) on literal cases of a few rows: no GPU,
no backend.  These are the places where the rows of the resident tables and the landmarks of the harness's map part company."""
import importlib

import numpy as np
import pytest


@pytest.fixture(scope="module")
def seqm():
    return importlib.import_module("pl-svo_amd.sequence")


def tiny_seq(n_pts=4, n_seg=1):
    px = np.arange(2.0 * n_pts).reshape(n_pts, 2)
    f = np.tile([0.0, 0.0, 1.0], (n_pts, 1))
    z2, z3 = np.zeros((n_seg, 2)), np.tile([0.0, 0.0, 1.0], (n_seg, 1))
    return dict(poses_true=np.array([[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]]), pt_pos=10.0 + np.arange(3.0 * n_pts).reshape(n_pts, 3), pt_px0=px, pt_f0=f,
                seg_spos=np.ones((n_seg, 3)), seg_epos=2 * np.ones((n_seg, 3)), seg_spx0=z2, seg_epx0=z2 + 1, seg_sf0=z3, seg_ef0=z3)


def tables(seqm, known=(True, True, False, False)):
    """four landmarks, 0 and 1 in the map and in keyframe 0, 2 and 3 seeds; staged once, so that pt_pos holds the four positions"""
    seq = tiny_seq()
    mt = seqm._MapTables(seq, np.array(known))
    assert mt.stage_job(seq["pt_pos"]) is not None and mt.stage_job(seq["pt_pos"]) is None    # dirty at the start, clean behind a stage
    return mt, seq


def inverse_on_live_rows(mt):
    """a landmark's row is a row of that landmark -- the LAST one: a converged seed's own staged row stays behind, empty, under its new row"""
    for lm, row in enumerate(mt.lm_row):
        assert row < 0 or mt.row_lm[row] == lm
    for lm in set(mt.row_lm) - {-1}:
        assert mt.lm_row[lm] == max(row for row, v in enumerate(mt.row_lm) if v == lm)


def test_a_converged_seed_is_a_new_row_and_the_rows_follow_a_compaction(seqm):
    mt, seq = tables(seqm)
    assert mt.cm["kf_pt"] == [[0, 1]] and [len(o) for o in mt.cm["pt_obs"]] == [1, 1, 0, 0] and mt.row_lm == [0, 1, 2, 3]
    # seed 3 converges: row 4; a seed from the image: row 5, no landmark; seed 2: row 6
    assert mt.append_candidate([1.0, 2.0, 3.0], 0, seq["pt_px0"][3], seq["pt_f0"][3], 0, [0.0, 0.0], 3) == 4
    assert mt.append_candidate([4.0, 5.0, 6.0], 0, [7.0, 8.0], [0.0, 0.0, 1.0], 2, [1.0, 0.0], -1) == 5
    assert mt.append_candidate([7.0, 8.0, 9.0], 0, seq["pt_px0"][2], seq["pt_f0"][2], 0, [0.0, 0.0], 2) == 6
    cm = mt.cm
    assert mt.row_lm == [0, 1, 2, 3, 3, -1, 2] and list(mt.lm_row) == [0, 1, 6, 4] and cm["pt_cand"] == [4, 5, 6] and not mt.dirty
    inverse_on_live_rows(mt)
    assert cm["pt_pos"][4:] == [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0]] and cm["pt_type"][4:] == [seqm.abi.LM_CANDIDATE] * 3
    assert cm["pt_obs"][5] == [dict(kf=0, px=[7.0, 8.0], f=[0.0, 0.0, 1.0], level=2, type=seqm.abi.FTR_CORNER, grad=[1.0, 0.0])]
    assert cm["pt_obs"][4][0]["px"] == [6.0, 7.0] and all(type(v) is float for v in cm["pt_obs"][4][0]["px"] + cm["pt_pos"][4])
    assert list(mt.lm_of_rows([4, 5, 6])) == [3, -1, 2] and list(mt.row_of_lm([3, 2])) == [4, 6]
    # the compaction deletes row 1 (a landmark of the map), row 5 (the row without a landmark, in the middle) and row 6 (at the end)
    mt.so_keys["pt"] = [10, 11, 12, 13, 14, 15]                         # (row 6 was appended since the keys were read)
    mt.apply_pt_remap(np.array([0, -1, 1, 2, 3, -1, -1]))
    # landmark 1 has no row any more; landmark 2 lost its new row and is back at the one it was staged in
    assert mt.row_lm == [0, 2, 3, 3] and list(mt.lm_row) == [0, -1, 1, 3] and mt.so_keys["pt"] == [10, 12, 13, 14]
    inverse_on_live_rows(mt)
    # keys of rows behind the remap (appended since the compaction's report) stay
    mt.so_keys["pt"] = [1, 2, 3, 4, 5]
    mt.apply_pt_remap(np.array([0, 1, -1, 2]))
    assert mt.row_lm == [0, 2, 3] and list(mt.lm_row) == [0, -1, 1, 2] and mt.so_keys["pt"] == [1, 2, 4, 5]
    inverse_on_live_rows(mt)


def test_on_the_restaging_path_a_converged_seed_fills_its_own_row(seqm):
    mt, seq = tables(seqm)
    assert mt.append_candidate(None, 0, seq["pt_px0"][2], seq["pt_f0"][2], 0, [0.0, 0.0], 2, own_row=True) == 2
    assert mt.dirty and mt.row_lm == [0, 1, 2, 3] and mt.cm["pt_cand"] == [2] and mt.cm["pt_type"][2] == seqm.abi.LM_CANDIDATE and len(mt.cm["pt_pos"]) == 4
    assert mt.cm["pt_obs"][2] == [dict(kf=0, px=[4.0, 5.0], f=[0.0, 0.0, 1.0], level=0, type=seqm.abi.FTR_CORNER, grad=[0.0, 0.0])]
    moved = seq["pt_pos"] + 1.0
    assert mt.stage_job(moved) is not None and mt.cm["pt_pos"][2] == [float(v) for v in moved[2]] and not mt.dirty


def test_the_seed_keyframe_row_follows_the_removals(seqm):
    mt, _ = tables(seqm)
    mt.seed_kf = 2
    mt.keyframe_removed(3); assert mt.seed_kf == 2
    mt.keyframe_removed(0); assert mt.seed_kf == 1
    mt.keyframe_removed(1); assert mt.seed_kf is None
    mt.keyframe_removed(0); assert mt.seed_kf is None


def test_key_point_positions_skip_null_and_out_of_range_holders(seqm):
    mt, seq = tables(seqm, known=(True, True, True, False))
    mt.cm["kf_pt"] = [[0, 1, 2], [2, -1]]                               # keyframe 1: landmark 2, and a feature safeDelete* cut loose
    mt.cm["kf_T"].append(mt.cm["kf_T"][0])
    kp = [[2, -1, 0, 3, 1], [1, 0, 2, -1, 0]]                           # holders: positions in the feature lists; 3 / 2 are out of range, [1][0] holds no landmark
    kpos, kval = mt.key_point_positions(kp)
    assert kval.dtype == np.uint8 and kval.tolist() == [[1, 0, 1, 0, 1], [0, 1, 0, 0, 1]] and kpos.shape == (2, 5, 3)
    P = seq["pt_pos"]
    assert np.array_equal(kpos[0], [P[2], [0, 0, 0], P[0], [0, 0, 0], P[1]]) and np.array_equal(kpos[1], [[0, 0, 0], P[2], [0, 0, 0], [0, 0, 0], P[2]])
    # the same table read from a fetched record of the device's tables, whose positions differ from the harness's own
    fetched = dict(kf_pt_off=np.array([0, 3, 5], np.int32), kf_pt_lm=np.array([0, 1, 2, 2, -1], np.int32), pt_pos=P + 100.0)
    kpos_f, kval_f = mt.key_point_positions(kp, fetched)
    assert np.array_equal(kval_f, kval) and np.array_equal(kpos_f, kpos + 100.0 * kval[:, :, None])


def test_the_selection_s_deletions_cut_keyframe_features_loose(seqm):
    mt, _ = tables(seqm)
    abi = seqm.abi
    q = dict(pt_event=np.array([0, abi.LM_EVENT_DELETED, 0, 0]), seg_event=np.array([0]), pt_type=np.array([abi.LM_UNKNOWN, abi.LM_DELETED, abi.LM_UNKNOWN, abi.LM_CANDIDATE]),
             seg_type=np.array([abi.LM_UNKNOWN]), pt_cand=np.array([3]), seg_cand=np.array([], np.int64))
    mt.follow_selection(q)
    assert mt.cm["kf_pt"] == [[0, -1]] and mt.cm["kf_seg"] == [[0]] and mt.cm["pt_type"] == [int(v) for v in q["pt_type"]] and mt.cm["pt_cand"] == [3]


def test_seed_rows_follow_removals_starts_and_erasures(seqm):
    abi = seqm.abi
    rows = seqm._SeedRows()
    rows.rows = [(7, 0, None), (9, 0, None), (-1, 1, dict(px=[1.0, 1.0])), (-1, 2, dict(px=[2.0, 2.0])), (-1, 3, dict(px=[3.0, 3.0]))]
    assert list(rows.lms()) == [7, 9, -1, -1, -1] and rows.lms().dtype == np.int64 and rows.n_image() == 3
    rows.remove_keyframe(1)                                             # its seed leaves, the keyframe rows behind it move down
    assert [(lm, kf) for lm, kf, _ in rows.rows] == [(7, 0), (9, 0), (-1, 1), (-1, 2)] and [r[2]["px"][0] for r in rows.rows[2:]] == [2.0, 3.0]
    lists = dict(pt_ref_kf=np.zeros(6), pt_px=np.arange(12.0).reshape(6, 2), pt_f=np.ones((6, 3)), pt_level=np.arange(6))
    rows.started(2, 3, lists)
    assert rows.rows[4:] == [(-1, 3, dict(px=[8.0, 9.0], f=[1.0, 1.0, 1.0], level=4)), (-1, 3, dict(px=[10.0, 11.0], f=[1.0, 1.0, 1.0], level=5))]
    with pytest.raises(AssertionError):
        rows.started(1, 3, lists)                                       # the fetched lists must hold exactly the rows the harness follows
    rows.drop(np.array([abi.SEED_UPDATED, abi.SEED_CONVERGED, abi.SEED_NAN, abi.SEED_UPDATED, abi.SEED_AGED, abi.SEED_UPDATED]))
    assert [(lm, kf) for lm, kf, _ in rows.rows] == [(7, 0), (-1, 2), (-1, 3)] and rows.n_image() == 2
    rows.remove_keyframe(0)
    assert [(lm, kf) for lm, kf, _ in rows.rows] == [(-1, 1), (-1, 2)] and len(rows.lms()) == 2
