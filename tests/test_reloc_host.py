"""tests/np_reloc.py tied down on the CPU: the closest keyframe against the front of np_keystage's close list, the job from a keyframe
against the job the host path assembles for the same keyframe (pl-svo_amd/sequence.py::align_kf_job_host), the gate against a literal
transcription of the reference's lines with their unsigned arithmetic and against the host path's comparisons (track_gate_host)."""
import itertools

import numpy as np

import alignjob_cases as A
import np_keyframe as K
import np_keystage as Ks
import np_reloc as R
import reloc_cases as Rc


def test_the_closest_keyframe_is_the_front_of_the_close_list():
    s = Rc.three_keyframes()
    st, cam = s["st"], A.SMALL["cam_t"]
    t = R.tables_of(st)
    key = Ks.fresh(st, cam)
    seen = set()
    for dx, self_kf in itertools.product((-0.07, -0.05, -0.045, -0.02, 0.0, 0.01), (-1, 0, 1, 2)):
        T = Rc.far_T(dx)
        c = Ks.close(st, key, T, cam, max_n_kfs=10)
        order = [int(i) for i in c["close_idx"]]
        want = None if not order else order[0] if order[0] != self_kf else (order[1] if len(order) > 1 else None)
        assert R.closest_keyframe(t, key, T, cam, self_kf) == want, (dx, self_kf, order)
        seen.add(want)
    assert seen == {0, 1, 2}
    # an exact tie keeps the lower row; nothing visible: None; self the only close one: None (PINNED)
    assert R.closest_keyframe(t, key, Rc.far_T(-0.045), cam) == 0 and R.closest_keyframe(t, key, Rc.far_T(-0.045), cam, self_kf=0) == 1
    assert R.closest_keyframe(t, key, [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0], cam) is None
    only = np.array([[-1] * 5, [-1] * 5, list(key[2])], np.int32)
    assert R.closest_keyframe(t, only, Rc.far_T(0.0), cam) == 2 and R.closest_keyframe(t, only, Rc.far_T(0.0), cam, self_kf=2) is None


HOST_ARRAYS = ("pt_px", "pt_xyz_ref", "seg_spx", "seg_epx", "seg_len", "seg_p_ref", "seg_q_ref", "seg_alive_in")


def test_the_job_from_a_keyframe_equals_the_host_paths_job(P):
    """pl-svo_amd/sequence.py::align_kf_job_host is what a host caller assembles from fetched tables (tools/bench_reloc.py's host path):
    the restatement's job equals it in every array, exactly"""
    cam, cfg = A.SMALL["cam_t"], Rc.cfg()
    for s, rows in ((Rc.holes(), (0, 1, 2)), (Rc.shared(), (0, 1)), (Rc.kept_points(70), (0, 1)), (Rc.only(0, 0), (1,))):
        t = R.tables_of(s["st"])
        for k in rows:
            for T_init, src in ((Rc.T_INIT, R.INIT_HOST), (None, R.INIT_KEYFRAME)):
                w = R.kf_align_job(t, k, T_init, cam, cfg, 64, init_source=src)
                h = P.sequence.align_kf_job_host(cam, cfg["max_level"], cfg["min_level"], t, k, T_init, Rc.CUR_SLOT)
                assert w["report"]["status"] == R.OK and w["report"]["ref_kf"] == k and (h.c.ref_slot, h.c.cur_slot) == (s["st"]["kf_slot"][k], Rc.CUR_SLOT)
                for f in HOST_ARRAYS:
                    g = np.asarray(getattr(h, f))
                    assert g.tobytes() == np.asarray(w[f], g.dtype).reshape(g.shape).tobytes(), (k, f)
                assert np.array(h.c.T_cur_from_ref[:]).tobytes() == np.asarray(w["T0"], float).tobytes(), (k, "T0")
    cam, cfg = A.SMALL["cam_t"], Rc.cfg()
    # the keyframe's own pose as the initial one: T_kf * T_kf^-1
    t = R.tables_of(Rc.holes()["st"])
    w = R.kf_align_job(t, 1, None, cam, cfg, 64, init_source=R.INIT_KEYFRAME)
    kfT = Rc.holes()["st"]["kf_T"][1]
    assert np.array_equal(w["T0"], K.se3_mul(kfT, K.se3_inv(kfT)))
    # capacities: one more kept point, or one more segment feature, than the rows
    assert R.kf_align_job(t, 1, Rc.T_INIT, cam, Rc.cfg(cap_pts=10), 64)["report"]["status"] == R.NO_ROOM
    assert R.kf_align_job(t, 1, Rc.T_INIT, cam, Rc.cfg(cap_seg=8), 64)["report"]["status"] == R.NO_ROOM
    assert R.kf_align_job(t, 1, Rc.T_INIT, cam, Rc.cfg(cap_pts=11, cap_seg=9), 64)["report"]["status"] == R.OK


U64 = 1 << 64


def literal_gate(n_pt, n_ls, obs_pt, obs_ls, last_pt, last_ls, mode, min_fts, max_drop, max_fts, max_fts_segs):
    """src/frame_handler_mono.cpp:315-321, :335, src/frame_handler_base.cpp:173-190 line by line; size_t arithmetic wraps at 2^64 and
    `const int feature_drop = static_cast<int>(std::min(..)) - num_observations` converts the unsigned difference to int"""
    def to_int(v):
        v %= 1 << 32
        return v - (1 << 32) if v >= 1 << 31 else v
    if (n_pt + n_ls) % U64 < min_fts:
        return R.FAIL_MATCHES, R.INSUFFICIENT, True, None, None      # new_frame_->T_f_w_ = last_frame_->T_f_w_; tracking_quality_ = TRACKING_INSUFFICIENT
    if (obs_pt + obs_ls) % U64 < 10:
        return R.FAIL_EDGES, R.INSUFFICIENT, mode == R.GATE_RELOC, None, None   # RESULT_FAILURE: finishFrameProcessingCommon sets TRACKING_INSUFFICIENT; :432 resets
    quality = R.GOOD
    if (obs_pt + obs_ls) % U64 < min_fts:
        quality = R.BAD
    drop_pt = to_int((to_int(min(last_pt, max_fts)) - obs_pt) % U64)
    drop_ls = to_int((to_int(min(last_ls, max_fts_segs)) - obs_ls) % U64)
    if drop_pt > int(max_drop):
        quality = R.BAD
    return R.GATE_OK, quality, False, drop_pt, drop_ls


def test_the_gate_equals_the_literal_transcription(P):
    T_opt, T_reset = np.arange(7.0), -np.arange(7.0)
    results = set()
    for name, c in Rc.gate_counts().items():
        for mode in (R.GATE_TRACK, R.GATE_RELOC):
            rec, T, last = R.gate(*c, T_opt, T_reset, mode=mode)
            result, quality, reset, drop_pt, drop_ls = literal_gate(*c, mode, 20, 50.0, 100, 100)
            if result == R.GATE_OK:
                assert (rec["drop_pt"], rec["drop_ls"]) == (drop_pt, drop_ls), name
            assert (rec["result"], rec["tracking_quality"]) == (result, quality), (name, mode)
            assert np.array_equal(T, T_reset if reset else T_opt), (name, mode)
            assert last == (c[0], c[1]) and rec["n_matched"] == c[0] + c[1] and rec["n_edges"] == c[2] + c[3]
            results.add((name, rec["result"], rec["tracking_quality"]))
            assert P.sequence.track_gate_host(*c, relocalizing=mode == R.GATE_RELOC) == (result, quality, reset), (name, mode)   # the host path's comparisons
    want = dict(matched_19=(R.FAIL_MATCHES, R.INSUFFICIENT), matched_20=(R.GATE_OK, R.GOOD), edges_9=(R.FAIL_EDGES, R.INSUFFICIENT), edges_10=(R.GATE_OK, R.BAD),
                edges_19=(R.GATE_OK, R.BAD), edges_20=(R.GATE_OK, R.GOOD), drop_50=(R.GATE_OK, R.GOOD), drop_51=(R.GATE_OK, R.BAD), clamp=(R.GATE_OK, R.GOOD),
                clamp_above=(R.GATE_OK, R.BAD), seg_drop_alone=(R.GATE_OK, R.GOOD), nothing=(R.FAIL_MATCHES, R.INSUFFICIENT))
    assert results == {(k,) + v for k, v in want.items()}
    assert R.gate(*Rc.gate_counts()["seg_drop_alone"], T_opt, T_reset)[0]["drop_ls"] == 85
