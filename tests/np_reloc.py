"""Restatement of relocalisation on the resident map (pl-svo_amd/csrc/alignjob_device.hpp: map_align_kf_job_kernel, map_track_gate_kernel;
plsvo_candidates_align_build_kf, plsvo_candidates_track_gate) in the reference's sequential form (test infrastructure only):

  closest_keyframe   Map::getClosestKeyframe (src/map.cpp:181-199) over Map::getCloseKeyframes (:158-179) on the key-point table and the
                     LIVE position of each key point's landmark
  kf_align_job       what SparseImgAlign::run(ref_keyframe, new_frame_) reads of a keyframe of the tables
                     (src/frame_handler_mono.cpp:408-436, src/sparse_img_align.cpp:80, :229-230, :327-330, src/feature.cpp:90), laid out by
                     np_alignjob's first-fit
  gate               the gates of FrameHandlerMono::processFrame (:315-321, :335) and FrameHandlerBase::setTrackingQuality
                     (src/frame_handler_base.cpp:173-190)

The tables are the flat arrays capi.Context.candidates_fetch_map() returns (CSR offsets relative to the stream); tables_of() makes
them from a stream dict of tests/candidates_cases.py.  Arithmetic on Python floats in the device's operation order, as tests/np_alignjob.py."""
import numpy as np

import np_alignjob as NA
import np_keyframe as K

TYPE_DELETED = NA.TYPE_DELETED
OK, NO_ROOM, NO_KEYFRAME = 0, 1, 2
CLOSEST = -1
INIT_HOST, INIT_DEV, INIT_KEYFRAME = 0, 1, 2
GATE_TRACK, GATE_RELOC = 0, 1
GATE_OK, FAIL_MATCHES, FAIL_EDGES = 0, 1, 2
INSUFFICIENT, BAD, GOOD = 0, 1, 2


def tables_of(st):
    """the flat tables of a stream dict (candidates_cases.to_job's arrays)"""
    import candidates_cases as Cc
    return {f: np.array(v) for f, v in Cc.to_job(st).t.items()}


def _rows(t, f, w):
    return np.asarray(t[f], np.float64).reshape(-1, w)


def first_obs(obs_off, obs_kf, lm, kf):
    """the first observation of landmark lm whose obs_kf is kf (keystage_device.hpp::ks_feature_px's pairing), or -1"""
    for o in range(int(obs_off[lm]), int(obs_off[lm + 1])):
        if int(obs_kf[o]) == kf:
            return o
    return -1


def close_list(t, key_pts, T_last, cam):
    """Map::getCloseKeyframes: (row, distance) in keyframe order"""
    kf_T, pt_pos = _rows(t, "kf_T", 7), _rows(t, "pt_pos", 3)
    T = [float(v) for v in T_last]
    out = []
    for i in range(len(kf_T)):
        f0, n_ftr = int(t["kf_pt_off"][i]), int(t["kf_pt_off"][i + 1]) - int(t["kf_pt_off"][i])
        for k in range(5):
            h = int(key_pts[i][k])
            if h < 0 or h >= n_ftr:
                continue
            lm = int(t["kf_pt_lm"][f0 + h])
            if lm < 0:
                continue
            if K.is_visible(T, cam, [float(v) for v in pt_pos[lm]]):
                Kf = [float(v) for v in kf_T[i]]
                out.append((i, K.norm3(T[4] - Kf[4], T[5] - Kf[5], T[6] - Kf[6])))
                break
    return out


def closest_keyframe(t, key_pts, T_last, cam, self_kf=-1):
    """Map::getClosestKeyframe: the front of the stable sort by distance; when that is the frame itself, the next one.  PINNED: with the
    frame itself the only close keyframe the reference calls front() on an empty list; here that is None"""
    close = close_list(t, key_pts, T_last, cam)
    if not close:
        return None
    close.sort(key=lambda e: e[1])                     # stable, like std::list::sort
    if close[0][0] != self_kf:
        return close[0][0]
    close.pop(0)
    return close[0][0] if close else None


def kf_align_job(t, ref_kf, T_init, cam, cfg, seg_align, init_source=INIT_HOST, key_pts=None, T_last=None, self_kf=-1):
    """the job of plsvo_candidates_align_build_kf for one stream, as np_alignjob.align_job reports a job, with report["ref_kf"]"""
    if ref_kf == CLOSEST:
        k = closest_keyframe(t, key_pts, T_last, cam, self_kf)
        ref_kf = -1 if k is None else k
    kf_T = _rows(t, "kf_T", 7)
    have = ref_kf >= 0
    if init_source == INIT_KEYFRAME and have:
        T_init = kf_T[ref_kf]
    T_init = [float(v) for v in T_init]
    T_ref = [float(v) for v in kf_T[ref_kf]] if have else T_init
    T_inv = K.se3_inv(T_ref)
    T0 = K.se3_mul(T_init, T_inv)                      # src/sparse_img_align.cpp:80
    ref_pos = T_inv[4:]
    levels = list(range(cfg["max_level"], cfg["min_level"] - 1, -1))
    z2, z3 = np.zeros((0, 2)), np.zeros((0, 3))
    empty = dict(pt_px=z2, pt_xyz_ref=z3, seg_spx=z2, seg_epx=z2, seg_len=np.zeros(0), seg_p_ref=z3, seg_q_ref=z3, seg_alive_in=np.zeros(0, np.uint8),
                 seg_code=np.zeros((len(levels), 0), np.int32))
    if not have:                                       # "No reference keyframe" (:413-417)
        job = dict(n_pts=0, n_seg=0, skip=1, long_mask=0, n_slots=np.zeros(NA.MAX_LEVELS, np.int32), n_patches=0, T0=np.array(T0), T_ref=np.array(T_ref),
                   report=dict(n_pts=0, n_seg=0, n_seg_alive=0, n_slots=0, long_mask=0, status=NO_KEYFRAME, ref_kf=-1))
        job.update(empty)
        return job
    pt_pos, seg_spos, seg_epos = _rows(t, "pt_pos", 3), _rows(t, "seg_spos", 3), _rows(t, "seg_epos", 3)
    pt_obs_px, pt_obs_f = _rows(t, "pt_obs_px", 2), _rows(t, "pt_obs_f", 3)
    spx, epx, sf, ef = _rows(t, "seg_obs_spx", 2), _rows(t, "seg_obs_epx", 2), _rows(t, "seg_obs_sf", 3), _rows(t, "seg_obs_ef", 3)
    # -- points: the keyframe's list in order
    kept = []
    for i in range(int(t["kf_pt_off"][ref_kf]), int(t["kf_pt_off"][ref_kf + 1])):
        lm = int(t["kf_pt_lm"][i])
        if lm < 0 or int(t["pt_type"][lm]) == TYPE_DELETED:
            continue
        o = first_obs(t["pt_obs_off"], t["pt_obs_kf"], lm, ref_kf)
        if o >= 0:
            kept.append((lm, o))
    # -- segments: all of them
    seg_ftr = []
    for i in range(int(t["kf_seg_off"][ref_kf]), int(t["kf_seg_off"][ref_kf + 1])):
        lm = int(t["kf_seg_lm"][i])
        o = first_obs(t["seg_obs_off"], t["seg_obs_kf"], lm, ref_kf) if lm >= 0 and int(t["seg_type"][lm]) != TYPE_DELETED else -1
        seg_ftr.append((lm, o))
    alive = [o >= 0 for _, o in seg_ftr]
    segs = [[float(spx[o][0]), float(spx[o][1]), float(epx[o][0]), float(epx[o][1])] if o >= 0 else [0.0] * 4 for _, o in seg_ftr]
    n_pts, n_seg = len(kept), len(seg_ftr)
    fits = n_pts <= cfg["cap_pts"] and n_seg <= cfg["cap_seg"]
    laid_out = fits
    n_slots, long_mask, patches, finest = [0] * NA.MAX_LEVELS, 0, 0, 0
    codes = {}
    if laid_out:
        for level in levels:
            r = NA.layout_level(n_pts, segs, alive, level, cam, seg_align)
            if r is None:
                laid_out = False
                break
            codes[level], n_slots[level], any_long, np_ = r
            if n_slots[level] > cfg["slot_cap"]:
                fits = False
            long_mask |= int(any_long) << level
            patches += np_
            finest = n_slots[level]
    if not laid_out:
        fits, long_mask, finest = False, 0, 0
    report = dict(n_pts=n_pts, n_seg=n_seg, n_seg_alive=sum(alive), n_slots=finest, long_mask=long_mask, status=OK if fits else NO_ROOM, ref_kf=ref_kf)
    skip = (not fits) or (n_pts == 0 and n_seg == 0)
    job = dict(n_pts=n_pts if fits else 0, n_seg=n_seg if fits else 0, skip=int(skip), long_mask=long_mask if fits else 0,
               n_slots=np.array(n_slots if fits else [0] * NA.MAX_LEVELS, np.int32), n_patches=0 if skip else patches, T0=np.array(T0), T_ref=np.array(T_ref), report=report)
    if not fits:
        job.update(empty)
        return job
    px, xyz = [], []
    for lm, o in kept:
        f, d = [float(v) for v in pt_obs_f[o]], NA.dist([float(v) for v in pt_pos[lm]], ref_pos)   # the STORED bearing
        px.append([float(pt_obs_px[o][0]), float(pt_obs_px[o][1])])
        xyz.append([f[0] * d, f[1] * d, f[2] * d])
    p_ref, q_ref, length = [], [], []
    for (lm, o), px4 in zip(seg_ftr, segs):
        if o < 0:                                      # PINNED: no pixels in the tables for a feature without a landmark: zeros
            p_ref.append([0.0] * 3); q_ref.append([0.0] * 3); length.append(0.0)
            continue
        ds, de = NA.dist([float(v) for v in seg_spos[lm]], ref_pos), NA.dist([float(v) for v in seg_epos[lm]], ref_pos)
        a, b = [float(v) for v in sf[o]], [float(v) for v in ef[o]]
        p_ref.append([a[0] * ds, a[1] * ds, a[2] * ds]); q_ref.append([b[0] * de, b[1] * de, b[2] * de]); length.append(NA.seg_len(px4))
    job.update(pt_px=np.array(px).reshape(-1, 2), pt_xyz_ref=np.array(xyz).reshape(-1, 3), seg_spx=np.array([s[:2] for s in segs]).reshape(-1, 2),
               seg_epx=np.array([s[2:] for s in segs]).reshape(-1, 2), seg_len=np.array(length), seg_p_ref=np.array(p_ref).reshape(-1, 3),
               seg_q_ref=np.array(q_ref).reshape(-1, 3), seg_alive_in=np.array(alive, np.uint8),
               seg_code=np.array([codes[level] for level in sorted(levels)], np.int32).reshape(len(levels), n_seg))
    return job


def gate(n_matches, n_ls_matches, num_obs_pt, num_obs_ls, num_obs_last_pt, num_obs_last_ls, T_opt, T_reset, mode=GATE_TRACK, quality_min_fts=20,
         quality_max_drop_fts=50, max_fts=100, max_fts_segs=100):
    """-> (record: plsvo_cand_gate_out's fields, the pose carried forward, the new (num_obs_last_pt, num_obs_last_ls))"""
    n_matched, n_edges = n_matches + n_ls_matches, num_obs_pt + num_obs_ls
    if n_matched < quality_min_fts:                    # "Not enough matched features" (:315-321)
        result = FAIL_MATCHES
    elif n_edges < 10:                                 # :335
        result = FAIL_EDGES
    else:
        result = GATE_OK
    quality = GOOD                                     # setTrackingQuality
    if n_edges < quality_min_fts:
        quality = BAD
    drop_pt = min(num_obs_last_pt, max_fts) - num_obs_pt
    drop_ls = min(num_obs_last_ls, max_fts_segs) - num_obs_ls
    if drop_pt > quality_max_drop_fts:
        quality = BAD
    if result != GATE_OK:                              # finishFrameProcessingCommon
        quality = INSUFFICIENT
    reset = result == FAIL_MATCHES or (result == FAIL_EDGES and mode == GATE_RELOC)
    rec = dict(result=result, tracking_quality=quality, n_matched=n_matched, n_edges=n_edges, drop_pt=drop_pt, drop_ls=drop_ls, num_obs_last_pt=num_obs_last_pt,
               num_obs_last_ls=num_obs_last_ls)
    return rec, np.array(T_reset if reset else T_opt, np.float64), (n_matches, n_ls_matches)
