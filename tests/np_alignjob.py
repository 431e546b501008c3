"""Restatement of the alignment job built on the device from the resident selection (plsvo_candidates_align_build,
pl-svo_amd/csrc/alignjob_device.hpp) in sequential form (test infrastructure only): what the caller of SparseImgAlign::run(last_frame_,
new_frame_) gathers (src/frame_handler_mono.cpp:266-274, src/sparse_img_align.cpp:80, :229-230, :327-330, src/feature.cpp:90, :160-173)
and the static patch-slot layout of the alignment launch, per level.

Every function works on Python floats (IEEE binary64, one rounding per operation, no contraction) in the device's operation order, so
the device's arrays can be compared byte for byte; sqrt is correctly rounded on both sides.  The layout is written on its own, as a
plain first-fit loop over the segments in decreasing N, not after plsvo_capi.hip::slot_layout.

Inputs of align_job(): the selection (pt_lm, pt_px [n, 2], seg_lm, seg_px [n, 4]: spx, epx), the keep masks in selection order, the
landmarks' types and positions as the tables hold them at build time, the reference frame's pose, the camera (fx, fy, cx, cy, w, h) and the
reserve's configuration.  PINNED as on the device: a feature whose landmark is TYPE_DELETED counts as feat3D == NULL."""
import math

import numpy as np

import np_keyframe as K

TYPE_DELETED = 0
OK, NO_ROOM = 0, 1
ROUND = 64
BINS = 128                                             # wave-rounds the short segments of one level may open (kAlignJobBins)
MAX_LEVELS = 8


def bearing(cam, px):
    """vk::PinholeCamera::cam2world, normalised as Feature's constructor does (select_device.hpp::sel_bearing)"""
    x, y = (px[0] - cam[2]) / cam[0], (px[1] - cam[3]) / cam[1]
    n = math.sqrt((x * x + y * y) + 1.0)
    return [x / n, y / n, 1.0 / n]


def dist(p, ref):
    dx, dy, dz = p[0] - ref[0], p[1] - ref[1], p[2] - ref[2]
    return math.sqrt(dx * dx + dy * dy + dz * dz)


def seg_len(px4):
    dx, dy = px4[2] - px4[0], px4[3] - px4[1]
    return math.sqrt(dx * dx + dy * dy)


def _div(a, b):
    return a / b if b != 0.0 else (math.nan if a == 0.0 or a != a else math.copysign(math.inf, a))


def num_samples(px4, length, level):
    """LineFeat::setupSampling (src/feature.cpp:160-173) and N = 1 + (N0 - 1) / 2^level (src/sparse_img_align.cpp:320)"""
    d0, d1 = abs(px4[2] - px4[0]), abs(px4[3] - px4[1])
    tan_dir = _div(min(d0, d1) if d0 == d0 and d1 == d1 else math.nan, max(d0, d1))
    sin_dir = tan_dir / math.sqrt(1.0 + tan_dir * tan_dir)
    correction = 2.0 * math.sqrt(1.0 + sin_dir * sin_dir)
    v = _div(length, 2.0 * 4 * correction)
    n0 = int(v) if 1.0 < v else 1
    return 1 + (n0 - 1) // (1 << level)


def in_border(px4, level, cam):
    """both end points pass the 3-pixel border test of the level (src/sparse_img_align.cpp:299-301)"""
    scale = 1.0 / float(1 << level)
    cw, ch = int(cam[4]) // (1 << level), int(cam[5]) // (1 << level)
    u = [int(px4[0] * scale), int(px4[2] * scale)]
    v = [int(px4[1] * scale), int(px4[3] * scale)]
    return all(3 <= a < cw - 3 for a in u) and all(3 <= b < ch - 3 for b in v)


def layout_level(n_pts, segs, alive, level, cam, seg_align):
    """-> (codes per segment: first slot | N << 20 or -1, slots in use, a segment of more than 64 samples?, points + samples), or None when
    the level cannot be laid out at all (a segment of more than 2047 samples, more rounds than bins)"""
    n_seg = len(segs)
    N = [num_samples(s, seg_len(s), level) if a and in_border(s, level, cam) else -1 for s, a in zip(segs, alive)]
    if any(n > 2047 for n in N):
        return None
    patches = n_pts + sum(n for n in N if n > 0)
    codes = [-1] * n_seg
    seg0 = ((n_pts + ROUND - 1) // ROUND) * ROUND if (seg_align == 64 and n_seg > 0) else n_pts
    first_round, used = seg0 // ROUND, n_pts
    shorts = sorted((s for s in range(n_seg) if 0 <= N[s] <= ROUND), key=lambda s: (-N[s], s))      # decreasing N, ties in feature order
    taken = [seg0 - first_round * ROUND]               # slots taken in round first_round + k
    for s in shorts:
        k = next((k for k, t in enumerate(taken) if t + N[s] <= ROUND), None)
        if k is None:
            if len(taken) >= BINS:
                return None
            taken.append(0)
            k = len(taken) - 1
        first = (first_round + k) * ROUND + taken[k]
        taken[k] += N[s]
        codes[s] = (N[s] << 20) | first
        used = max(used, first + N[s])
    longs = [s for s in range(n_seg) if N[s] > ROUND]
    if longs:                                          # behind the packed rounds, in feature order
        cur = (first_round + len(taken)) * ROUND if shorts else ((seg0 + ROUND - 1) // ROUND) * ROUND
        for s in longs:
            codes[s] = (N[s] << 20) | (cur & 0xfffff)
            cur += N[s]
        used = cur
    return codes, used, bool(longs), patches


def align_job(sel, pt_keep, seg_keep, pt_type, seg_type, pt_pos, seg_spos, seg_epos, T_ref, cam, cfg, seg_align):
    """cfg: dict(max_level, min_level, cap_pts, cap_seg, slot_cap).  -> dict of the job as plsvo_candidates_align_fetch_job reports it
    (n_pts, n_seg, skip, long_mask, n_slots [8], n_patches, T0, T_ref, the feature arrays, seg_code [levels from min_level, n_seg]) and
    `report` (plsvo_cand_align_report's fields)"""
    T_ref = [float(v) for v in T_ref]
    T_inv = K.se3_inv(T_ref)
    T0 = K.se3_mul(T_ref, T_inv)                       # cur.T_f_w * ref.T_f_w^-1 with cur.T_f_w = ref.T_f_w: not the literal identity
    ref_pos = T_inv[4:]
    pt_lm, seg_lm = [int(v) for v in sel["pt_lm"]], [int(v) for v in sel["seg_lm"]]
    pt_px = [[float(v) for v in p] for p in np.asarray(sel["pt_px"], float).reshape(-1, 2)]
    segs = [[float(v) for v in p] for p in np.asarray(sel["seg_px"], float).reshape(-1, 4)]
    kept = [i for i, lm in enumerate(pt_lm) if pt_keep[i] and pt_type[lm] != TYPE_DELETED]
    alive = [bool(seg_keep[s]) and seg_type[lm] != TYPE_DELETED for s, lm in enumerate(seg_lm)]
    n_pts, n_seg = len(kept), len(segs)
    levels = list(range(cfg["max_level"], cfg["min_level"] - 1, -1))
    fits = n_pts <= cfg["cap_pts"] and n_seg <= cfg["cap_seg"]
    laid_out = fits
    n_slots, long_mask, patches, finest = [0] * MAX_LEVELS, 0, 0, 0
    codes = {}
    if laid_out:
        for level in levels:
            r = layout_level(n_pts, segs, alive, level, cam, seg_align)
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
    report = dict(n_pts=n_pts, n_seg=n_seg, n_seg_alive=sum(alive), n_slots=finest, long_mask=long_mask, status=OK if fits else NO_ROOM)
    skip = (not fits) or (n_pts == 0 and n_seg == 0)
    job = dict(n_pts=n_pts if fits else 0, n_seg=n_seg if fits else 0, skip=int(skip), long_mask=long_mask if fits else 0,
               n_slots=np.array(n_slots if fits else [0] * MAX_LEVELS, np.int32), n_patches=0 if skip else patches, T0=np.array(T0), T_ref=np.array(T_ref), report=report)
    z2, z3 = np.zeros((0, 2)), np.zeros((0, 3))
    if not fits:                                       # dropped whole: no feature rows
        job.update(pt_px=z2, pt_xyz_ref=z3, seg_spx=z2, seg_epx=z2, seg_len=np.zeros(0), seg_p_ref=z3, seg_q_ref=z3, seg_alive_in=np.zeros(0, np.uint8),
                   seg_code=np.zeros((len(levels), 0), np.int32))
        return job
    xyz = []
    for i in kept:
        f, d = bearing(cam, pt_px[i]), dist(pt_pos[pt_lm[i]], ref_pos)
        xyz.append([f[0] * d, f[1] * d, f[2] * d])
    p_ref, q_ref = [], []
    for s, (px4, a) in enumerate(zip(segs, alive)):
        if not a:
            p_ref.append([0.0] * 3); q_ref.append([0.0] * 3)
            continue
        sf, ef = bearing(cam, px4[:2]), bearing(cam, px4[2:])
        ds, de = dist(seg_spos[seg_lm[s]], ref_pos), dist(seg_epos[seg_lm[s]], ref_pos)
        p_ref.append([sf[0] * ds, sf[1] * ds, sf[2] * ds]); q_ref.append([ef[0] * de, ef[1] * de, ef[2] * de])
    job.update(pt_px=np.array([pt_px[i] for i in kept]).reshape(-1, 2), pt_xyz_ref=np.array(xyz).reshape(-1, 3),
               seg_spx=np.array([s[:2] for s in segs]).reshape(-1, 2), seg_epx=np.array([s[2:] for s in segs]).reshape(-1, 2),
               seg_len=np.array([seg_len(s) for s in segs]), seg_p_ref=np.array(p_ref).reshape(-1, 3), seg_q_ref=np.array(q_ref).reshape(-1, 3),
               seg_alive_in=np.array(alive, np.uint8),
               seg_code=np.array([codes[level] for level in sorted(levels)], np.int32).reshape(len(levels), n_seg))
    return job


def empty_job(cfg):
    """a stream that has never been built: the reserve's empty job at the identity"""
    ident = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    z2, z3 = np.zeros((0, 2)), np.zeros((0, 3))
    return dict(n_pts=0, n_seg=0, skip=1, long_mask=0, n_slots=np.zeros(MAX_LEVELS, np.int32), n_patches=0, T0=ident, T_ref=ident, pt_px=z2, pt_xyz_ref=z3, seg_spx=z2,
                seg_epx=z2, seg_len=np.zeros(0), seg_p_ref=z3, seg_q_ref=z3, seg_alive_in=np.zeros(0, np.uint8),
                seg_code=np.zeros((cfg["max_level"] - cfg["min_level"] + 1, 0), np.int32),
                report=dict(n_pts=0, n_seg=0, n_seg_alive=0, n_slots=0, long_mask=0, status=OK))


def compose(T_cur_from_ref, T_ref):
    """cur_frame->T_f_w_ = T_cur_from_ref * ref_frame->T_f_w_ (src/sparse_img_align.cpp:92)"""
    return np.array(K.se3_mul(T_cur_from_ref, T_ref))
