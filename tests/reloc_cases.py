"""Cases of relocalisation on the resident map (plsvo_candidates_align_build_kf, plsvo_candidates_track_gate), on alignjob_cases.Builder:
streams of two or three keyframes under the 326 x 246 camera (and the wide one for the packing), tens of features.  A keyframe's
feature is a landmark of its list whose observation in that keyframe holds px, f, sf, ef.  Built once, never changed."""
import functools

import numpy as np

import alignjob_cases as A
import select_cases as Sc

D, C_, U, G = Sc.D, Sc.C_, Sc.U, Sc.G
T_INIT = [0.004, 0.001, -0.002, 0.99998875, -0.02, 0.015, 0.01]   # an initial pose handed over by the host (copied, never normalised)
CUR_SLOT = 3


def cfg(**kw):
    return A.cfg(**kw)


def grid(b, n_pt, n_seg, kfs=(0,), first_cell=11, typ=G):
    for k in range(n_pt):
        b.pt(*A.cell_px(b.geo, k + first_cell), kfs=kfs, typ=typ)
    cells = iter(c for c in range(16, 126, 2) if 2 <= c % 14 <= 10)
    for k in range(n_seg):
        p = A.cell_px(b.geo, next(cells), True)
        b.seg((p[0] - 6, p[1]), (p[0] + 6, p[1] + 2 + k % 3), kfs=kfs, typ=typ)
    return b


@functools.lru_cache(maxsize=None)
def holes():
    """keyframe 1's lists: -1 features (no landmark) at the head, in the middle and at the tail, a TYPE_DELETED landmark in the middle
    of each list, a TYPE_CANDIDATE landmark of each kind (kept); keyframe 0 and 2 hold a few features of their own"""
    b = A.Builder(A.SMALL, 3)
    grid(b, 4, 2, kfs=(0,))
    grid(b, 12, 6, kfs=(1,), first_cell=30)
    grid(b, 3, 1, kfs=(2,), first_cell=60)
    st = b.st
    pts, segs = st["kf_pt"][1], st["kf_seg"][1]
    st["pt_type"][pts[5]] = D; st["pt_type"][pts[7]] = C_
    st["seg_type"][segs[2]] = D; st["seg_type"][segs[4]] = C_
    for at in (0, 4, 9, len(pts) + 3):
        pts.insert(at, -1)
    for at in (0, 3, len(segs) + 2):
        segs.insert(at, -1)
    return b.done()


@functools.lru_cache(maxsize=None)
def shared():
    """landmarks observed in both keyframes, the OTHER keyframe's observation first in their lists; a landmark that is a feature of
    keyframe 1 twice (its first observation in that keyframe serves both); features of keyframe 1 without an observation in it"""
    b = A.Builder(A.SMALL, 2)
    grid(b, 8, 4, kfs=(0, 1))                          # observation lists: keyframe 0 first
    grid(b, 3, 2, kfs=(1, 0), first_cell=40)           # keyframe 1 first
    st = b.st
    p, s = st["kf_pt"][1], st["kf_seg"][1]
    p.insert(2, p[6]); s.insert(1, s[3])               # twice
    lone_p = b.pt(*A.cell_px(A.SMALL, 70), kfs=(0,))   # observed in keyframe 0 alone, yet features of keyframe 1
    lone_s = b.seg((200.5, 40.125), (215.5, 44.125), kfs=(0,))
    p.insert(5, lone_p); s.insert(2, lone_s)
    # a second observation of one landmark in keyframe 1 with other pixels: the first one is the pairing
    lm = p[0]
    o = dict(st["pt_obs"][lm][1]); o["px"] = [o["px"][0] + 3.0, o["px"][1] - 2.0]
    st["pt_obs"][lm].append(o)
    return b.done()


@functools.lru_cache(maxsize=None)
def kept_points(n):
    """n kept point features in keyframe 0 (64, 65, 70: the rounds of the ballot prefix), a -1 and a deleted landmark among them"""
    b = A.Builder(A.SMALL, 2)
    grid(b, n + 1, 3, kfs=(0,), first_cell=8)
    st = b.st
    st["pt_type"][st["kf_pt"][0][20]] = D
    st["kf_pt"][0].insert(40, -1)
    return b.done()


@functools.lru_cache(maxsize=None)
def only(n_pt, n_seg):
    b = A.Builder(A.SMALL, 2)
    grid(b, n_pt, n_seg, kfs=(1,))
    grid(b, 2, 1, kfs=(0,), first_cell=50)
    return b.done()


@functools.lru_cache(maxsize=None)
def wide_lines():
    """the wide camera: segments of 64 and 65 samples at level 1 as features of keyframe 0"""
    b = A.Builder(A.WIDE, 2)
    for k in range(5):
        b.pt(45.5 + 30 * k, 45.125)
    for x0, length, y in ((40, 2040, 40.125), (40, 2072, 56.125)):
        b.seg((x0 + 0.5, y), (x0 + 0.5 + length, y))
    return b.done()


@functools.lru_cache(maxsize=None)
def overflow_batch():
    """under OVERFLOW_CFG: 21 kept points (cap_pts 20), 21 segment features (cap_seg 20), 76 + a round of slots (slot_cap 80), one that fits"""
    def lines(n_pt, ls):
        b = A.Builder(A.SMALL, 2)
        grid(b, n_pt, 0, kfs=(0,))
        for x0, length, y in ls:
            b.seg((x0 + 0.5, y), (x0 + 0.5 + length, y), kfs=(0,))
        return b.done()
    many_seg = A.Builder(A.SMALL, 2)
    grid(many_seg, 5, 18, kfs=(0,))
    many_seg.st["kf_seg"][0] += [-1, -1, -1]
    return (lines(21, []), many_seg.done(), lines(10, [(50, 200, 30.125 + 25 * k) for k in range(8)]), lines(10, [(50, 200, 105.125)]))


OVERFLOW_CFG = dict(cap_pts=20, cap_seg=20, slot_cap=80)


def far_T(dx):
    """a frame pose without rotation whose camera centre lies dx along x"""
    return [0.0, 0.0, 0.0, 1.0, -float(dx), 0.0, 0.0]


@functools.lru_cache(maxsize=None)
def three_keyframes():
    """three keyframes at centres -0.06, -0.03, 0.0 along x with features of their own, all in view of a frame near them"""
    b = A.Builder(A.SMALL, 3)
    for k in range(3):
        grid(b, 7, 2, kfs=(k,), first_cell=11 + 14 * k)
    return b.done()


@functools.lru_cache(maxsize=None)
def tiny(k):
    b = A.Builder(A.SMALL, 2)
    grid(b, 2 + k % 3, 1 + k % 2, kfs=(k % 2,), first_cell=20 + k % 5)
    return b.done()


def gate_counts():
    """(n_matches, n_ls_matches, num_obs_pt, num_obs_ls, num_obs_last_pt, num_obs_last_ls) around every threshold at quality_min_fts 20,
    quality_max_drop_fts 50, max_fts 100 / 100"""
    return dict(
        matched_19=(12, 7, 12, 7, 12, 7), matched_20=(12, 8, 12, 8, 12, 8),
        edges_9=(30, 10, 6, 3, 30, 10), edges_10=(30, 10, 6, 4, 30, 10), edges_19=(30, 10, 12, 7, 30, 10), edges_20=(30, 10, 12, 8, 30, 10),
        drop_50=(40, 10, 30, 10, 80, 10), drop_51=(40, 10, 29, 10, 80, 10),
        clamp=(60, 10, 50, 10, 400, 10),               # min(400, 100) - 50 = 50: not above the limit; unclamped it would be 350
        clamp_above=(60, 10, 49, 10, 400, 10),
        seg_drop_alone=(40, 30, 40, 5, 40, 90),        # the segments' drop of 85 is reported and decides nothing
        nothing=(0, 0, 0, 0, 0, 0))
