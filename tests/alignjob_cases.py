"""Cases of the alignment job built on the device from the resident selection (plsvo_candidates_align_build), shared by
tests/test_gpu_alignjob.py and tests/test_alignjob_host.py.  A stream is the dict of tests/candidates_cases.py with the counters of
np_select.quality(); the new frame sits at the origin without rotation, so a landmark's pixel in it is chosen directly, and every
landmark sits in grid cells of its own and is found, so that it becomes a feature of the new frame.  The matcher's results are inputs
(select_cases.match_of: the projection shifted by a fixed amount), and so are the keep masks where the pose optimiser would not produce
the pattern.

Two cameras: the 326 x 246 one of tests/select_cases.py, and a WIDE one of 2176 x 96 pixels for the segment packing -- a segment has
N = 1 + (length / 16 - 1) / 2^level samples when it runs along an image axis, so 64 and 65 samples at level 1 take 2032 and 2064 pixels
(the lengths here lie half a step above a threshold).
Pyramids of four levels, alignment over levels 3 .. 1.  Built once (seeded), never changed."""
import functools

import numpy as np

import candidates_cases as Cc
import insert_cases as Ic
import np_keyframe as K
import np_select as S
import select_cases as Sc

abi = Cc.abi
G = Sc.G
MAX_LEVEL, MIN_LEVEL, N_PYR = 3, 1, 4
SMALL = dict(cam_t=Sc.CAM_T, cell=Sc.CELL, seg_cell=Sc.SEG_CELL, boundary=Sc.BOUNDARY)
WIDE_T = (256.0, 256.0, 1088.0, 48.0, 2176, 96)
WIDE = dict(cam_t=WIDE_T, cell=30, seg_cell=25, boundary=8)
PARAMS = Ic.PARAMS
T_REF = [0.002, -0.001, 0.0015, 0.99999675, 0.03, -0.01, 0.02]   # a reference pose handed over by the host (copied, never normalised)


def cfg(cap_pts=96, cap_seg=40, slot_cap=512, n_iter=30):
    return dict(max_level=MAX_LEVEL, min_level=MIN_LEVEL, cap_pts=cap_pts, cap_seg=cap_seg, slot_cap=slot_cap, n_iter=n_iter)


def images(cam_t, n, seed=0):
    """n frames of one smooth random texture, each shifted by a pixel against the one before"""
    w, h = int(cam_t[4]), int(cam_t[5])
    rng = np.random.default_rng(7300 + seed)
    coarse = rng.uniform(30, 220, ((h + 40) // 4 + 2, (w + 40) // 4 + 2))
    big = np.kron(coarse, np.ones((4, 4)))
    big = (big + np.roll(big, 1, 0) + np.roll(big, 1, 1) + np.roll(big, 2, 0) + np.roll(big, 2, 1)) / 5.0 + rng.uniform(-6, 6, big.shape)
    return [np.clip(big[8 + k:8 + k + h, 8 + 2 * k:8 + 2 * k + w], 0, 255).astype(np.uint8) for k in range(n)]


class Builder:
    """one stream under either camera: keyframes next to the new frame, every observation gives has_view 1"""

    def __init__(self, geo, n_kf=2):
        self.geo, self.cam = geo, geo["cam_t"]
        self.kf_T = [Cc.kf_at(Ic.kf_centre(k)) for k in range(n_kf)]
        self.st = S.quality(Cc.empty_stream(self.kf_T))
        self.found_pt, self.found_seg = {}, {}

    def pos_at(self, px, py, z=4.0):
        c = self.cam
        return [(px - c[2]) / c[0] * z, (py - c[3]) / c[1] * z, float(z)]

    def observe(self, kf, pos, level=0):
        c = self.cam
        p = K.se3_act(self.kf_T[kf], pos)
        n = K.norm3(*p)
        return dict(kf=kf, px=[c[0] * p[0] / p[2] + c[2], c[1] * p[1] / p[2] + c[3]], f=[p[0] / n, p[1] / n, p[2] / n], level=level, type=0, grad=[1.0, 0.0])

    def pt(self, px, py, found=1, kfs=(0,), typ=G):
        pos = self.pos_at(px, py)
        lm = Cc.add_pt(self.st, pos, typ, [self.observe(k, pos, level=(len(self.st["pt_pos"]) + k) % 2) for k in kfs])
        self.st["pt_nfail"].append(0); self.st["pt_nsucc"].append(0)
        for k in kfs:
            self.st["kf_pt"][k].append(lm)
        self.found_pt[lm] = int(found)
        return lm

    def seg(self, s, e, found=(1, 1), kfs=(0,), typ=G):
        sp, ep = self.pos_at(*s), self.pos_at(*e)
        obs = []
        for k in kfs:
            a, b = self.observe(k, sp), self.observe(k, ep)
            obs.append(dict(kf=k, spx=a["px"], epx=b["px"], sf=a["f"], ef=b["f"], level=(len(self.st["seg_spos"]) + k) % 2))
        lm = Cc.add_seg(self.st, sp, ep, typ, obs)
        self.st["seg_nfail"].append(0); self.st["seg_nsucc"].append(0)
        for k in kfs:
            self.st["kf_seg"][k].append(lm)
        self.found_seg[lm] = (int(found[0]), int(found[1]))
        return lm

    def done(self):
        return dict(st=self.st, T=list(Cc.IDENT), overlap=tuple(range(len(self.kf_T))), found_pt=self.found_pt, found_seg=self.found_seg, geo=self.geo)


def cell_px(geo, cell, seg=False, dx=0.5, dy=0.5):
    size = geo["seg_cell"] if seg else geo["cell"]
    cols = -(-int(geo["cam_t"][4]) // size)
    return (cell % cols) * size + size // 2 + dx, (cell // cols) * size + size // 2 + dy


# ---- the small camera ---------------------------------------------------------------------------------------------------------------
def small(n_pt, n_seg, double_seg=(), first_cell=11):
    """n_pt points in cells of their own (the grid has 88 whole cells), n_seg short segments inside one cell each; `double_seg`: segments that span two
    cells and win both (a feature twice)"""
    b = Builder(SMALL)
    for k in range(n_pt):
        b.pt(*cell_px(SMALL, k + first_cell), kfs=(k % 2,))
    cells = iter(c for c in range(16, 126, 2) if 2 <= c % 14 <= 10)
    for k in range(n_seg):
        if k in double_seg:
            c = next(cells)
            while c % 14 > 8:
                c = next(cells)
            next(cells)
            b.seg(cell_px(SMALL, c, True), cell_px(SMALL, c + 2, True), kfs=(k % 2,))
        else:
            p = cell_px(SMALL, next(cells), True)
            b.seg((p[0] - 4, p[1]), (p[0] + 4, p[1] + 2), kfs=(k % 2,))
    return b.done()


@functools.lru_cache(maxsize=None)
def eighty():
    """80 point features (more than a round of 64) and 12 segments, two of them doubly won"""
    return small(80, 12, double_seg=(3, 8), first_cell=8)


@functools.lru_cache(maxsize=None)
def only_points():
    return small(9, 0)


@functools.lru_cache(maxsize=None)
def only_segments():
    return small(0, 5, double_seg=(1,))


@functools.lru_cache(maxsize=None)
def nothing_found():
    """landmarks in view, none matched: the new frame has no feature at all (skip)"""
    s = small(6, 3)
    s["found_pt"] = {k: 0 for k in s["found_pt"]}
    s["found_seg"] = {k: (0, 0) for k in s["found_seg"]}
    return s


def no_map():
    return Builder(SMALL, 0).done()


@functools.lru_cache(maxsize=None)
def border():
    """long segments in the small image; one ends at x = 20: 2 at level 3 (inside the 3-pixel border), 5 at level 2, 10 at level 1"""
    b = Builder(SMALL)
    for k in range(5):
        b.pt(*cell_px(SMALL, 12 + 2 * k))
    b.seg((20.5, 100.125), (250.5, 110.125))          # (match_of moves an end by (-0.5, +0.375))
    b.seg((40.5, 150.125), (280.5, 150.125))
    b.seg((60.5, 60.125), (60.5, 200.125))
    return b.done()


def small_lines(n_pt, lines):
    """lines: (x0, length, y) of horizontal segments, each in seg-grid cells of its own: it wins both of them and is a feature twice, of
    1 + (length / 16 - 1) / 2^level samples"""
    b = Builder(SMALL)
    for k in range(n_pt):
        b.pt(*cell_px(SMALL, k + 11))
    for x0, length, y in lines:
        b.seg((x0 + 0.5, y), (x0 + 0.5 + length, y))
    return b.done()


@functools.lru_cache(maxsize=None)
def overflow_batch():
    """under OVERFLOW_CFG: 30 points (cap_pts), 24 segment features (cap_seg), 16 segment features of 6 samples at level 1 behind 10
    points (64 + 96 slots in rounds of 60: slot_cap), and a stream that fits (10 points, 2 features of 6: 76 slots)"""
    return (small(30, 2), small_lines(5, [(30 if k < 6 else 160, 100, 30.125 + 25 * (k % 6)) for k in range(12)]),
            small_lines(10, [(50, 200, 30.125 + 25 * k) for k in range(8)]), small_lines(10, [(50, 200, 105.125)]))


OVERFLOW_CFG = dict(cap_pts=20, cap_seg=20, slot_cap=80)


@functools.lru_cache(maxsize=None)
def tiny(k):
    """a few features: the streams of the large batch"""
    return small(2 + k % 3, 1 + k % 2, double_seg=(0,) if k % 2 else (), first_cell=20 + k % 5)


# ---- the wide camera ----------------------------------------------------------------------------------------------------------------
def wide(n_pt, lines):
    """lines: (x0, length, y) of horizontal segments; each wins both its cells, so it is a feature twice: equal N, ties in feature order"""
    b = Builder(WIDE)
    for k in range(n_pt):
        b.pt(45.5 + 30 * k, 45.125)
    for x0, length, y in lines:
        b.seg((x0 + 0.5, y), (x0 + 0.5 + length, y))
    return b.done()


@functools.lru_cache(maxsize=None)
def sixty_four_and_five():
    """2040 pixels: 64 samples at level 1 (a round of its own); 2072 pixels: 65 (long at level 1, 33 at level 2: short there)"""
    return wide(5, ((40, 2040, 40.125), (40, 2072, 56.125)))


@functools.lru_cache(maxsize=None)
def third_round():
    """eight shorts of 40, 40, 30, 30, 20, 20, 10, 10 samples at level 1, given out of order: first-fit in decreasing N fills
    40 + 20, 40 + 20, 30 + 30 and opens a fourth round for 10 + 10"""
    return wide(7, ((100, 16 * 19 + 8, 32.125), (150, 16 * 79 + 8, 40.125), (200, 16 * 39 + 8, 48.125), (250, 16 * 59 + 8, 56.125)))


@functools.lru_cache(maxsize=None)
def equal_n():
    """three segments of equal length (six features of equal N at every level) and one shorter: the tie order is the feature order"""
    return wide(3, ((60, 16 * 25 + 8, 30.125), (700, 16 * 25 + 8, 38.125), (1400, 16 * 25 + 8, 46.125), (300, 16 * 9 + 8, 58.125)))


@functools.lru_cache(maxsize=None)
def long_only():
    """no short at level 1: two long segments right behind the points' round"""
    return wide(2, ((40, 2072, 40.125), (40, 2104, 56.125)))


@functools.lru_cache(maxsize=None)
def seventy_rounds():
    """no points; 32 lines of 40 samples at level 1 (64 features: a round each, the whole first bin group), two of 33 (four more rounds, in
    the second group) and one of 30, whose two features fit nowhere in the first group and are placed in the second group's first two rounds"""
    lines = [(25 * c + 5, 16 * 79 + 8, 30.125 + 25 * r) for r in range(2) for c in range(1, 17)]
    lines += [(25 * 26 + 5, 16 * 65 + 8, 30.125), (25 * 27 + 5, 16 * 65 + 8, 30.125), (25 * 30 + 5, 16 * 59 + 8, 55.125)]
    return wide(0, lines)


@functools.lru_cache(maxsize=None)
def beyond_the_bins():
    """68 lines of 33 samples at level 1 in four rows of the segments' grid: 136 features, a round each -- more than the 128 rounds the
    shorts of a level may open: the level cannot be laid out and the stream is dropped"""
    return wide(0, [(25 * c + 5, 16 * 65 + 8, 12.125 + 25 * r) for r in range(4) for c in range(1, 18)])
