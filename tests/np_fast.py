"""NumPy restatement of the corner detector's contract: what feature_detection::FastDetector::detect
(src/feature_detection.cpp:53-104) computes with fast_corner_detect_10 / fast_corner_score_10 / fast_nonmax_3x3 ([ext] fast) and
vk::shiTomasiScore ([ext] vikit).  Neither library is vendored, so this is a restatement from knowledge of upstream and parity with the
reference binaries is unpinned; the device code is checked against THIS file, bit for bit.

Two forms of the two FAST steps are kept side by side: the literal ones (a per-pixel segment test, upstream's binary search for the
score) and the vectorised closed forms the tests run on whole images; tests/test_detect_host.py asserts they agree."""
import math

import numpy as np

# the 16 Bresenham offsets of radius 3 (dx, dy), circular, from (0, 3)
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
CORNER_DTYPE = np.dtype([("x", np.int32), ("y", np.int32), ("score", np.float32), ("level", np.int32)])


# ---- literal forms (one pixel at a time) ------------------------------------------------------------------------------------------
def is_corner_literal(img, x, y, b):
    """the segment test of fast_corner_detect_10 at threshold b: 10 contiguous ring pixels all > p + b, or all < p - b (strict, integers)"""
    h, w = img.shape
    if not (3 <= x < w - 3 and 3 <= y < h - 3):
        return False
    p = int(img[y, x])
    ring = [int(img[y + dy, x + dx]) for dx, dy in RING]
    for s in range(16):
        arc = [ring[(s + k) % 16] for k in range(10)]
        if all(v > p + b for v in arc) or all(v < p - b for v in arc):
            return True
    return False


def score_search_literal(img, x, y, b):
    """fast_corner_score_10 for a corner at threshold b: upstream's binary search (bmin = b, bmax = 255)"""
    bmin, bmax = b, 255
    t = (bmax + bmin) // 2
    while True:
        if is_corner_literal(img, x, y, t):
            bmin = t
        else:
            bmax = t
        if bmin == bmax - 1 or bmin == bmax:
            return bmin
        t = (bmin + bmax) // 2


# ---- closed forms on a whole image ----------------------------------------------------------------------------------------------------
def _arc_strength(img):
    """t[y, x] = max over the 32 arcs (16 starts, 2 signs) of the min over the arc's 10 pixels of +-(ring - p); -256 within 3 px of the border"""
    h, w = img.shape
    t = np.full((h, w), -256, dtype=np.int32)
    if h < 7 or w < 7:
        return t
    I = img.astype(np.int32)
    p = I[3:h - 3, 3:w - 3]
    d = np.stack([I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - p for dx, dy in RING])          # [16, h-6, w-6]
    best = np.full(p.shape, -256, dtype=np.int32)
    for s in range(16):
        arc = d[[(s + k) % 16 for k in range(10)]]
        best = np.maximum(best, np.maximum(arc.min(axis=0), (-arc).min(axis=0)))
    t[3:h - 3, 3:w - 3] = best
    return t


def corner_map(img, b):
    """bool [h, w]: the set fast_corner_detect_10 returns"""
    return _arc_strength(img) > b


def score_map(img, b):
    """uint8 [h, w]: fast_corner_score_10 of every corner (in [b, 254]), 0 where the pixel is no corner"""
    t = _arc_strength(img)
    return np.where(t > b, t - 1, 0).astype(np.uint8)


def nonmax_map(score):
    """fast_nonmax_3x3 on a score map (0 = no corner): a corner survives iff no 8-neighbour that is a corner scores >= it"""
    h, w = score.shape
    s = np.zeros((h + 2, w + 2), dtype=np.int32)
    s[1:-1, 1:-1] = score
    c = s[1:-1, 1:-1]
    keep = c > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= s[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx] < c
    return keep


def shi_tomasi(img, u, v):
    """vk::shiTomasiScore(img, u, v) -> np.float32"""
    h, w = img.shape
    if u - 4 < 1 or u + 4 >= w - 1 or v - 4 < 1 or v + 4 >= h - 1:
        return np.float32(0.0)
    I = img.astype(np.int64)
    dx = I[v - 4:v + 4, u - 3:u + 5] - I[v - 4:v + 4, u - 5:u + 3]
    dy = I[v - 3:v + 5, u - 4:u + 4] - I[v - 5:v + 3, u - 4:u + 4]
    sxx, syy, sxy = int((dx * dx).sum()), int((dy * dy).sum()), int((dx * dy).sum())
    assert max(sxx, syy, abs(sxy)) < 2 ** 24          # upstream's float sums are exact
    # float sums divided by 2.0 * 64 and stored as float (exact), then double arithmetic in upstream's order
    a, b, c = (float(np.float32(np.float32(q) / np.float32(128.0))) for q in (sxx, syy, sxy))
    s = a + b
    return np.float32(0.5 * (s - math.sqrt(s * s - 4.0 * (a * b - c * c))))


# ---- the grid -----------------------------------------------------------------------------------------------------------------------
def grid(width, height, cell):
    return -(-width // cell), -(-height // cell)


def cell_index(cols, cell, px_x, px_y):
    """FastDetector::setGridOccpuancy's index (src/feature_detection.cpp:115-121)"""
    return int(px_y / cell) * cols + int(px_x / cell)


def survivors(level_img, b):
    """[(x, y)] of one level in raster order"""
    ys, xs = np.nonzero(nonmax_map(score_map(level_img, b)))
    return list(zip(xs.tolist(), ys.tolist()))


def detect(levels, cell=25, b=20, detection_threshold=20.0, occupancy=None, stats=None):
    """FastDetector::detect on a pyramid (list of uint8 images, level 0 first): records (CORNER_DTYPE) in cell-index order.
    stats (a dict) receives `ties`: survivors that met a cell entry of exactly their own score."""
    h0, w0 = levels[0].shape
    cols, rows = grid(w0, h0, cell)
    thr = np.float32(detection_threshold)
    assert float(thr) == detection_threshold >= 0.0
    best = [(thr, None)] * (cols * rows)
    ties = 0
    for L, img in enumerate(levels):
        for x, y in survivors(img, b):
            k = ((y << L) // cell) * cols + ((x << L) // cell)
            if occupancy is not None and occupancy[k]:
                continue
            st = shi_tomasi(img, x, y)
            if best[k][1] is not None and st == best[k][0]:
                ties += 1
            if st > best[k][0]:
                best[k] = (st, (x << L, y << L, L))
    if stats is not None:
        stats["ties"] = ties
    out = [(c[0], c[1], s, c[2]) for s, c in best if c is not None]
    return np.array(out, dtype=CORNER_DTYPE)
