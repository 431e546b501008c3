"""The corner detector's contract without a GPU: the NumPy restatement (tests/np_fast.py) is consistent with itself -- upstream's
literal binary search for the score equals the closed form the kernel uses, the vectorised corner test equals a per-pixel segment test
-- the host-only grid helpers of the C ABI equal the NumPy values, a hand-made image has the answers worked out by hand, and
sequence.seeds_from_corners gives the PointSeed constructor's values."""
import numpy as np
import pytest

import np_fast as F


def test_literal_score_search_equals_closed_form_on_noise():
    img = np.random.default_rng(3).integers(0, 256, (60, 80), dtype=np.uint8)
    score = F.score_map(img, 20)
    corners = F.corner_map(img, 20)
    assert np.array_equal(corners, score > 0) and corners.sum() > 500
    ys, xs = np.nonzero(corners)
    mismatches = sum(int(F.score_search_literal(img, x, y, 20) != score[y, x]) for x, y in zip(xs.tolist(), ys.tolist()))
    assert mismatches == 0
    assert score[corners].min() >= 20 and score.max() <= 254


@pytest.mark.parametrize("b", [20, 1, 90])
def test_corner_map_equals_literal_segment_test(b):
    img = np.random.default_rng(4).integers(0, 256, (40, 50), dtype=np.uint8)
    cm = F.corner_map(img, b)
    lit = np.array([[F.is_corner_literal(img, x, y, b) for x in range(50)] for y in range(40)])
    assert np.array_equal(cm, lit) and 0 < cm.sum() < cm.size
    assert not cm[:3].any() and not cm[-3:].any() and not cm[:, :3].any() and not cm[:, -3:].any()


@pytest.mark.parametrize("w,h,cell", [(157, 93, 25), (157, 93, 30), (640, 480, 25), (752, 480, 30), (150, 100, 25), (7, 7, 100), (8191, 13, 1)])
def test_grid_helpers_equal_numpy(P, w, h, cell):
    cols, rows = P.capi.detect_grid(w, h, cell)
    assert (cols, rows) == F.grid(w, h, cell) == (int(np.ceil(w / cell)), int(np.ceil(h / cell)))
    rng = np.random.default_rng(w + cell)
    pts = np.column_stack([rng.uniform(0, w, 200), rng.uniform(0, h, 200)]).tolist() + [(0.0, 0.0), (w - 1.0, h - 1.0), (cell, cell), (cell - 1e-9, cell * 2.0)]
    for x, y in [q for q in pts if q[0] < w and q[1] < h]:
        k = P.capi.detect_cell(cols, cell, x, y)
        assert k == F.cell_index(cols, cell, x, y) and 0 <= k < cols * rows


def test_grid_helpers_refuse_bad_arguments(P):
    import ctypes as C
    L = P.capi.lib()
    c, r = C.c_int(-5), C.c_int(-5)
    for a in ((0, 10, 5), (10, 0, 5), (10, 10, 0), (-1, 10, 5)):
        assert L.plsvo_detect_grid(*a, C.byref(c), C.byref(r)) == P.abi.E_INVALID
    assert L.plsvo_detect_grid(10, 10, 5, None, C.byref(r)) == P.abi.E_INVALID and (c.value, r.value) == (-5, -5)
    for a in ((0, 25, 1.0, 1.0), (7, 0, 1.0, 1.0), (7, 25, -1.0, 1.0), (7, 25, 1.0, float("nan")), (7, 25, float("inf"), 1.0)):
        assert L.plsvo_detect_cell(*a) == P.abi.E_INVALID
    with pytest.raises(P.capi.PlsvoError):
        P.capi.detect_grid(10, 10, 0)


def test_ctypes_mirrors_have_the_c_layouts(P, tmp_path):
    import ctypes as C
    import os
    import subprocess
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "plsvo_hip.h")
    structs = {"plsvo_corner": P.abi.Corner, "plsvo_detect_params": P.abi.DetectParams}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void){"]
    for cname, ct in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in ct._fields_]
    lines.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, ct in structs.items():
        assert int(got[cname]) == C.sizeof(ct)
        for f, _ in ct._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(ct, f).offset
    assert P.abi.CORNER_DTYPE.itemsize == C.sizeof(P.abi.Corner) == 16 and P.abi.CORNER_DTYPE == F.CORNER_DTYPE


def _field(w=64, h=48, v=255):
    return np.full((h, w), v, dtype=np.uint8)


def test_single_dark_pixel_scores_254():
    img = _field()
    img[20, 30] = 0
    score = F.score_map(img, 20)
    # the pixel itself: every ring pixel is 255 > 0 + b for every b <= 254
    assert score[20, 30] == 254 == F.score_search_literal(img, 30, 20, 20)
    # the 16 pixels that see it on their ring have ONE dark ring pixel: no arc of 10
    assert (score > 0).sum() == 1
    assert F.nonmax_map(score).sum() == 1
    st = F.shi_tomasi(img, 30, 20)
    # gradients: dx = -+255 at (29, 20), (31, 20), dy the same at (30, 19), (30, 21): dXX = dYY = 2 * 255^2 / 128, dXY = 0 -> min eigenvalue = dXX
    assert st == np.float32(2 * 255 * 255 / 128.0)
    got = F.detect([img], 25, 20, 20.0)
    assert len(got) == 1 and tuple(got[0]) == (30, 20, st, 0)


def test_two_adjacent_equal_corners_both_vanish():
    img = _field()
    img[20, 30] = 0
    img[20, 31] = 0
    score = F.score_map(img, 20)
    # each dark pixel has all 16 ring pixels bright (the other dark pixel is at distance 1, not on the ring)
    assert score[20, 30] == score[20, 31] == 254 and (score > 0).sum() == 2
    assert F.nonmax_map(score).sum() == 0
    assert len(F.detect([img], 25, 20, 0.0)) == 0
    # unequal neighbours: the weaker one goes, the stronger one stays
    img[20, 31] = 100
    score = F.score_map(img, 20)
    assert score[20, 30] == 254 and score[20, 31] == 154
    keep = F.nonmax_map(score)
    assert keep[20, 30] and not keep[20, 31]


def test_corner_near_the_border_has_no_shi_tomasi_score_and_yields_no_feature():
    img = _field()
    img[4, 30] = 0          # a FAST corner (y >= 3) whose 8 x 8 box would leave the image (v - 4 < 1)
    img[43, 10] = 0         # v + 4 >= h - 1
    img[20, 4] = 0          # u - 4 < 1
    img[20, 59] = 0         # u + 4 >= w - 1
    score = F.score_map(img, 20)
    assert (score > 0).sum() == 4 and F.nonmax_map(score).sum() == 4
    for x, y in ((30, 4), (10, 43), (4, 20), (59, 20)):
        assert F.shi_tomasi(img, x, y) == 0.0
    assert len(F.detect([img], 25, 20, 0.0)) == 0
    img[5, 30] = 0          # first row with a score: but now (30, 4) and (30, 5) are equal neighbours
    img[4, 30] = 255
    assert F.shi_tomasi(img, 30, 5) > 0 and len(F.detect([img], 25, 20, 0.0)) == 1


def test_cell_keeps_the_first_of_equal_scores_and_the_stronger_of_unequal():
    img = _field(100, 60)
    img[10, 10] = 0
    img[15, 18] = 0         # same cell (cell 25), same Shi-Tomasi score: the earlier in raster order stays
    img[40, 40] = 0
    img[45, 45] = 128       # same cell, weaker
    st = {}
    got = F.detect([img], 25, 20, 20.0, stats=st)
    assert [(r["x"], r["y"]) for r in got] == [(10, 10), (40, 40)] and st["ties"] == 1
    occ = np.zeros(12, np.uint8)
    occ[0] = 1
    assert [(r["x"], r["y"]) for r in F.detect([img], 25, 20, 20.0, occupancy=occ)] == [(40, 40)]


def test_seeds_from_corners_are_the_point_seed_constructor_values(P):
    f32 = np.float32
    cam = (315.5, 315.5, 376.0, 240.0, 752, 480)          # the harness carries the camera as (fx, fy, cx, cy, width, height)
    corners = np.array([(100, 50, 31.5, 0), (404, 236, 80.25, 1), (640, 400, 1000.0, 2)], dtype=F.CORNER_DTYPE)
    depth_mean, depth_min = 2.37, 0.61
    s = P.sequence.seeds_from_corners(corners, cam, depth_mean, depth_min)
    n = 3
    # PointSeed::PointSeed(ftr, float depth_mean, float depth_min) (src/depth_filter.cpp:53-61): a(10), b(10), mu(1.0 / depth_mean),
    # z_range(1.0 / depth_min) -- double divisions of the float arguments, stored as float -- and sigma2(z_range * z_range / 36) in float
    z = f32(1.0 / float(f32(depth_min)))
    assert s["a"].dtype == s["b"].dtype == s["mu"].dtype == s["z_range"].dtype == s["sigma2"].dtype == np.float32
    assert np.array_equal(s["a"], np.full(n, 10, f32)) and np.array_equal(s["b"], np.full(n, 10, f32))
    assert np.array_equal(s["mu"], np.full(n, f32(1.0 / float(f32(depth_mean))))) and np.array_equal(s["z_range"], np.full(n, z))
    assert np.array_equal(s["sigma2"], np.full(n, f32(z * z) / f32(36)))
    assert s["sigma2"][0].tobytes() == (f32(z * z) / f32(36)).tobytes()
    assert np.array_equal(s["px"], np.array([[100.0, 50.0], [404.0, 236.0], [640.0, 400.0]])) and s["px"].dtype == np.float64
    assert np.array_equal(s["level"], np.array([0, 1, 2], np.int32)) and np.array_equal(s["type"], np.zeros(n, np.uint8))
    for i in range(n):
        v = np.array([(corners["x"][i] - 376.0) / 315.5, (corners["y"][i] - 240.0) / 315.5, 1.0])
        assert np.allclose(s["f"][i], v / np.sqrt(v @ v), rtol=0, atol=1e-15)         # cam2world: the unit bearing vector (double)
    assert np.array_equal(s["grad"], np.tile([1.0, 0.0], (n, 1)))
    e = P.sequence.seeds_from_corners(corners[:0], cam, depth_mean, depth_min)
    assert all(len(v) == 0 for v in e.values())
