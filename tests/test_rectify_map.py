"""plsvo_rectify_map (host only, no device) against the NumPy restatement of OpenCV's initUndistortRectifyMap (tests/np_rectify.py),
bit for bit, and the NumPy remap's own invariants.

Sensitivity of the unpinned part: OpenCV accumulates `_x += ir[0]` (and _y, _w) along a row.  Evaluating `j*ir[0] + (i*ir[1] + ir[2])`
instead changes 0 of the 360 960 map entries of EuRoC cam0 and 0 of the 307 200 of the TUM-like camera below (asserted in
test_accumulated_row_sum_sensitivity): with K's inverse the running sum's rounding stays far below the 1/32-pixel grid of the map."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import np_rectify as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EUROC = dict(width=752, height=480, fx=458.654, fy=457.296, cx=367.215, cy=248.375, d=[-0.28340811, 0.07395907, 1.9359e-4, 1.76187114e-5])
TUM = dict(width=640, height=480, fx=517.306408, fy=516.469215, cx=318.643040, cy=255.313989, d=[0.262383, -0.953104, -0.005358, 0.002628, 1.163314])
CAMERAS = {
    "euroc_cam0": EUROC,
    "tum_like": TUM,
    "strong_barrel": dict(width=320, height=240, fx=180.0, fy=181.5, cx=161.3, cy=118.7, d=[-0.45, 0.22, 0.0, 0.0, -0.05]),
    "pincushion": dict(width=320, height=240, fx=250.0, fy=250.0, cx=160.0, cy=120.0, d=[0.35, 0.12, 0.001, -0.002]),
    "nonzero_k3": dict(width=256, height=192, fx=200.2, fy=199.7, cx=127.9, cy=96.4, d=[-0.1, 0.03, 0.0005, 0.0007, 0.02]),
    "odd_size": dict(width=157, height=93, fx=120.3, fy=121.1, cx=77.9, cy=46.2, d=[-0.2, 0.05, 0.002, -0.001, 0.001]),
    "odd_tiny": dict(width=1, height=3, fx=10.0, fy=10.0, cx=0.2, cy=1.1, d=[-0.3, 0.0, 0.0, 0.0]),
}


def lib_map(P, c):
    return P.capi.rectify_map(P.abi.pinhole_radtan(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], c["d"]))


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_map_equals_numpy_bit_for_bit(P, name):
    c = CAMERAS[name]
    xy, fr = lib_map(P, c)
    nxy, nfr = R.rectify_map(c)
    assert xy.shape == (c["height"], c["width"], 2) and fr.shape == (c["height"], c["width"])
    assert np.array_equal(xy, nxy), f"{name}: {(xy != nxy).any(-1).sum()} tap positions differ"
    assert np.array_equal(fr, nfr), f"{name}: {(fr != nfr).sum()} fractions differ"


def test_euroc_map_is_plausible(P):
    xy, fr = lib_map(P, EUROC)
    # barrel distortion (k1 < 0): a rectified corner samples well inside the raw frame, the centre barely moves
    assert 10 < xy[0, 0, 0] < 367 and 10 < xy[0, 0, 1] < 248
    cy, cx = 248, 367
    assert abs(int(xy[cy, cx, 0]) - cx) <= 1 and abs(int(xy[cy, cx, 1]) - cy) <= 1
    assert fr.max() <= 1023


def test_parameters_equal_in_float_give_identical_maps(P):
    c = dict(CAMERAS["odd_size"])
    c3 = dict(c, fx=float(np.float32(c["fx"])), fy=float(np.float32(c["fy"])), cx=float(np.float32(c["cx"])), cy=float(np.float32(c["cy"])),
              d=[float(np.float32(v)) for v in c["d"]])
    a, b, e = lib_map(P, c), lib_map(P, c3), lib_map(P, dict(c, d=[float(np.float32(v)) for v in c["d"]]))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0], e[0]) and np.array_equal(a[1], e[1])
    # a parameter that differs in float does change the map
    f = lib_map(P, dict(c, fx=c["fx"] * 1.01))
    assert not np.array_equal(a[0], f[0])


def test_zero_distortion_map_is_the_identity(P):
    for w, h in ((77, 33), (640, 480), (752, 480)):
        c = dict(width=w, height=h, fx=300.7, fy=299.1, cx=w / 2 + 0.3, cy=h / 2 - 0.2, d=[0, 0, 0, 0, 0])
        xy, fr = lib_map(P, c)
        jj, ii = np.meshgrid(np.arange(w), np.arange(h))
        assert np.array_equal(xy[..., 0], jj) and np.array_equal(xy[..., 1], ii) and not fr.any()


def test_accumulated_row_sum_sensitivity():
    """the count the module docstring records: OpenCV's running sum vs j*ir[0] (the part of the contract no upstream binary pins)"""
    for c in (EUROC, TUM):
        a, b = R.rectify_map(c), R.rectify_map(c, accumulate=False)
        diff = ((a[0] != b[0]).any(-1) | (a[1] != b[1])).sum()
        assert diff == 0, diff


def test_bad_cameras_are_rejected_and_nothing_is_written(P):
    L = P.capi.lib()
    good = CAMERAS["odd_size"]
    bad = [dict(good, fx=float("nan")), dict(good, cy=float("inf")), dict(good, d=[float("nan"), 0, 0, 0]), dict(good, d=[0, 0, 0, 0, float("inf")]),
           dict(good, fx=1e300), dict(good, fy=0.0), dict(good, width=0), dict(good, height=-2), dict(good, width=2047), dict(good, height=2047)]
    for c in bad:
        cam = P.abi.pinhole_radtan(c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], c["d"])
        xy = np.full(good["width"] * good["height"] * 2, 7, dtype=np.int16)
        fr = np.full(good["width"] * good["height"], 9, dtype=np.uint16)
        rc = L.plsvo_rectify_map(C.byref(cam), xy.ctypes.data_as(C.POINTER(C.c_int16)), fr.ctypes.data_as(C.POINTER(C.c_uint16)))
        assert rc == P.abi.E_INVALID, c
        assert (xy == 7).all() and (fr == 9).all()
    assert L.plsvo_rectify_map(None, None, None) == P.abi.E_INVALID


def test_largest_addressable_size_builds(P):
    c = dict(width=2046, height=8, fx=900.0, fy=900.0, cx=1022.5, cy=3.5, d=[-0.1, 0.0, 0.0, 0.0])
    xy, fr = lib_map(P, c)
    nxy, nfr = R.rectify_map(c)
    assert np.array_equal(xy, nxy) and np.array_equal(fr, nfr)


def test_pinhole_radtan_struct_matches_the_c_header(P, tmp_path):
    header = os.path.join(ROOT, "include", "plsvo_hip.h")
    src = tmp_path / "l.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{header}"\nint main(void){{printf("%zu %zu %zu %d\\n", sizeof(plsvo_pinhole_radtan), '
                   f'offsetof(plsvo_pinhole_radtan, cam), offsetof(plsvo_pinhole_radtan, d), PLSVO_MAX_RECTIFY_MAPS);return 0;}}\n')
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "l"), str(src)], check=True)
    size, off_cam, off_d, nmaps = map(int, subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.split())
    assert size == C.sizeof(P.abi.PinholeRadtan) and off_cam == P.abi.PinholeRadtan.cam.offset and off_d == P.abi.PinholeRadtan.d.offset
    assert nmaps >= 2


# ---- the NumPy remap's own invariants (the GPU tests compare the device against it) ----

def test_interpolation_table_entries():
    tab = R.inter_tab_linear()
    assert tab[0].tolist() == [32767, 0, 0, 1]
    for ty in (0, 5, 31):
        for tx in (1, 16, 31):
            assert tab[ty * 32 + tx].tolist() == [(32 - ty) * (32 - tx) * 32, (32 - ty) * tx * 32, ty * (32 - tx) * 32, ty * tx * 32]


def test_remap_identity_map_copies_and_border_reads_zero():
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 256, (9, 13), dtype=np.uint8)
    jj, ii = np.meshgrid(np.arange(13), np.arange(9))
    xy = np.stack([jj, ii], -1).astype(np.int16)
    assert np.array_equal(R.remap_bilinear(raw, xy, np.zeros((9, 13), np.uint16)), raw)
    # half a pixel to the right of the last column: half the pixel, half the constant border 0
    xy2 = np.array([[[12, 4]]], dtype=np.int16)
    out = R.remap_bilinear(raw, xy2, np.array([[16]], np.uint16))
    assert int(out[0, 0]) == (int(raw[4, 12]) * 16 * 32 * 32 + (1 << 14)) >> 15
    assert R.remap_bilinear(raw, np.array([[[-5, 2]]], np.int16), np.array([[7]], np.uint16))[0, 0] == 0


def test_identity_branch_ignores_d1_to_d4():
    rng = np.random.default_rng(4)
    raw = rng.integers(0, 256, (24, 31), dtype=np.uint8)
    c = dict(width=31, height=24, fx=30.0, fy=30.0, cx=15.0, cy=12.0, d=[0.0, 0.4, 0.01, 0.01, 0.2])
    assert np.array_equal(R.undistort(raw, c), raw)
    assert np.array_equal(R.undistort(raw, c, flip=True), raw[::-1])
    c2 = dict(c, d=[2e-7] + c["d"][1:])
    assert not np.array_equal(R.undistort(raw, c2), raw)
