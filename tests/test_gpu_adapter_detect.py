"""The C++ drop-in for feature_detection::FastDetector (pl-svo_amd/host/plsvo/hip_adapter.hpp) on the GPU, through
pl-svo_amd/host/detect_driver: the feature list detect() appends equals the C ABI's records (position, level, order; f = cam2world(px)),
setExistingFeatures / setGridOccpuancy mask exactly the cells of the given features, and the grid is reset after every detect.
The driver links the product library, so the emulated run leaves this file out by name (tests/test_emu_parity.py)."""
import os
import subprocess

import numpy as np
import pytest

import np_fast as F
from test_gpu_detect import _scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "pl-svo_amd", "host", "detect_driver")
W, H, CELL, THR = 160, 120, 25, 20.0
CAM = (95.3, 96.1, 79.6, 60.2)


@pytest.fixture(scope="module")
def run(P, tmp_path_factory):
    assert os.path.exists(DRIVER), "build it with __graft_entry__.build()"
    ctx = P.capi.Context(0)
    ctx.config_pyramids(1, W, H, 3)
    ctx.build_pyramid(0, _scene(22))
    levels = ctx.download_pyramid(0)
    free = ctx.detect_fast(0, 1, CELL, 3, 20, THR)[0]
    # existing features: in the cells of every third detected feature (off the corner itself), and two in cells without a detection
    cols, rows = P.capi.detect_grid(W, H, CELL)
    taken = (free["y"] // CELL) * cols + free["x"] // CELL
    existing = [((k % cols) * CELL + 3.25, (k // cols) * CELL + 11.5) for k in taken[::3]]
    empty = [k for k in range(cols * rows) if k not in set(taken.tolist())][:2]
    existing += [((k % cols) * CELL + 0.0, (k // cols) * CELL + 0.5) for k in empty]
    occ_all = np.zeros(cols * rows, np.uint8)
    for x, y in existing:
        occ_all[P.capi.detect_cell(cols, CELL, x, y)] = 1
    occ_one = np.zeros(cols * rows, np.uint8)
    occ_one[P.capi.detect_cell(cols, CELL, *existing[0])] = 1
    want = dict(free=free, existing=ctx.detect_fast(0, 1, CELL, 3, 20, THR, occupancy=occ_all[None])[0],
                one=ctx.detect_fast(0, 1, CELL, 3, 20, THR, occupancy=occ_one[None])[0], reset=free)
    ctx.close()
    d = tmp_path_factory.mktemp("detect_driver")
    path, out = d / "in.bin", d / "out.txt"
    with open(path, "wb") as f:
        np.array([W, H, 3, 3, CELL, THR, len(existing)], dtype=np.float64).tofile(f)
        np.array(CAM, dtype=np.float64).tofile(f)
        for l in levels:
            np.ascontiguousarray(l, dtype=np.uint8).tofile(f)
        np.array(existing, dtype=np.float64).tofile(f)
    subprocess.run([DRIVER, str(path), str(out)], check=True, timeout=120)
    got = {}
    for line in open(out).read().splitlines():
        tag, *v = line.split()
        got.setdefault(tag, []).append([float(x) for x in v])
    return got, want, (cols, rows), occ_all, occ_one


def _check(rows, want):
    rows = np.array(rows).reshape(-1, 7)
    assert len(rows) == len(want)
    assert np.array_equal(rows[:, 0], want["x"]) and np.array_equal(rows[:, 1], want["y"]) and np.array_equal(rows[:, 2], want["level"])
    v = np.column_stack([(rows[:, 0] - CAM[2]) / CAM[0], (rows[:, 1] - CAM[3]) / CAM[1], np.ones(len(rows))])
    assert np.allclose(rows[:, 3:6], v / np.linalg.norm(v, axis=1)[:, None], rtol=0, atol=1e-15)      # f = cam2world(px), unit length
    assert np.all(rows[:, 6] == 1)                                                                     # Feature::frame is the frame


def test_fast_detector_feature_list_equals_the_c_abi_result(run):
    got, want, grid, _, _ = run
    assert got["grid"] == [[float(grid[0]), float(grid[1])]]
    assert len(want["free"]) >= 6 and np.all(np.bincount(want["free"]["level"], minlength=3) >= 1)
    _check(got["free"], want["free"])
    _check(got["reset"], want["free"])          # detect() resets the grid (src/feature_detection.cpp:103)


def test_set_existing_features_masks_the_right_cells(run):
    got, want, (cols, _), occ_all, occ_one = run
    _check(got["existing"], want["existing"])
    _check(got["one"], want["one"])
    ex = np.array(got["existing"]).reshape(-1, 7)
    k = (ex[:, 1] // CELL).astype(int) * cols + (ex[:, 0] // CELL).astype(int)
    assert not occ_all[k].any() and len(want["existing"]) < len(want["one"]) < len(want["free"])
    fk = (want["free"]["y"] // CELL) * cols + want["free"]["x"] // CELL
    assert len(ex) == int((occ_all[fk] == 0).sum()) and len(got["one"]) == int((occ_one[fk] == 0).sum()) == len(want["free"]) - 1
