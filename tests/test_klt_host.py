"""The NumPy restatement of the bootstrap's KLT track (tests/np_klt.py) against independent formulations, on the CPU:
the level rule, pyrDown and Scharr against dense correlations, the fixed-point weights, the exact integer sums, vk::getMedian's rank,
a sanity check that the restated tracker tracks, and the C structs against their ctypes mirrors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.ndimage as ndi

import klt_cases as Kc
import np_klt as K

A = Kc.abi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("plsvo_klt_reserve", "plsvo_klt_first_frame", "plsvo_klt_second_frame", "plsvo_klt_fetch", "plsvo_klt_fetch_tracks",
                "plsvo_klt_tracks_dev", "plsvo_klt_levels", "plsvo_klt_download_level", "plsvo_klt_track_points")


def test_level_rule():
    top = {(640, 480): 3, (320, 240): 2, (160, 120): 1, (61, 45): 0, (97, 71): 1}
    for (w, h), L in top.items():
        sizes = K.level_sizes(w, h)
        assert len(sizes) - 1 == L, (w, h)
        assert sizes == Kc.P.capi.klt_levels(w, h)                       # the library's host function agrees
        for (w0, h0), (w1, h1) in zip(sizes, sizes[1:]):
            assert (w1, h1) == ((w0 + 1) // 2, (h0 + 1) // 2)
    assert len(K.level_sizes(320, 240, max_level=1)) == 2 == len(Kc.P.capi.klt_levels(320, 240, 30, 1))
    assert len(K.level_sizes(4000, 3000)) == 5                           # the maxLevel cap
    with pytest.raises(Kc.P.capi.PlsvoError):
        Kc.P.capi.klt_levels(0, 10)
    with pytest.raises(Kc.P.capi.PlsvoError):
        Kc.P.capi.klt_levels(64, 64, 30, 5)


@pytest.mark.parametrize("w,h", [(97, 71), (61, 45), (64, 48), (33, 2)])
def test_pyr_down_and_scharr_against_dense_correlations(w, h):
    img = np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w)).astype(np.uint8)
    k = np.array([1, 4, 6, 4, 1], dtype=np.int64)
    dense = ndi.correlate(img.astype(np.int64), np.outer(k, k), mode="mirror")
    assert np.array_equal(K.pyr_down(img), ((dense[::2, ::2] + 128) >> 8).astype(np.uint8))
    sx = np.array([[-3, 0, 3], [-10, 0, 10], [-3, 0, 3]], dtype=np.int64)
    dx, dy = K.scharr(img)
    assert np.array_equal(dx, ndi.correlate(img.astype(np.int64), sx, mode="mirror"))
    assert np.array_equal(dy, ndi.correlate(img.astype(np.int64), sx.T, mode="mirror"))
    # the windows: reflect-101 image, zero derivative outside
    if h > 8:
        pad = np.pad(img, 8, mode="reflect")                             # NumPy's "reflect" is reflect-101
        assert np.array_equal(K.image_window(img, -5, h - 4, 9), pad[h + 4:h + 13, 3:12])
    assert np.array_equal(K.deriv_window(dx, -2, h - 3, 5), np.pad(dx, 2)[h - 1:h + 4, :5])      # (np.pad's default: constant 0)


def test_weights_sum_to_one_in_fixed_point():
    r = np.random.default_rng(5)
    fr = np.concatenate([r.random(4000).astype(np.float32), np.array([0.0, 0.5, np.nextafter(np.float32(1), np.float32(0)), 2.0 ** -20], dtype=np.float32)])
    for a, b in zip(fr, fr[::-1]):
        w = K.weights(a, b)
        assert sum(w) == 16384 and min(w) >= -1
    assert K.weights(0.0, 0.0) == (16384, 0, 0, 0) and K.weights(0.5, 0.5) == (4096, 4096, 4096, 4096)
    assert K.weights(np.float32(0.5), np.float32(2.0 ** -15)) == (8192, 8192, 0, 0)      # 0.25 rounds to even: 0


def test_sums_are_exact_integers():
    img = Kc.texture(160, 120)
    d = K.scharr(img)
    I, Ix, Iy = K.template(img, d, np.float32(60.3), np.float32(40.8))
    assert I.shape == Ix.shape == Iy.shape == (30, 30) and I.max() <= 8160 and np.abs(Ix).max() <= 4080
    for a in (Ix * Ix, Ix * Iy, Iy * Iy, (I - 4000) * Ix):
        s = K.isum(a)
        assert s == sum(int(v) for v in a.ravel())                       # Python integers: exact
        assert float(s) == float(np.sum(a.astype(np.float64)))           # below 2^53 a float64 sum of integers is exact too
        assert abs(s) < 2 ** 63 and 15 * 8160 * 4080 < 2 ** 31           # a lane's 15 products fit int32, the window's sum int64
    assert np.float32(K.isum(Ix * Ix)) * K.FLT_SCALE == np.float32(float(K.isum(Ix * Ix)) / 2 ** 20)   # one rounding, the scale is exact


def test_median_rank():
    assert K.get_median([3.0, 1.0, 2.0]) == 2.0
    assert K.get_median([4.0, 1.0, 3.0, 2.0]) == 3.0                    # even count: rank n / 2, the upper of the middle pair
    assert K.get_median([1.0, 2.0, 2.0, 2.0, 5.0, 0.0]) == 2.0 and K.get_median([7.0, 7.0]) == 7.0 and K.get_median([5.0]) == 5.0


# Worst error of 16 interior points measured with this file on the CPU: 0.0068 px at (3.3, -2.1) with at most 3 / 4 / 6
# iterations at levels 0 / 1 / 2, 0.0089 px at (12.4, 7.7) with at most 3 / 4 / 13; the views are cubic-spline resamplings quantised
# to 8 bits, which is where that error comes from.
MEASURED = {(3.3, -2.1): 0.0068, (12.4, 7.7): 0.0089}


@pytest.mark.parametrize("shift", sorted(MEASURED))
def test_the_restated_tracker_tracks(shift):
    w, h = 320, 240
    pts = Kc.interior_points(w, h, 16, 21)
    r = K.track(Kc.texture(w, h), Kc.texture(w, h, shift=shift), pts, pts)
    err = np.abs(r["next"].astype(np.float64) - pts - np.array(shift)).max()
    print(f"shift {shift}: worst error {err:.4f} px, iterations per level {r['iters'].max(axis=0)[:3]}")
    bound = 2.0 * MEASURED[shift]
    assert bound < 0.5                                                   # a tracker that is off by half a pixel is not tracking
    assert r["status"].all() and err <= bound
    assert not K.track(Kc.texture(w, h), Kc.texture(w, h, shift=(25.0, -18.5)), pts[:4], pts[:4])["exit"][:, 0].tolist().count(K.EXIT_EPS)


def test_exit_cases_take_their_exits():
    """every exit the GPU tests compare is one the restatement really takes on its input"""
    ref = {c["name"]: Kc.reference(c["name"]) for c in Kc.exit_cases()}
    for c in Kc.exit_cases():
        if c["code"] is not None:
            assert np.all(ref[c["name"]]["exit"][:, c["level"]] == c["code"]), c["name"]
    e = np.concatenate([ref[n]["exit"][:, :3].ravel() for n in ref])
    assert {K.EXIT_PREV_OOR, K.EXIT_FLAT, K.EXIT_ITER_OOR, K.EXIT_EPS, K.EXIT_OSC, K.EXIT_MAX_ITER} <= set(e.tolist())
    assert np.all(ref["prev_oor_level0"]["exit"][:, 1:3] > K.EXIT_FLAT) and not ref["prev_oor_level0"]["status"].any()   # level 0 alone is out
    assert ref["flat_level0"]["exit"][0, 2] != K.EXIT_FLAT and ref["flat_level0"]["status"][0] == 0
    assert np.all(ref["flat_coarse"]["exit"][0, 1:3] == K.EXIT_FLAT) and ref["flat_coarse"]["exit"][0, 0] in (K.EXIT_EPS, K.EXIT_OSC) and ref["flat_coarse"]["status"][0] == 1
    wo = ref["walk_out"]
    assert wo["exit"][0, 0] == wo["exit"][1, 0] == wo["exit"][2, 1] == K.EXIT_ITER_OOR and wo["iters"][0, 0] >= 1 and wo["iters"][1, 0] >= 1 and wo["iters"][2, 1] >= 1
    fc = ref["final_check"]
    assert np.all(fc["exit"][:, 0] == K.EXIT_MAX_ITER) and not fc["status"].any()          # level 0 ended by count, the range test behind it failed
    assert ref["offset_flow"]["status"].all() and ref["borders"]["status"].all()


def test_ctypes_mirrors_have_the_c_layouts(tmp_path):
    header = os.path.join(ROOT, "include", "plsvo_hip.h")
    structs = {"plsvo_klt_cfg": A.KltCfg, "plsvo_klt_first": A.KltFirst, "plsvo_klt_second": A.KltSecond, "plsvo_klt_params": A.KltParams,
               "plsvo_klt_report": A.KltReport, "plsvo_klt_tracks": A.KltTracks}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header}"', "int main(void){"]
    for cname, ct in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in ct._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append('printf("R %d %d %d %d %d %d %d %d\\n", PLSVO_KLT_FAILURE, PLSVO_KLT_NO_KEYFRAME, PLSVO_KLT_TRACKED, PLSVO_KLT_INACTIVE, PLSVO_KLT_DROPPED, '
                 'PLSVO_KLT_FIRST, PLSVO_KLT_MIN_FIRST, PLSVO_KLT_MAX_LEVEL);')
    lines.append('printf("E %d %d %d %d %d %d %d\\n", PLSVO_KLT_EXIT_NONE, PLSVO_KLT_EXIT_PREV_OOR, PLSVO_KLT_EXIT_FLAT, PLSVO_KLT_EXIT_ITER_OOR, '
                 'PLSVO_KLT_EXIT_EPS, PLSVO_KLT_EXIT_OSC, PLSVO_KLT_EXIT_MAX_ITER);')
    lines.append("return 0;}")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    got = {l.split()[0]: l.split()[1:] for l in out.strip().splitlines()}
    for cname, ct in structs.items():
        assert int(got[cname][0]) == C.sizeof(ct), cname
        for fname, _ in ct._fields_:
            assert int(got[f"{cname}.{fname}"][0]) == getattr(ct, fname).offset, f"{cname}.{fname}"
    assert [int(v) for v in got["R"]] == [A.KLT_FAILURE, A.KLT_NO_KEYFRAME, A.KLT_TRACKED, A.KLT_INACTIVE, A.KLT_DROPPED, A.KLT_FIRST, A.KLT_MIN_FIRST, A.KLT_MAX_LEVEL]
    assert [int(v) for v in got["R"]][:6] == [K.FAILURE, K.NO_KEYFRAME, K.TRACKED, K.INACTIVE, K.DROPPED, K.FIRST]
    assert [int(v) for v in got["E"]] == [K.EXIT_NONE, K.EXIT_PREV_OOR, K.EXIT_FLAT, K.EXIT_ITER_OOR, K.EXIT_EPS, K.EXIT_OSC, K.EXIT_MAX_ITER] == list(range(7))
    assert C.sizeof(A.KltReport) == 32


def test_the_library_exports_the_entry_points():
    lib = os.path.join(ROOT, "pl-svo_amd", "libplsvo_hip.so")
    assert os.path.exists(lib), "pl-svo_amd/libplsvo_hip.so is not built: run __graft_entry__.build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    for name in ENTRY_POINTS:
        assert f" T {name}\n" in out, name
        assert name in Kc.P.capi.SYMBOLS, name
    blob = open(lib, "rb").read()
    for kernel in (b"klt_track_kernel", b"klt_pyrdown_kernel", b"klt_commit_kernel", b"klt_first_kernel"):
        assert kernel in blob, kernel
