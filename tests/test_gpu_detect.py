"""FAST corners per grid cell on the device (plsvo_hip_detect_fast, plsvo_hip_detect_fast_dev, plsvo_hip_detect_stages) against the NumPy
restatement of feature_detection::FastDetector::detect (tests/np_fast.py).  Every comparison is exact: the FAST scores are integers and
the Shi-Tomasi path is deterministic double arithmetic, so records are compared byte for byte (count, order, x, y, level, score bits).
Images stay at <= 160 x 120 and a few slots so that the emulated run (tests/test_emu_parity.py) takes them too; the name of the one
640 x 480 check contains `full_size`.  The pyramids the NumPy side reads are the slot's own levels, downloaded."""
import ctypes as C

import numpy as np
import pytest

import np_fast as F

pytestmark = pytest.mark.gpu

W, H = 160, 120
E_INVALID, E_STATE = -1, -5


@pytest.fixture
def ctx(P):
    c = P.capi.Context(0)
    yield c
    c.close()


def _noise(seed, w=W, h=H):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _blur(img, sigma):
    r = int(3 * sigma) + 1
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    p = np.pad(img, r, mode="edge")
    p = np.apply_along_axis(lambda v: np.convolve(v, k, mode="valid"), 1, p)
    return np.apply_along_axis(lambda v: np.convolve(v, k, mode="valid"), 0, p)


def _scene(seed, w=W, h=H):
    """rectangles at three scales of sharpness on a dim gradient: sharp ones give level-0 corners, the blurred ones only become FAST
    corners after one or two half-samplings"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w)) + 60 + 20 * xx / w
    n = max(6, (w * h) // 1600)
    for sigma in (2.6, 1.3, 0.0):
        layer, mask = np.zeros((h, w)), np.zeros((h, w))
        for _ in range(n):
            cx, cy = rng.uniform(8, w - 8), rng.uniform(8, h - 8)
            a, b = rng.uniform(5, 14) * (1 + sigma), rng.uniform(5, 14) * (1 + sigma)
            th = rng.uniform(0, np.pi)
            u, v = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th), -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
            inside = (np.abs(u) < a) & (np.abs(v) < b)
            layer = np.where(inside, rng.choice([5.0, 250.0]), layer)
            mask = np.where(inside, 1.0, mask)
        if sigma > 0:
            layer, mask = _blur(np.where(mask > 0, layer, img), sigma), _blur(mask, sigma)
        img = mask * layer + (1 - mask) * img
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _motif(seed, w=W, h=H):
    """a 12 x 12 noise motif tiled over the image: the same corner many times in a cell, i.e. equal Shi-Tomasi scores"""
    m = np.random.default_rng(seed).integers(0, 256, (12, 12), dtype=np.uint8)
    return np.tile(m, (h // 12 + 1, w // 12 + 1))[:h, :w].copy()


def _load(ctx, imgs, n_levels=3):
    h, w = imgs[0].shape
    ctx.config_pyramids(len(imgs) + 1, w, h, n_levels)     # slot 0 stays empty: slot arithmetic is exercised
    for i, im in enumerate(imgs):
        ctx.build_pyramid(1 + i, im)
    return [ctx.download_pyramid(1 + i) for i in range(len(imgs))]


def _same(a, b):
    return len(a) == len(b) and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("kind,w,h", [("noise", W, H), ("scene", W, H), ("noise", 157, 93), ("scene", 157, 93)])
def test_stages_equal_numpy_on_every_level(ctx, kind, w, h):
    img = _noise(11, w, h) if kind == "noise" else _scene(12, w, h)
    lv = _load(ctx, [img])[0]
    pairs = 0
    for l in range(3):
        score, surv = ctx.detect_stages(1, l)
        want = F.score_map(lv[l], 20)
        assert np.array_equal(score, want), f"level {l}: {(score != want).sum()} scores differ"
        assert np.array_equal(surv.astype(bool), F.nonmax_map(want)), f"level {l}: survivors differ"
        c = want.astype(int)
        pairs += int(((c[:, 1:] == c[:, :-1]) & (c[:, 1:] > 0)).sum() + ((c[1:] == c[:-1]) & (c[1:] > 0)).sum())
    if kind == "noise":
        assert pairs >= 1, "no pair of equal-score neighbouring corners: equal neighbours must suppress each other somewhere"
    # another FAST threshold than the reference's
    score, surv = ctx.detect_stages(1, 0, fast_threshold=35)
    assert np.array_equal(score, F.score_map(lv[0], 35)) and np.array_equal(surv.astype(bool), F.nonmax_map(F.score_map(lv[0], 35)))


@pytest.mark.parametrize("kind,seed", [("noise", 21), ("scene", 22), ("scene", 23), ("scene", 24), ("motif", 25)])
def test_records_equal_numpy(ctx, kind, seed):
    img = dict(noise=_noise, scene=_scene, motif=_motif)[kind](seed)
    lv = _load(ctx, [img])[0]
    st = {}
    want = F.detect(lv, 25, 20, 20.0, stats=st)
    got = ctx.detect_fast(1, 1)[0]
    assert got.dtype == F.CORNER_DTYPE and _same(got, want), (len(got), len(want))
    assert len(want) >= 5
    if kind == "scene":
        assert np.all(np.bincount(want["level"], minlength=3) >= 1), f"features per level {np.bincount(want['level'], minlength=3)}"
    if kind == "motif":
        assert st["ties"] >= 1, "no equal-score tie inside a cell"
    # other grid and thresholds: a cell size that does not divide the image, a zero threshold, a small cell (more cells per tile
    # than the workgroup reduces in LDS)
    for cell, thr, b in ((30, 0.0, 20), (7, 64.5, 30), (3, 20.0, 20)):
        assert _same(ctx.detect_fast(1, 1, cell, 3, b, thr)[0], F.detect(lv, cell, b, thr)), (cell, thr, b)
    assert _same(ctx.detect_fast(1, 1, n_levels=1)[0], F.detect(lv[:1]))


def test_odd_size_and_two_calls_in_a_row(ctx):
    lv = _load(ctx, [_scene(31, 157, 93)])[0]
    want = F.detect(lv)
    a, b = ctx.detect_fast(1, 1)[0], ctx.detect_fast(1, 1)[0]
    assert _same(a, want) and _same(b, want) and len(want) >= 3     # the second call found the keys re-armed


def test_occupancy_masks_cells_and_leaves_the_others(ctx):
    lv = _load(ctx, [_scene(41)])[0]
    cols, rows = F.grid(W, H, 25)
    free = ctx.detect_fast(1, 1)[0]
    occ = np.random.default_rng(42).integers(0, 2, cols * rows).astype(np.uint8) * 7    # any non-zero byte means occupied
    got = ctx.detect_fast(1, 1, occupancy=occ[None])[0]
    k = (got["y"] // 25) * cols + got["x"] // 25
    assert not occ[k].any()
    kf = (free["y"] // 25) * cols + free["x"] // 25
    assert _same(got, free[occ[kf] == 0]) and 0 < len(got) < len(free)
    assert _same(got, F.detect(lv, occupancy=occ))


def test_batch_of_different_images_equals_one_slot_calls(ctx):
    imgs = [_scene(51), _noise(52), _motif(53), _scene(54)]
    lvs = _load(ctx, imgs)
    batch = ctx.detect_fast(1, 4)
    occ = np.random.default_rng(55).integers(0, 2, (4, 35)).astype(np.uint8)
    batch_occ = ctx.detect_fast(1, 4, occupancy=occ)
    for i in range(4):
        assert _same(batch[i], ctx.detect_fast(1 + i, 1)[0]) and _same(batch[i], F.detect(lvs[i]))
        assert _same(batch_occ[i], F.detect(lvs[i], occupancy=occ[i]))
    assert len({b.tobytes() for b in batch}) == 4


def _device_buffer(nbytes):
    """zeroed device memory the library's d_ pointers can reach: HBM through torch on a GPU box, a host array on the emulation build
    -> (keep-alive, pointer, read-back function)"""
    import torch
    if torch.cuda.is_available():
        t = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        return t, t.data_ptr(), lambda: t.cpu().numpy()
    a = np.zeros(nbytes, dtype=np.uint8)
    return a, a.ctypes.data, lambda: a.copy()


def test_device_buffers_equal_host_form(ctx):
    lvs = _load(ctx, [_scene(61), _noise(62)])
    cells = 35
    kc, pc, rc = _device_buffer(2 * cells * 16)
    kn, pn, rn = _device_buffer(2 * 4)
    occ = np.zeros((2, cells), np.uint8)
    occ[1, ::3] = 1
    ko, po, _ = _device_buffer(2 * cells)
    if isinstance(ko, np.ndarray):
        ko[:] = occ.ravel()
    else:
        import torch
        ko.copy_(torch.from_numpy(occ.ravel()))
        torch.cuda.synchronize()
    for d_occ, o in ((None, None), (po, occ)):
        ctx.detect_fast_dev(1, 2, pc, pn, d_occupancy=d_occ)
        ctx.synchronize()
        counts = rn().view(np.int32)
        recs = rc().view(F.CORNER_DTYPE).reshape(2, cells)
        host = ctx.detect_fast(1, 2, occupancy=o)
        for i in range(2):
            assert counts[i] == len(host[i]) > 0 and _same(recs[i, :counts[i]], host[i])


def test_rejected_arguments_return_their_code_and_write_nothing(P, ctx):
    L = ctx.L
    cells = 35
    out = np.full(cells * 2, 0x5A, dtype=np.uint8).repeat(16)
    counts = np.full(2, -77, dtype=np.int32)
    sc, sv = np.full(W * H, 0x5A, np.uint8), np.full(W * H, 0x5A, np.uint8)
    u8, i32 = P.abi.c_u8_p, P.abi.c_i32_p
    cp = C.POINTER(P.abi.Corner)

    def call(first=1, n=1, corners=True, cnt=True, params=True, **kw):
        pr = P.abi.detect_params(**kw)
        return L.plsvo_hip_detect_fast(ctx.h, first, n, C.byref(pr) if params else None, None, out.ctypes.data_as(cp) if corners else None,
                                       counts.ctypes.data_as(i32) if cnt else None)

    def stages(slot=1, level=0, b=20, s=True, v=True):
        return L.plsvo_hip_detect_stages(ctx.h, slot, level, b, sc.ctypes.data_as(u8) if s else None, sv.ctypes.data_as(u8) if v else None)

    assert call() == E_STATE and stages() == E_STATE                                    # pyramids not configured
    _load(ctx, [_noise(71)])                                                            # 2 slots, 3 levels
    assert call() == 0
    out[:] = 0x5A
    counts[:] = -77
    for kw in (dict(first=-1), dict(first=2), dict(first=1, n=2), dict(n=0), dict(n_levels=0), dict(n_levels=4), dict(cell_size=0), dict(cell_size=-3),
               dict(fast_threshold=0), dict(fast_threshold=255), dict(detection_threshold=-1.0), dict(detection_threshold=float("nan")),
               dict(detection_threshold=float("inf")), dict(detection_threshold=0.1), dict(corners=False), dict(cnt=False), dict(params=False)):
        assert call(**kw) == E_INVALID, kw
        assert b"detect_fast" in L.plsvo_hip_last_error(ctx.h)
    pr = P.abi.detect_params()
    for a in ((None, 8, 8), (8, None, 8), (8, 8, None)):
        assert L.plsvo_hip_detect_fast_dev(ctx.h, 1, 1, C.byref(pr) if a[0] else None, None, a[1], a[2]) == E_INVALID
    assert L.plsvo_hip_detect_fast_dev(ctx.h, 2, 1, C.byref(pr), None, 8, 8) == E_INVALID
    for kw in (dict(slot=-1), dict(slot=2), dict(level=-1), dict(level=3), dict(b=0), dict(b=255), dict(s=False), dict(v=False)):
        assert stages(**kw) == E_INVALID, kw
    assert np.all(out == 0x5A) and np.all(counts == -77) and np.all(sc == 0x5A) and np.all(sv == 0x5A)
    # a level smaller than 7 x 7, and an image beyond 13 bits per coordinate
    ctx.config_pyramids(1, 24, 24, 3)
    assert call(first=0) == E_INVALID and call(first=0, n_levels=2) == 0
    ctx.config_pyramids(1, 8192, 8, 1)
    assert call(first=0, n_levels=1) == E_INVALID
    ctx.config_pyramids(1, 8191, 8, 1)
    assert call(first=0, n_levels=1, cell_size=1000) == 0


def test_detection_follows_rectification_without_a_host_round_trip(P, ctx):
    cam = P.abi.pinhole_radtan(W, H, 95.3, 96.1, 79.6, 60.2, [-0.28340811, 0.07395907, 1.9359e-4, 1.76187114e-5])
    ctx.config_pyramids(3, W, H, 3)
    mid = ctx.config_rectify(cam)
    raws = np.stack([_scene(81), _scene(82)])
    import torch
    if torch.cuda.is_available():
        keep = torch.from_numpy(raws).cuda()
        torch.cuda.synchronize()
        p_raw = keep.data_ptr()
    else:
        keep, p_raw = raws, raws.ctypes.data
    cells = 35
    kc, pc, rc = _device_buffer(2 * cells * 16)
    kn, pn, rn = _device_buffer(2 * 4)
    ctx.rectify_build_pyramids_dev(mid, 1, 2, p_raw, W, W * H)      # both calls only enqueue
    ctx.detect_fast_dev(1, 2, pc, pn)
    ctx.synchronize()
    counts, recs = rn().view(np.int32), rc().view(F.CORNER_DTYPE).reshape(2, cells)
    for i in range(2):
        want = F.detect(ctx.download_pyramid(1 + i))
        assert len(want) >= 3 and _same(recs[i, :counts[i]], want)
    # ... and the host form after the host form of the rectification
    ctx.rectify_build_pyramid(mid, 0, raws[0])
    assert _same(ctx.detect_fast(0, 1)[0], F.detect(ctx.download_pyramid(0)))


def test_full_size_640x480_equals_numpy(ctx):
    img = _scene(91, 640, 480)
    img[300:420, 100:260] = _motif(92, 160, 120)
    img[40:140, 400:560] = _noise(93, 160, 100)
    lv = _load(ctx, [img, _scene(94, 640, 480)])
    got = ctx.detect_fast(1, 2)
    for i in range(2):
        want = F.detect(lv[i])
        assert _same(got[i], want) and np.all(np.bincount(want["level"], minlength=3) >= 1)
    for l in range(3):
        score, surv = ctx.detect_stages(1, l)
        want = F.score_map(lv[0][l], 20)
        assert np.array_equal(score, want) and np.array_equal(surv.astype(bool), F.nonmax_map(want))
