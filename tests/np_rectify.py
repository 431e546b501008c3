"""NumPy restatement of vk::PinholeCamera::undistortImage ([ext] vikit) for radial-tangential pinhole cameras, written from OpenCV 3.x's
documented semantics -- initUndistortRectifyMap(K, D, I, K, size, CV_16SC2) and remap(INTER_LINEAR, BORDER_CONSTANT 0) on 8-bit data --
and not from the library's C++ (DESIGN.md "Rectification").  Whole rows at a time, in float64; the operations stay in OpenCV's order
(NumPy never fuses a multiply with an add).

  undistort(raw, cam, flip)      the level-0 image the device builds: optional vertical flip, then the identity branch or the remap
  rectify_map(cam)               OpenCV's map: xy int16 [h, w, 2] (top-left tap), frac uint16 [h, w] = (v & 31) * 32 + (u & 31)
  remap_bilinear(raw, xy, frac)  remap with the fixed-point weights of initInterTab2D

cam: dict(width, height, fx, fy, cx, cy, d=[k1, k2, p1, p2(, k3)]).
"""
import numpy as np


def _f(v):
    """vikit keeps K and D as cv::Mat_<float>: every parameter passes through float32 first"""
    return float(np.float32(v))


def inverse_K(cam):
    """(newK * R)^-1 with newK = K and R = I, by cv::invert(DECOMP_LU) -- for a 3x3 matrix OpenCV uses the adjugate times 1/det"""
    fx, fy, cx, cy = _f(cam["fx"]), _f(cam["fy"]), _f(cam["cx"]), _f(cam["cy"])
    m = [[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]]
    eye = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    a = [[m[i][0] * eye[0][j] + m[i][1] * eye[1][j] + m[i][2] * eye[2][j] for j in range(3)] for i in range(3)]   # K * R, in double
    det = (a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0])
           + a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]))
    d = 1.0 / det
    return [(a[1][1] * a[2][2] - a[1][2] * a[2][1]) * d, (a[0][2] * a[2][1] - a[0][1] * a[2][2]) * d,
            (a[0][1] * a[1][2] - a[0][2] * a[1][1]) * d, (a[1][2] * a[2][0] - a[1][0] * a[2][2]) * d,
            (a[0][0] * a[2][2] - a[0][2] * a[2][0]) * d, (a[0][2] * a[1][0] - a[0][0] * a[1][2]) * d,
            (a[1][0] * a[2][1] - a[1][1] * a[2][0]) * d, (a[0][1] * a[2][0] - a[0][0] * a[2][1]) * d,
            (a[0][0] * a[1][1] - a[0][1] * a[1][0]) * d]


def cv_round(v):
    """cvRound on x86 (cvtsd2si): nearest, ties to even; INT_MIN when the result does not fit in int32"""
    v = np.asarray(v, dtype=np.float64)
    ok = (v >= -2147483648.5) & (v < 2147483647.5)
    return np.where(ok, np.rint(np.where(ok, v, 0.0)), -2147483648.0).astype(np.int64).astype(np.int32)


def rectify_map(cam, accumulate=True):
    """initUndistortRectifyMap's scalar loop.  accumulate=False evaluates _x = j*ir[0] + (i*ir[1] + ir[2]) instead of OpenCV's running
    sum (the unpinned variant the map tests measure the sensitivity to)."""
    W, H = int(cam["width"]), int(cam["height"])
    ir = inverse_K(cam)
    d = [_f(v) for v in (list(cam["d"]) + [0.0] * 5)[:5]]
    k1, k2, p1, p2, k3 = d
    k4 = k5 = k6 = 0.0
    fx, fy, u0, v0 = _f(cam["fx"]), _f(cam["fy"]), _f(cam["cx"]), _f(cam["cy"])
    i = np.arange(H, dtype=np.float64)[:, None]
    starts = [i * ir[1] + ir[2], i * ir[4] + ir[5], i * ir[7] + ir[8]]
    steps = [ir[0], ir[3], ir[6]]
    acc = []
    for s0, st in zip(starts, steps):
        if accumulate:   # _x += ir[0] after every pixel, left to right: a sequential running sum per row
            terms = np.empty((H, W), dtype=np.float64)
            terms[:, :1] = s0
            terms[:, 1:] = st
            acc.append(np.add.accumulate(terms, axis=1))
        else:
            acc.append(np.arange(W, dtype=np.float64)[None, :] * st + s0)
    _x, _y, _w = acc
    w = 1.0 / _w
    x = _x * w
    y = _y * w
    x2 = x * x
    y2 = y * y
    r2 = x2 + y2
    _2xy = 2 * x * y
    kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
    xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)
    yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy
    u = fx * xd + u0
    v = fy * yd + v0
    iu = cv_round(u * 32)
    iv = cv_round(v * 32)
    xy = np.stack([(iu >> 5).astype(np.int16), (iv >> 5).astype(np.int16)], axis=-1)
    frac = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    return xy, frac


def inter_tab_linear():
    """initInterTab2D(INTER_LINEAR, fixed point): [1024, 4] int32 weights (top-left, top-right, bottom-left, bottom-right) of fraction
    ty * 32 + tx; float products * 32768 saturated to short, then OpenCV's fix-up of a sum != 32768 (only entry 0: 32768 -> 32767, the
    missing 1 lands on the last tap)"""
    t = np.arange(32, dtype=np.float32) / np.float32(32)
    tab = np.zeros((32, 32, 4), dtype=np.int32)
    for ty in range(32):
        for tx in range(32):
            cy = (np.float32(1) - t[ty], t[ty])
            cx = (np.float32(1) - t[tx], t[tx])
            vals = [int(np.clip(np.rint(np.float32(cy[a] * cx[b]) * np.float32(32768)), -32768, 32767)) for a in range(2) for b in range(2)]
            tab[ty, tx] = vals
    tab = tab.reshape(1024, 4)
    tab[0] = [32767, 0, 0, 1]   # stated literally: saturation of 32768, then the fix-up
    assert (tab[1:].sum(axis=1) == 32768).all()
    return tab


_TAB = None


def remap_bilinear(raw, xy, frac):
    """cv::remap(raw, out, xy, frac, INTER_LINEAR, BORDER_CONSTANT, 0) for u8: taps outside raw read 0,
    out = (sum tap * weight + (1 << 14)) >> 15, saturated to u8"""
    global _TAB
    if _TAB is None:
        _TAB = inter_tab_linear()
    raw = np.asarray(raw, dtype=np.uint8)
    h, w = raw.shape
    x0 = xy[..., 0].astype(np.int64)
    y0 = xy[..., 1].astype(np.int64)
    wt = _TAB[frac.astype(np.int64)]
    acc = np.full(x0.shape, 1 << 14, dtype=np.int64)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        yy, xx = y0 + dy, x0 + dx
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        tap = np.where(inside, raw[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], 0).astype(np.int64)
        acc += tap * wt[..., k]
    return np.clip(acc >> 15, 0, 255).astype(np.uint8)


def undistort(raw, cam, flip=False):
    """run_pipeline's frame path: flip (cam_fy < 0), then undistortImage -- a copy when |d0| <= 1e-7 (vikit's distortion_ flag, decided on
    the double d0 whatever d1..d4 hold), the remap otherwise"""
    raw = np.asarray(raw, dtype=np.uint8)
    if flip:
        raw = raw[::-1]
    if not abs(float(cam["d"][0])) > 1e-7:
        return raw.copy()
    xy, frac = rectify_map(cam)
    return remap_bilinear(raw, xy, frac)

