"""NumPy restatement of the bootstrap's KLT track: KltHomographyInit::addFirstFrame / addSecondFrame up to the disparity
gate (src/initialization.cpp:40-69) and trackKlt (:170-215) with [ext] cv::calcOpticalFlowPyrLK (win 30, maxLevel 4, 30 iterations,
eps 0.001, minEigThreshold 1e-4, OPTFLOW_USE_INITIAL_FLOW) restated from knowledge of upstream -- OpenCV is not available here, parity
with an upstream binary is unpinned.  Independent of the device code: the Scharr derivatives are dense images here, the kernel computes
them on the fly from a staged window.

Float arithmetic is IEEE single, one operation at a time in the order written (np.float32 scalars); every sum over the window is an exact
integer that is converted to float once (pinned: upstream's scalar and SIMD paths add floats in different orders)."""
import numpy as np

F = np.float32
WIN, MAX_LEVEL, MAX_ITER, EPS, MIN_EIG = 30, 4, 30, 0.001, 1e-4
FAILURE, NO_KEYFRAME, TRACKED, INACTIVE, DROPPED, FIRST = 0, 1, 2, 3, 4, 5
EXIT_NONE, EXIT_PREV_OOR, EXIT_FLAT, EXIT_ITER_OOR, EXIT_EPS, EXIT_OSC, EXIT_MAX_ITER = 0, 1, 2, 3, 4, 5, 6
MIN_FIRST = 100
HALF = F(14.5)
FLT_SCALE = F(1.0 / (1 << 20))
FLT_EPSILON = F(np.finfo(np.float32).eps)


def level_sizes(w, h, win=WIN, max_level=MAX_LEVEL):
    """sizes of levels 0 .. L: the first level whose NEXT size has w <= win or h <= win is the top level"""
    out = []
    for _ in range(max_level + 1):
        out.append((w, h))
        nw, nh = (w + 1) // 2, (h + 1) // 2
        if nw <= win or nh <= win:
            break
        w, h = nw, nh
    return out


def reflect101(i, n):
    """cv::borderInterpolate(i, n, BORDER_REFLECT_101) for an index array"""
    i = np.asarray(i, dtype=np.int64).copy()
    if n == 1:
        return np.zeros_like(i)
    while True:
        bad = (i < 0) | (i >= n)
        if not bad.any():
            return i
        i = np.where(i < 0, -i, i)
        i = np.where(i >= n, 2 * n - 2 - i, i)


def pyr_down(img):
    """cv::pyrDown of a uint8 image: 5 x 5 binomial, reflect-101, (sum + 128) >> 8"""
    h, w = img.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    k = (1, 4, 6, 4, 1)
    src = img.astype(np.int64)
    acc = np.zeros((oh, ow), dtype=np.int64)
    for dy in range(-2, 3):
        ry = reflect101(2 * np.arange(oh) + dy, h)
        for dx in range(-2, 3):
            rx = reflect101(2 * np.arange(ow) + dx, w)
            acc += k[dy + 2] * k[dx + 2] * src[np.ix_(ry, rx)]
    return ((acc + 128) >> 8).astype(np.uint8)


def build_pyramid(img0, win=WIN, max_level=MAX_LEVEL):
    sizes = level_sizes(img0.shape[1], img0.shape[0], win, max_level)
    pyr = [np.ascontiguousarray(img0, dtype=np.uint8)]
    for _ in sizes[1:]:
        pyr.append(pyr_down(pyr[-1]))
    assert [(p.shape[1], p.shape[0]) for p in pyr] == sizes
    return pyr


def scharr(img):
    """Scharr derivatives (3, 10, 3) of a uint8 image on reflect-101 neighbours: int64 dx, dy of the image's size"""
    h, w = img.shape
    p = img.astype(np.int64)[np.ix_(reflect101(np.arange(-1, h + 1), h), reflect101(np.arange(-1, w + 1), w))]
    dx = 3 * (p[:-2, 2:] - p[:-2, :-2]) + 10 * (p[1:-1, 2:] - p[1:-1, :-2]) + 3 * (p[2:, 2:] - p[2:, :-2])
    dy = 3 * (p[2:, :-2] - p[:-2, :-2]) + 10 * (p[2:, 1:-1] - p[:-2, 1:-1]) + 3 * (p[2:, 2:] - p[:-2, 2:])
    return dx, dy


def weights(a, b):
    """the fixed-point bilinear weights of the fractions a, b (float32): cvRound of the float products, the last by difference"""
    a, b, one, s = F(a), F(b), F(1), F(16384)
    w00 = int(np.rint((one - a) * (one - b) * s))
    w01 = int(np.rint(a * (one - b) * s))
    w10 = int(np.rint((one - a) * b * s))
    return w00, w01, w10, 16384 - w00 - w01 - w10


def image_window(img, x0, y0, n):
    """n x n pixels from (x0, y0), reflect-101 outside the image"""
    h, w = img.shape
    return img.astype(np.int64)[np.ix_(reflect101(np.arange(y0, y0 + n), h), reflect101(np.arange(x0, x0 + n), w))]


def deriv_window(d, x0, y0, n):
    """n x n values of a derivative image from (x0, y0), 0 outside (constant border)"""
    h, w = d.shape
    out = np.zeros((n, n), dtype=np.int64)
    ys, xs = np.arange(y0, y0 + n), np.arange(x0, x0 + n)
    my, mx = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
    if my.any() and mx.any():
        out[np.ix_(my, mx)] = d[np.ix_(ys[my], xs[mx])]
    return out


def bilinear_int(win, wt):
    """sum of the four taps of every window pixel with integer weights; win is (n + 1) x (n + 1)"""
    return win[:-1, :-1] * wt[0] + win[:-1, 1:] * wt[1] + win[1:, :-1] * wt[2] + win[1:, 1:] * wt[3]


def in_range(fx, fy, w, h, win=WIN):
    """the window test on the floored position; a position cvFloor cannot hold (huge, NaN) is outside"""
    return bool(fx >= F(-win) and fx < F(w) and fy >= F(-win) and fy < F(h))


def template(img, dxy, plx, ply):
    """I (scaled by 32), Ix, Iy over the 30 x 30 window of prev_l - half = (plx, ply)"""
    fx, fy = np.floor(plx), np.floor(ply)
    ix, iy = int(fx), int(fy)
    wt = weights(plx - fx, ply - fy)
    I = (bilinear_int(image_window(img, ix, iy, WIN + 1), wt) + 256) >> 9
    Ix = (bilinear_int(deriv_window(dxy[0], ix, iy, WIN + 1), wt) + 8192) >> 14
    Iy = (bilinear_int(deriv_window(dxy[1], ix, iy, WIN + 1), wt) + 8192) >> 14
    return I, Ix, Iy


def isum(a):
    """exact integer sum (Python int)"""
    return int(np.asarray(a, dtype=np.int64).sum())


def track_point(ref_pyr, ref_d, cur_pyr, prev, nxt, max_iter=MAX_ITER, eps=EPS, min_eig_thr=MIN_EIG):
    """one point through every level -> (next (2 float32), status, exit[5], iters[5]); ref_d: scharr() of every reference level"""
    L = len(ref_pyr) - 1
    exits, iters = [EXIT_NONE] * (MAX_LEVEL + 1), [0] * (MAX_LEVEL + 1)
    status = 1
    px, py = F(prev[0]), F(prev[1])
    nx, ny = F(nxt[0]), F(nxt[1])
    with np.errstate(all="ignore"):
        for l in range(L, -1, -1):
            img, cur = ref_pyr[l], cur_pyr[l]
            h, w = img.shape
            inv = F(1.0 / (1 << l))
            plx, ply = px * inv - HALF, py * inv - HALF
            if l == L:
                nx, ny = nx * inv, ny * inv
            else:
                nx, ny = nx * F(2), ny * F(2)
            if not in_range(np.floor(plx), np.floor(ply), w, h):
                exits[l] = EXIT_PREV_OOR
                if l == 0:
                    status = 0
                continue
            I, Ix, Iy = template(img, ref_d[l], plx, ply)
            A11, A12, A22 = F(isum(Ix * Ix)) * FLT_SCALE, F(isum(Ix * Iy)) * FLT_SCALE, F(isum(Iy * Iy)) * FLT_SCALE
            D = A11 * A22 - A12 * A12
            dd = A11 - A22
            min_eig = (A22 + A11 - np.sqrt(dd * dd + F(4) * A12 * A12)) / F(1800)
            if float(min_eig) < min_eig_thr or D < FLT_EPSILON:
                exits[l] = EXIT_FLAT
                if l == 0:
                    status = 0
                continue
            D = F(1) / D
            qx, qy = nx - HALF, ny - HALF
            pdx, pdy = F(0), F(0)
            exits[l], iters[l] = EXIT_MAX_ITER, max_iter
            for j in range(max_iter):
                fx, fy = np.floor(qx), np.floor(qy)
                if not in_range(fx, fy, w, h):
                    if l == 0:
                        status = 0
                    exits[l], iters[l] = EXIT_ITER_OOR, j
                    break
                wt = weights(qx - fx, qy - fy)
                diff = ((bilinear_int(image_window(cur, int(fx), int(fy), WIN + 1), wt) + 256) >> 9) - I
                b1, b2 = F(isum(diff * Ix)) * FLT_SCALE, F(isum(diff * Iy)) * FLT_SCALE
                dx, dy = (A12 * b2 - A22 * b1) * D, (A12 * b1 - A11 * b2) * D
                qx, qy = qx + dx, qy + dy
                nx, ny = qx + HALF, qy + HALF
                if float(dx) * float(dx) + float(dy) * float(dy) <= eps * eps:
                    exits[l], iters[l] = EXIT_EPS, j + 1
                    break
                if j > 0 and abs(float(dx + pdx)) < 0.01 and abs(float(dy + pdy)) < 0.01:
                    nx, ny = nx - dx * F(0.5), ny - dy * F(0.5)
                    exits[l], iters[l] = EXIT_OSC, j + 1
                    break
                pdx, pdy = dx, dy
        if status and not in_range(np.floor(nx - HALF), np.floor(ny - HALF), ref_pyr[0].shape[1], ref_pyr[0].shape[0]):
            status = 0   # the error output's range test behind level 0
    return np.array([nx, ny], dtype=np.float32), status, exits, iters


def track(ref_img, cur_img, prev, nxt, win=WIN, max_level=MAX_LEVEL, max_iter=MAX_ITER, eps=EPS, min_eig=MIN_EIG):
    """calcOpticalFlowPyrLK on two level-0 images -> dict of next (n x 2 float32), status, exit and iters (n x 5 uint8)"""
    ref_pyr, cur_pyr = build_pyramid(ref_img, win, max_level), build_pyramid(cur_img, win, max_level)
    ref_d = [scharr(p) for p in ref_pyr]
    prev, nxt = np.asarray(prev, dtype=np.float32).reshape(-1, 2), np.asarray(nxt, dtype=np.float32).reshape(-1, 2)
    n = len(prev)
    out = dict(next=np.zeros((n, 2), np.float32), status=np.zeros(n, np.uint8), exit=np.zeros((n, MAX_LEVEL + 1), np.uint8),
               iters=np.zeros((n, MAX_LEVEL + 1), np.uint8))
    for i in range(n):
        out["next"][i], out["status"][i], out["exit"][i], out["iters"][i] = track_point(ref_pyr, ref_d, cur_pyr, prev[i], nxt[i], max_iter, eps, min_eig)
    return out


def bearing(cam, px):
    """cam2world of float pixels in double (sel_bearing's expressions); cam = (fx, fy, cx, cy)"""
    px = np.asarray(px, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    x, y = (px[:, 0] - cam[2]) / cam[0], (px[:, 1] - cam[3]) / cam[1]
    n = np.sqrt((x * x + y * y) + 1.0)
    return np.stack([x / n, y / n, 1.0 / n], axis=1)


def get_median(v):
    """vk::getMedian: the element of rank n / 2"""
    v = sorted(float(x) for x in v)
    return v[len(v) // 2]


def first_frame(cam, px, extra_px=None, extra_f=None, cap_pts=1 << 30):
    """addFirstFrame: the lists and the report of a first frame (corners, then the extra points with their given bearings)"""
    px = np.asarray(px, dtype=np.float32).reshape(-1, 2)
    f = bearing(cam, px)
    if extra_px is not None and len(extra_px):
        px = np.concatenate([px, np.asarray(extra_px, dtype=np.float32).reshape(-1, 2)])
        f = np.concatenate([f, np.asarray(extra_f, dtype=np.float64).reshape(-1, 3)])
    n = len(px)
    result = DROPPED if n > cap_pts else (FAILURE if n < MIN_FIRST else FIRST)
    if result != FIRST:
        px, f = px[:0], f[:0]
    lists = dict(px_ref=px.copy(), px_cur=px.copy(), f_ref=f.copy(), f_cur=np.zeros((0, 3)), disparity=np.zeros(0))
    return lists, dict(result=result, n_before=n, n_after=len(px), median_disparity=0.0, n_calls=0)


def second_frame(lists, cam, ref_img, cur_img, n_calls, min_tracked=40, min_disparity=40.0, **cfg):
    """addSecondFrame up to the gates: the track from px_cur, the lists closed up over status == 0, bearings, disparities, median, gates"""
    tr = track(ref_img, cur_img, lists["px_ref"], lists["px_cur"], **cfg)
    keep = tr["status"] != 0
    px_ref, px_cur, f_ref = lists["px_ref"][keep], tr["next"][keep], lists["f_ref"][keep]
    d = (px_ref - px_cur).astype(np.float64)            # float differences, double norm
    disp = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    n = int(keep.sum())
    median = get_median(disp) if n else 0.0
    result = FAILURE if n < min_tracked else (NO_KEYFRAME if median < min_disparity else TRACKED)
    out = dict(px_ref=px_ref, px_cur=px_cur, f_ref=f_ref, f_cur=bearing(cam, px_cur), disparity=disp)
    return out, dict(result=result, n_before=len(keep), n_after=n, median_disparity=median, n_calls=n_calls + 1), tr
