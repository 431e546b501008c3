"""Restatement of the keyframe stage in plain float64, loop for loop like the reference (test infrastructure only):

  Frame::isVisible                 src/frame.cpp:156-165
  Map::getCloseKeyframes           src/map.cpp:158-179, sorted and cut like Reprojector::reprojectMap (src/reprojector.cpp:147-163)
  frame_utils::getSceneDepth       src/frame.cpp:182-217 (vk::getMedian: the element of rank m // 2)
  FrameHandlerMono::needNewKf      src/frame_handler_mono.cpp:475-499
  Frame::setKeyPoints / checkKeyPoints   src/frame.cpp:87-141
  Map::getFurthestKeyframe         src/map.cpp:201-214
  [ext] Sophus SE3::log, SO3::logAndTheta, SE3::inverse, operator*; Eigen's quaternion rotation and norm()

Every function works on Python floats (IEEE binary64, one rounding per operation, no contraction) in the expression order of
Eigen / Sophus, so the device results can be compared bit for bit; only atan / tan of the logarithm come from the host's libm.
Poses are (qx, qy, qz, qw, tx, ty, tz).  Two places where the reference leaves the result open are pinned: of zeros of both signs the
negative one is the smaller depth (fmin and nth_element do not order them)."""
import math

import numpy as np


def _f(a):
    return [float(v) for v in np.asarray(a, dtype=np.float64).reshape(-1)]


def q_rot(q, v):
    """Eigen::Quaternion::_transformVector"""
    qx, qy, qz, qw = q
    ux = qy * v[2] - qz * v[1]
    uy = qz * v[0] - qx * v[2]
    uz = qx * v[1] - qy * v[0]
    ux += ux
    uy += uy
    uz += uz
    return [v[0] + qw * ux + (qy * uz - qz * uy), v[1] + qw * uy + (qz * ux - qx * uz), v[2] + qw * uz + (qx * uy - qy * ux)]


def se3_act(T, p):
    T, p = _f(T), _f(p)
    r = q_rot(T[:4], p)
    return [r[0] + T[4], r[1] + T[5], r[2] + T[6]]


def se3_inv(T):
    T = _f(T)
    qc = [-T[0], -T[1], -T[2], T[3]]
    return qc + q_rot(qc, [-T[4], -T[5], -T[6]])


def se3_mul(A, B):
    A, B = _f(A), _f(B)
    ax, ay, az, aw = A[:4]
    bx, by, bz, bw = B[:4]
    w = aw * bw - ax * bx - ay * by - az * bz
    x = aw * bx + ax * bw + ay * bz - az * by
    y = aw * by + ay * bw + az * bx - ax * bz
    z = aw * bz + az * bw + ax * by - ay * bx
    n = math.sqrt(x * x + y * y + z * z + w * w)
    rt = q_rot(A[:4], B[4:])
    return [x / n, y / n, z / n, w / n, A[4] + rt[0], A[5] + rt[1], A[6] + rt[2]]


def norm3(x, y, z):
    """Eigen's norm() of a Vector3d"""
    return math.sqrt((x * x + y * y) + z * z)


def se3_log(T):
    """Sophus SE3::log: (upsilon, omega); SMALL_EPS = 1e-10; theta keeps the sign of w and the small-angle test is on the signed value"""
    T = _f(T)
    qx, qy, qz, w = T[:4]
    n = norm3(qx, qy, qz)
    squared_w = w * w
    if n < 1e-10:
        f = 2.0 / w - 2.0 * (n * n) / (w * squared_w)
    elif abs(w) < 1e-10:
        f = (math.pi if w > 0.0 else -math.pi) / n
    else:
        f = 2.0 * math.atan(n / w) / n
    theta = f * n
    ox, oy, oz = f * qx, f * qy, f * qz
    if theta < 1e-10:
        c = 1.0 / 12.0
    else:
        c = (1.0 - theta / (2.0 * math.tan(theta / 2.0))) / (theta * theta)
    O2_00, O2_11, O2_22 = -(oy * oy + oz * oz), -(ox * ox + oz * oz), -(ox * ox + oy * oy)
    O2_01, O2_02, O2_12 = ox * oy, ox * oz, oy * oz
    V = [1.0 + c * O2_00, 0.5 * oz + c * O2_01, -0.5 * oy + c * O2_02,
         -0.5 * oz + c * O2_01, 1.0 + c * O2_11, 0.5 * ox + c * O2_12,
         0.5 * oy + c * O2_02, -0.5 * ox + c * O2_12, 1.0 + c * O2_22]
    t = T[4:]
    ups = [(V[3 * i] * t[0] + V[3 * i + 1] * t[1]) + V[3 * i + 2] * t[2] for i in range(3)]
    return ups + [ox, oy, oz]


def w2c(cam, xyz):
    """vk::PinholeCamera::world2cam without distortion; cam = (fx, fy, cx, cy, width, height)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        x, y, z = (np.float64(v) for v in xyz)
        return float(np.float64(cam[0]) * (x / z) + np.float64(cam[2])), float(np.float64(cam[1]) * (y / z) + np.float64(cam[3]))


def is_visible(T_f_w, cam, xyz_w):
    xyz_f = se3_act(T_f_w, xyz_w)
    if xyz_f[2] < 0.0:
        return False
    px = w2c(cam, xyz_f)
    return bool(px[0] >= 0.0 and px[1] >= 0.0 and px[0] < cam[4] and px[1] < cam[5])


def close_keyframes(T_f_w, cam, kf_T, keypt_pos, keypt_valid, max_n_kfs=10):
    """-> dict(n_close, n_overlap, close_idx, close_dist): the list getCloseKeyframes builds, after the stable sort by distance"""
    T = _f(T_f_w)
    kf_T = np.asarray(kf_T, np.float64).reshape(-1, 7)
    kp = np.asarray(keypt_pos, np.float64).reshape(-1, 5, 3)
    kv = np.asarray(keypt_valid).reshape(-1, 5)
    close = []
    for i in range(kf_T.shape[0]):
        for k in range(5):
            if not kv[i, k]:
                continue
            if is_visible(T, cam, kp[i, k]):
                K = _f(kf_T[i])
                close.append((i, norm3(T[4] - K[4], T[5] - K[5], T[6] - K[6])))
                break
    close.sort(key=lambda e: e[1])          # list.sort is stable, like std::list::sort
    return dict(n_close=len(close), n_overlap=min(len(close), int(max_n_kfs)), close_idx=np.array([e[0] for e in close], np.int32),
                close_dist=np.array([e[1] for e in close], np.float64))


def _below(a, b):
    """a before b in the order of the depths: as numbers, and -0.0 before +0.0"""
    return a < b or (a == b and math.copysign(1.0, a) < math.copysign(1.0, b))


def scene_depth(T_f_w, pt_pos, pt_alive, seg_spos, seg_epos, seg_alive):
    """-> dict(has_depth, n_depth, depth_mean, depth_min); without a feature depth_mean = 0 (the reference leaves it untouched)"""
    DBL_MAX = float(np.finfo(np.float64).max)
    pt_pos = np.asarray(pt_pos, np.float64).reshape(-1, 3)
    sp, ep = np.asarray(seg_spos, np.float64).reshape(-1, 3), np.asarray(seg_epos, np.float64).reshape(-1, 3)
    vec = []
    depth_min = DBL_MAX
    for i in range(pt_pos.shape[0]):
        if pt_alive is None or pt_alive[i]:
            z = se3_act(T_f_w, pt_pos[i])[2]
            vec.append(z)
            depth_min = z if _below(z, depth_min) else depth_min
    for i in range(sp.shape[0]):
        if seg_alive is None or seg_alive[i]:
            zs, ze = se3_act(T_f_w, sp[i])[2], se3_act(T_f_w, ep[i])[2]
            vec += [zs, ze]
            depth_min = zs if _below(zs, depth_min) else depth_min
            depth_min = ze if _below(ze, depth_min) else depth_min
    if not vec:
        return dict(has_depth=0, n_depth=0, depth_mean=0.0, depth_min=DBL_MAX)
    s = sorted(vec, key=lambda z: (z, math.copysign(1.0, z)))
    return dict(has_depth=1, n_depth=len(vec), depth_mean=s[len(vec) // 2], depth_min=depth_min)


def need_new_kf(T_last_w, overlap_T, min_t=0.06, min_r=3.0):
    """-> dict(need_new_kf, blocking, delta_t, delta_r): the loop of needNewKf, with every delta kept"""
    T_last_inv = se3_inv(T_last_w)
    dts, drs, blocking = [], [], -1
    for j, T_kf in enumerate(np.asarray(overlap_T, np.float64).reshape(-1, 7)):
        xi = se3_log(se3_mul(T_last_inv, T_kf))
        delta_t = norm3(xi[0], xi[1], xi[2])
        delta_r = norm3(xi[3], xi[4], xi[5]) * 180.0 / 3.1416
        dts.append(delta_t)
        drs.append(delta_r)
        if blocking < 0 and delta_t < min_t and delta_r < min_r:
            blocking = j
    return dict(need_new_kf=int(blocking < 0), blocking=blocking, delta_t=np.array(dts, np.float64), delta_r=np.array(drs, np.float64))


def set_key_points(width, height, pt_px, pt_alive, key_pts_prev):
    """Frame::setKeyPoints on indices (-1 = NULL): drop dead holders, then checkKeyPoints for every alive point in list order"""
    px = np.asarray(pt_px, np.float64).reshape(-1, 2)
    alive = [True] * px.shape[0] if pt_alive is None else [bool(a) for a in pt_alive]
    key = [int(k) for k in key_pts_prev]
    for i in range(5):
        if key[i] >= 0 and not alive[key[i]]:
            key[i] = -1
    cu, cv = int(width) // 2, int(height) // 2
    X = lambda i: float(px[i, 0])
    Y = lambda i: float(px[i, 1])
    prod = lambda i: (X(i) - cu) * (Y(i) - cv)
    for f in range(px.shape[0]):
        if not alive[f]:
            continue
        if key[0] < 0:
            key[0] = f
        elif max(abs(X(f) - cu), abs(Y(f) - cv)) < max(abs(X(key[0]) - cu), abs(Y(key[0]) - cv)):
            key[0] = f
        tests = (X(f) >= cu and Y(f) >= cv, X(f) >= cu and Y(f) < cv, X(f) < cv and Y(f) < cv, X(f) < cv and Y(f) >= cv)   # (cv: as the reference)
        for s in range(4):
            if tests[s]:
                if key[s + 1] < 0:
                    key[s + 1] = f
                elif prod(f) > prod(key[s + 1]):
                    key[s + 1] = f
    return np.array(key, np.int32)


def furthest_keyframe(T_new_w, kf_T):
    pos = se3_inv(T_new_w)[4:]
    furthest, maxdist = -1, 0.0
    for i, K in enumerate(np.asarray(kf_T, np.float64).reshape(-1, 7)):
        p = se3_inv(K)[4:]
        dist = norm3(p[0] - pos[0], p[1] - pos[1], p[2] - pos[2])
        if dist > maxdist:
            maxdist, furthest = dist, i
    return furthest


def decide(job):
    """everything plsvo_keyframe_decide returns for one abi.KeyframeDecideJob (job.T_new: the pose to use)"""
    c = job.c
    T_new, T_last = list(c.T_new_w), list(c.T_last_w)
    r = scene_depth(T_new, job.pt_pos, job.pt_alive, job.seg_spos, job.seg_epos, job.seg_alive)
    r.update(need_new_kf(T_last, job.kf_T[job.overlap_idx] if job.n_overlap else np.zeros((0, 7)), c.kfselect_mindist_t, c.kfselect_mindist_r))
    r["key_pts"] = set_key_points(c.cam.width, c.cam.height, job.pt_px, job.pt_alive, list(c.key_pts_prev))
    r["furthest_kf"] = furthest_keyframe(T_new, job.kf_T)
    return r


def close(job):
    c = job.c
    cam = (c.cam.fx, c.cam.fy, c.cam.cx, c.cam.cy, c.cam.width, c.cam.height)
    return close_keyframes(list(c.T_f_w), cam, job.kf_T, job.keypt_pos, job.keypt_valid, c.max_n_kfs)
