"""An independent NumPy restatement of the depth filter's seed update (test infrastructure only), with a record of the path each
epipolar search took.

Written from the reference source -- DepthFilter::updatePointSeeds / updateLineSeeds / updatePointSeed / updateLineSeed / computeTau
(src/depth_filter.cpp:270-584) and Matcher::findEpipolarMatchDirect / findEpipolarMatchDirectSegmentEndpoint / depthFromTriangulation
(src/matcher.cpp:133-146, :277-586) -- not from oracle/plsvo_oracle.c and not from the kernel.  It reuses the NumPy warp and align2D of
tests/test_match_direct.py.  update_seeds() returns the same fields as plsvo_update_seeds plus the records.

Where the reference's behaviour is undefined the restatement says what it does:
  * a non-finite epipolar length in the POINT search (`size_t n_steps = NaN / 0.7`) ends the search without a match (exit
    `epi_nonfinite`), as the end-point variant does explicitly (:480-484);
  * warpAffine with a NaN inverse returns without writing the patch (:99-103) and the reference goes on with the previous seed's
    patch: here the search ends without a match (exit `warp_fail`);
  * a pixel position beyond the int range (|px| >= 1e9) in the visibility test counts as outside the image; in the walk it raises:
    the directed inputs must not reach it."""
import math

import numpy as np

import np_restatement as npr
import test_match_direct as tm

f32, f64 = np.float32, np.float64
NOT_VISIBLE, NO_MATCH, UPDATED, CONVERGED, NAN = 0, 1, 2, 3, 4
EXITS = ("invisible", "nan_bounds", "edgelet_reject", "epi_nonfinite", "warp_fail", "short_ok", "short_align_fail", "short_tri_fail",
         "too_many_steps", "no_score_below_threshold", "walk_ok", "walk_align_fail", "walk_tri_fail")
THRESHOLD = 2000 * 64          # vk::patch_score::ZMSSD<4>::threshold()
DEFAULTS = dict(n_pyr_levels=3, align_max_iter=10, max_epi_search_steps=1000, edgelet_filtering=True, edgelet_max_angle=0.7, px_noise=1.0,
                convergence_sigma2_thresh=200.0)


def se3_inv(T):
    q = np.array([-T[0], -T[1], -T[2], T[3]])
    return np.concatenate([q, npr.q_rot(q, -np.asarray(T[4:], float))])


def rotation_matrix(T):
    x, y, z, w = T[:4]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def new_record(ref_level, exit_=None):
    return dict(exit=exit_, ref_level=int(ref_level), search_level=-1, n_steps=0, n_scored=0, n_repeat_skipped=0, n_out_of_frame_skipped=0,
                n_positions_at_best=0, first_row_phase_best=-1, row_phases_best=frozenset(), row_phases=frozenset())


def depth_from_triangulation(T_search_ref, f_ref, f_cur):
    """src/matcher.cpp:133-146 -> (ok, depth)"""
    A = np.stack([rotation_matrix(T_search_ref) @ f_ref, f_cur], axis=1)
    AtA = A.T @ A
    if AtA[0, 0] * AtA[1, 1] - AtA[0, 1] * AtA[1, 0] < 0.000001:
        return False, 0.0
    return True, abs(float((-np.linalg.inv(AtA) @ A.T @ T_search_ref[4:])[0]))


def compute_tau(T_ref_cur, f, z, px_error_angle):
    """src/depth_filter.cpp:568-584 (PI of include/plsvo/global.h)"""
    t = np.asarray(T_ref_cur[4:], float)
    a = f * z - t
    t_norm, a_norm = math.sqrt(t @ t), math.sqrt(a @ a)
    alpha = math.acos(f @ t / t_norm)
    beta = math.acos(a @ (-t) / (t_norm * a_norm))
    beta_plus = beta + px_error_angle
    gamma_plus = 3.14159265 - alpha - beta_plus
    return t_norm * math.sin(beta_plus) / math.sin(gamma_plus) - z


def tau2_of(T_ref_cur, f, z, px_error_angle):
    """the measurement (x, tau2) handed to the posterior: :320-324"""
    tau = compute_tau(T_ref_cur, f, z, px_error_angle)
    tau_inverse = 0.5 * (1.0 / max(0.0000001, z - tau) - 1.0 / (z + tau))
    with np.errstate(all="ignore"):
        return f32(1.0 / z), f32(tau_inverse * tau_inverse)


def _pdf(x, mean, sd):
    """boost::math::pdf(normal_distribution<float>(mean, sd), x), all in float"""
    if np.isinf(x):
        return f32(0)
    e = f32(x - mean)
    e = f32(e * f32(-e))
    e = f32(e / f32(f32(f32(2) * sd) * sd))
    r = f32(np.exp(f64(e)))                     # the correctly rounded float exp
    return f32(r / f32(sd * f32(np.sqrt(f32(f32(2) * f32(math.pi))))))


def posterior_end(x, tau2, a, b, z_range, mu, sigma2):
    """one end of updatePointSeed (:495-509) / updateLineSeed (:524-553) in the reference's float / double mix: every operator with a
    double literal (1., 2.) is evaluated in double, the others in float, every assignment rounds to float -> (mu, sigma2, f, e)"""
    x, tau2, a, b, z_range, mu, sigma2 = (f32(v) for v in (x, tau2, a, b, z_range, mu, sigma2))
    norm_scale = f32(np.sqrt(f32(sigma2 + tau2)))
    pdf = _pdf(x, mu, norm_scale)
    s2 = f32(1.0 / (1.0 / f64(sigma2) + 1.0 / f64(tau2)))
    m = f32(s2 * f32(f32(mu / sigma2) + f32(x / tau2)))
    ab = f32(a + b)
    C1 = f32(f32(a / ab) * pdf)
    C2 = f32(f64(f32(b / ab)) * 1.0 / f64(z_range))
    nc = f32(C1 + C2)
    C1, C2 = f32(C1 / nc), f32(C2 / nc)
    a_, b_, C1_, C2_ = f64(a), f64(b), f64(C1), f64(C2)
    ab1_ = f64(ab) + 1.0                                            # (seed->a+seed->b+1.): the float sum, then + 1. in double
    f = f32(C1_ * (a_ + 1.0) / ab1_ + f64(f32(C2 * a)) / ab1_)
    ab1, ab2 = f32(ab + f32(1)), f32(ab + f32(2))
    e = f32(C1_ * (a_ + 1.0) * (a_ + 2.0) / (ab1_ * (f64(ab) + 2.0)) + f64(f32(f32(f32(C2 * a) * f32(a + f32(1))) / f32(ab1 * ab2))))
    mu_new = f32(f32(C1 * m) + f32(C2 * mu))
    sigma2_new = f32(f32(f32(C1 * f32(s2 + f32(m * m))) + f32(C2 * f32(sigma2 + f32(mu * mu)))) - f32(mu_new * mu_new))
    return mu_new, sigma2_new, f, e


def _beta(f, e):
    a = f32(f32(e - f) / f32(f - f32(e / f)))
    return a, f32(f32(a * f32(f32(1) - f)) / f)


def epipolar_search(cam, T_ref, T_cur, ref_pyr, cur_pyr, px, f, level, ftype, grad, d_estimate, d_min, d_max, endpoint, opt):
    """findEpipolarMatchDirect (endpoint False, :277-420) / findEpipolarMatchDirectSegmentEndpoint (endpoint True, :422-586) with
    align2D and sub-pixel refinement, the reference's defaults -> (ok, depth, px_cur, record)"""
    fx, fy, cx, cy, W, H = cam
    W, H = int(W), int(H)
    level = int(level)
    rec = new_record(level)
    px_cur = np.zeros(2)

    def done(exit_, ok=False, depth=0.0):
        rec["exit"] = exit_
        return ok, depth, px_cur, rec
    T_cur_ref = npr.se3_mul(T_cur, se3_inv(T_ref))
    if endpoint and (math.isnan(d_min) or math.isnan(d_max)):
        return done("nan_bounds")
    with np.errstate(all="ignore"):
        pa, pb_ = npr.se3_act(T_cur_ref, f * d_min), npr.se3_act(T_cur_ref, f * d_max)
        A, B = pa[:2] / pa[2], pb_[:2] / pb_[2]
        epi_dir = A - B
        Aw = tm._np_warp_matrix(cam, px, f, d_estimate, T_cur_ref, level)
        if not endpoint and ftype == 1 and opt["edgelet_filtering"]:
            g = Aw @ np.asarray(grad, float)
            g = g / np.linalg.norm(g)
            if abs(g @ (epi_dir / np.linalg.norm(epi_dir))) < opt["edgelet_max_angle"]:
                return done("edgelet_reject")
        D = Aw[0, 0] * Aw[1, 1] - Aw[1, 0] * Aw[0, 1]
        sl = 0
        while D > 3.0 and sl < opt["n_pyr_levels"] - 1:
            sl += 1
            D *= 0.25
        rec["search_level"] = sl
        px_A = np.array([fx * A[0] + cx, fy * A[1] + cy])
        px_B = np.array([fx * B[0] + cx, fy * B[1] + cy])
        epi_length = float(np.linalg.norm(px_A - px_B)) / (1 << sl)
    if not math.isfinite(epi_length):
        return done("epi_nonfinite")
    with np.errstate(all="ignore"):
        inv00 = f32(Aw[1, 1] * (1.0 / (Aw[0, 0] * Aw[1, 1] - Aw[1, 0] * Aw[0, 1])))
    if np.isnan(inv00):
        return done("warp_fail")
    pb = tm._np_warp_affine(Aw, ref_pyr[level], px, level, sl)
    cur = cur_pyr[sl]
    rows, cols = cur.shape
    scale = 1 << sl

    def finish(start, kind):
        nonlocal px_cur
        px_cur = np.array(start, float)
        ok, _, e = tm._np_align2d(cur, pb, opt["align_max_iter"], (px_cur[0] / scale, px_cur[1] / scale))
        if not ok:
            return done(kind + "_align_fail")
        px_cur = np.array([e[0] * scale, e[1] * scale])
        r = np.array([(px_cur[0] - cx) / fx, (px_cur[1] - cy) / fy, 1.0])
        ok, depth = depth_from_triangulation(T_cur_ref, f, r / np.linalg.norm(r))
        return done(kind + "_ok", True, depth) if ok else done(kind + "_tri_fail")
    if epi_length < 2.0:
        return finish((px_A + px_B) / 2.0, "short")
    n_steps = int(epi_length / 0.7)
    rec["n_steps"] = n_steps
    step = epi_dir / float(n_steps)
    if n_steps > opt["max_epi_search_steps"]:
        return done("too_many_steps")
    ref = pb[1:9, 1:9].astype(np.int64).ravel()
    sA, sAA = int(ref.sum()), int((ref * ref).sum())
    best, uv_best, best_pxi, last = THRESHOLD, None, None, (0, 0)
    scores, phases = [], set()
    uv = B - step
    for _ in range(n_steps + 1):
        q = (fx * uv[0] + cx) / scale + 0.5, (fy * uv[1] + cy) / scale + 0.5
        assert abs(q[0]) < 1e9 and abs(q[1]) < 1e9, "a walk position beyond the int range: undefined in the reference"
        pxi = (int(q[0]), int(q[1]))              # Vector2i(double, double): truncation
        if pxi == last:
            rec["n_repeat_skipped"] += 1
        else:
            last = pxi
            if 8 <= pxi[0] < W // scale - 8 and 8 <= pxi[1] < H // scale - 8:       # isInFrame(pxi, patch_size_ = 8, search_level_)
                Bp = cur[pxi[1] - 4:pxi[1] + 4, pxi[0] - 4:pxi[0] + 4].astype(np.int64).ravel()
                sB = int(Bp.sum())
                num = sA * sA - 2 * sA * sB + sB * sB
                sc = sAA - 2 * int((ref * Bp).sum()) + int((Bp * Bp).sum()) - num // 64
                rec["n_scored"] += 1
                scores.append(sc)
                phases |= {((pxi[1] - 4 + r) * cols + (pxi[0] - 4)) & 3 for r in range(8)}
                if sc < best:
                    best, uv_best, best_pxi = sc, uv.copy(), pxi
            else:
                rec["n_out_of_frame_skipped"] += 1
        uv = uv + step
    rec["row_phases"] = frozenset(phases)
    if best < THRESHOLD:
        rec["n_positions_at_best"] = scores.count(best)
        ph = [((best_pxi[1] - 4 + r) * cols + (best_pxi[0] - 4)) & 3 for r in range(8)]
        rec["first_row_phase_best"], rec["row_phases_best"] = ph[0], frozenset(ph)
        return finish((fx * uv_best[0] + cx, fy * uv_best[1] + cy), "walk")
    return done("no_score_below_threshold")


def _in_image(cam, xyz):
    fx, fy, cx, cy, W, H = cam
    with np.errstate(all="ignore"):
        u, v = fx * (xyz[0] / xyz[2]) + cx, fy * (xyz[1] / xyz[2]) + cy
    if not (abs(u) < 1e9 and abs(v) < 1e9):
        return False
    return 0 <= int(u) < W and 0 <= int(v) < H           # isInFrame(f2c(xyz).cast<int>())


def _bounds(mu, sigma2):
    """:307-311: z_inv_min, z_inv_max in float; d_estimate, d_min, d_max in double"""
    with np.errstate(all="ignore"):
        root = f32(np.sqrt(sigma2))
        z_inv_min = f32(mu + root)
        z_inv_max = max(f32(mu - root), f32(0.00000001))          # std::max(NaN, c) = NaN
        return z_inv_min, 1.0 / f64(mu), 1.0 / f64(z_inv_min), 1.0 / f64(z_inv_max)


def update_point_seed(cam, T_ref, T_cur, ref_pyr, cur_pyr, s, opt):
    """DepthFilter::updatePointSeeds for one seed (:295-360).  s: px, f, level, type, grad, a, b, mu, z_range, sigma2 -> (result, record)"""
    a, b, mu, z_range, sigma2 = (f32(s[k]) for k in ("a", "b", "mu", "z_range", "sigma2"))
    f = np.asarray(s["f"], float)
    out = dict(status=NOT_VISIBLE, a=a, b=b, mu=mu, sigma2=sigma2, xyz_world=np.zeros(3), px_cur=np.zeros(2), depth=0.0)
    T_ref_cur = npr.se3_mul(T_ref, se3_inv(T_cur))
    with np.errstate(all="ignore"):
        xyz_f = npr.se3_act(se3_inv(T_ref_cur), (1.0 / f64(mu)) * f)
    if xyz_f[2] < 0.0 or not _in_image(cam, xyz_f):
        return out, new_record(s["level"], "invisible")
    z_inv_min, d_est, d_min, d_max = _bounds(mu, sigma2)
    ok, z, px_cur, rec = epipolar_search(cam, T_ref, T_cur, ref_pyr, cur_pyr, np.asarray(s["px"], float), f, s["level"], int(s["type"]), s["grad"],
                                         d_est, d_min, d_max, False, opt)
    out["px_cur"], out["depth"] = px_cur, z
    if not ok:
        out.update(status=NO_MATCH, b=f32(b + f32(1)))
        return out, rec
    px_error_angle = math.atan(opt["px_noise"] / (2.0 * abs(cam[0]))) * 2.0
    x, tau2 = tau2_of(T_ref_cur, f, z, px_error_angle)
    with np.errstate(all="ignore"):
        if not np.isnan(f32(np.sqrt(f32(sigma2 + tau2)))):
            mu, sigma2, fq, eq = posterior_end(x, tau2, a, b, z_range, mu, sigma2)
            a, b = _beta(fq, eq)
        out.update(status=UPDATED, a=a, b=b, mu=mu, sigma2=sigma2)
        if f32(np.sqrt(sigma2)) < f32(z_range / f32(opt["convergence_sigma2_thresh"])):
            out.update(status=CONVERGED, xyz_world=npr.se3_act(se3_inv(T_ref), f * (1.0 / f64(mu))))
        elif np.isnan(z_inv_min):
            out["status"] = NAN
    return out, rec


def update_line_seed(cam, T_ref, T_cur, ref_pyr, cur_pyr, s, opt):
    """DepthFilter::updateLineSeeds for one seed (:391-470).  s: px, f (segment centre), sf, ef, level, a, b, mu_s, mu_e, z_range_s,
    z_range_e, sigma2_s, sigma2_e -> (result, (record of the first search, record of the second or None))"""
    a, b, mu_s, mu_e, zr_s, zr_e, s2_s, s2_e = (f32(s[k]) for k in ("a", "b", "mu_s", "mu_e", "z_range_s", "z_range_e", "sigma2_s", "sigma2_e"))
    fc, sf, ef = (np.asarray(s[k], float) for k in ("f", "sf", "ef"))
    out = dict(status=NOT_VISIBLE, a=a, b=b, mu_s=mu_s, mu_e=mu_e, sigma2_s=s2_s, sigma2_e=s2_e, xyz_world_s=np.zeros(3), xyz_world_e=np.zeros(3),
               depth_s=0.0, depth_e=0.0)
    T_ref_cur = npr.se3_mul(T_ref, se3_inv(T_cur))
    T_cur_ref = se3_inv(T_ref_cur)
    with np.errstate(all="ignore"):
        xs, xe = npr.se3_act(T_cur_ref, (1.0 / f64(mu_s)) * sf), npr.se3_act(T_cur_ref, (1.0 / f64(mu_e)) * ef)
    if xs[2] < 0.0 or xe[2] < 0.0 or not _in_image(cam, xs) or not _in_image(cam, xe):
        return out, (new_record(s["level"], "invisible"), None)
    zmin_s, de_s, dmin_s, dmax_s = _bounds(mu_s, s2_s)
    zmin_e, de_e, dmin_e, dmax_e = _bounds(mu_e, s2_e)
    px = np.asarray(s["px"], float)
    # both ends are searched from the segment centre's px and bearing (`*it->ftr`, :411-414); `||`: the second only after the first
    ok_s, z_s, _, rec_s = epipolar_search(cam, T_ref, T_cur, ref_pyr, cur_pyr, px, fc, s["level"], 0, (0.0, 0.0), de_s, dmin_s, dmax_s, True, opt)
    out["depth_s"] = z_s
    ok_e, z_e, rec_e = False, 0.0, None
    if ok_s:
        ok_e, z_e, _, rec_e = epipolar_search(cam, T_ref, T_cur, ref_pyr, cur_pyr, px, fc, s["level"], 0, (0.0, 0.0), de_e, dmin_e, dmax_e, True, opt)
        out["depth_e"] = z_e
    if not (ok_s and ok_e):
        out.update(status=NO_MATCH, b=f32(b + f32(1)))
        return out, (rec_s, rec_e)
    px_error_angle = math.atan(opt["px_noise"] / (2.0 * abs(cam[0]))) * 2.0
    x_s, tau2_s = tau2_of(T_ref_cur, sf, z_s, px_error_angle)
    x_e, tau2_e = tau2_of(T_ref_cur, ef, z_e, px_error_angle)
    with np.errstate(all="ignore"):
        if not (np.isnan(f32(np.sqrt(f32(s2_s + tau2_s)))) or np.isnan(f32(np.sqrt(f32(s2_e + tau2_e))))):
            mu_s, s2_s, f_s, e_s = posterior_end(x_s, tau2_s, a, b, zr_s, mu_s, s2_s)
            mu_e, s2_e, f_e, e_e = posterior_end(x_e, tau2_e, a, b, zr_e, mu_e, s2_e)
            (a_s, b_s), (a_e, b_e) = _beta(f_s, e_s), _beta(f_e, e_e)
            a = a_e if a_s < a_e else a_s             # std::max(a_s, a_e)
            b = b_e if b_e < b_s else b_s             # std::min(b_s, b_e)
        out.update(status=UPDATED, a=a, b=b, mu_s=mu_s, mu_e=mu_e, sigma2_s=s2_s, sigma2_e=s2_e)
        thr = f32(opt["convergence_sigma2_thresh"])
        if f32(np.sqrt(s2_s)) < f32(zr_s / thr) and f32(np.sqrt(s2_e)) < f32(zr_e / thr):
            T_w_ref = se3_inv(T_ref)
            out.update(status=CONVERGED, xyz_world_s=npr.se3_act(T_w_ref, sf * (1.0 / f64(mu_s))), xyz_world_e=npr.se3_act(T_w_ref, ef * (1.0 / f64(mu_e))))
        elif np.isnan(zmin_s) or np.isnan(zmin_e):
            out["status"] = NAN
    return out, (rec_s, rec_e)


PT_OUT = (("status", np.int32), ("a", f32), ("b", f32), ("mu", f32), ("sigma2", f32), ("xyz_world", f64), ("px_cur", f64), ("depth", f64))
SEG_OUT = (("status", np.int32), ("a", f32), ("b", f32), ("mu_s", f32), ("mu_e", f32), ("sigma2_s", f32), ("sigma2_e", f32), ("xyz_world_s", f64),
           ("xyz_world_e", f64), ("depth_s", f64), ("depth_e", f64))


def update_seeds(cam, frame_T, frames, pt, seg, **options):
    """plsvo_update_seeds in NumPy.  frames[k]: the pyramid of frame k; pt / seg: the field dicts of abi.SeedsJob (or None); options as
    abi.SeedsJob's.  Returns (dict with the fields of plsvo_update_seeds except seg px, point records, line records (first, second))."""
    opt = dict(DEFAULTS, **options)
    frame_T = np.asarray(frame_T, float).reshape(-1, 7)
    res, pt_rec, seg_rec = {}, [], []
    for prefix, d, fn, spec, recs in (("pt_", pt, update_point_seed, PT_OUT, pt_rec), ("seg_", seg, update_line_seed, SEG_OUT, seg_rec)):
        rows = []
        for i in range(len(d["px"]) if d else 0):
            rf, cf = int(d["ref_frame"][i]), int(d["cur_frame"][i])
            s = {k: v[i] for k, v in d.items()}
            if prefix == "pt_":
                s.setdefault("type", 0)
                s.setdefault("grad", (0.0, 0.0))
            o, r = fn(cam, frame_T[rf], frame_T[cf], frames[rf], frames[cf], s, opt)
            rows.append(o)
            recs.append(r)
        for k, dt in spec:
            width = 3 if k.startswith("xyz") else 2 if k.startswith("px") else 0
            res[prefix + k] = np.array([r[k] for r in rows], dtype=dt).reshape((len(rows), width) if width else (len(rows),))
    return res, pt_rec, seg_rec


def np_update_point_seed_once(P, seq, frames, i, pt, cur_k, n_pyr_levels=3, max_steps=1000):
    """one point seed of a sequence.make_sequence sequence against frame cur_k -> (status class: 0 invisible, 1 no match, 2 matched,
    triangulated depth); the restatement tests/test_depth_filter.py pins the oracle's point search with"""
    T = seq["poses_true"]
    s = {k: pt[k][i] for k in ("px", "f", "level", "type", "grad", "a", "b", "mu", "z_range", "sigma2")}
    out, _ = update_point_seed(seq["cam"], T[0], T[cur_k], frames[0], frames[cur_k], s, dict(DEFAULTS, n_pyr_levels=n_pyr_levels, max_epi_search_steps=max_steps))
    return min(int(out["status"]), 2), out["depth"]
