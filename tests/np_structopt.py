"""Restatement of the structure optimiser that records the PATH it took (test infrastructure only).

  * `solve3` -- A.ldlt().solve(b) of Eigen 3.1 ... 3.2.1 (oracle flavour 320; the device implements no other for the 3x3 solve): an
    instrumented copy of np_restatement.eigen32_ldlt_solve, written from the mathematics (permute by a selection sort of the ORIGINAL
    diagonal, factor without pivoting, pseudo-inverse of D), not from the in-place code of oracle/plsvo_oracle.c::ldlt_solve_n nor from
    the unrolled scalars of pl-svo_amd/csrc/structopt_kernels.hip::ldlt_solve3.  Besides x it returns a SolveRecord.
  * `point_optimize`, `segment_optimize` -- plsvo::Point::optimize / LineSeg::optimize (reference src/feature3D_impl.cpp:36-95, :97-174,
    Point::jacobian_xyz2uv include/plsvo/feature3D.h:126-140) term by term in the order of the reference source, on float64 scalars:
    no BLAS, no matrix product whose summation order is somebody else's.  They return the position(s), the iteration count, the exit
    taken and every solve's record.

Everything is IEEE double arithmetic on numpy scalars (Python floats raise on a division by zero; these must produce Inf/NaN)."""
import collections

import numpy as np

F = np.float64
EPS_DBL = F(np.finfo(np.float64).eps)
TINY = F(1.0) / F(np.finfo(np.float64).max)      # 1 / highest()
EPS_CONV = F(0.0000000001)                         # EPS, include/plsvo/global.h:99

# order      original indices in the order the pivots took them; where the factorisation stopped the rest keep their stored order
# ties       per executed pivot search: the maximum was attained by more than one candidate (the first one wins)
# stop_at    step at which "the largest remaining stored diagonal is below the cutoff" ended the factorisation (n: it ran to the end)
# scaled     per column k < n-1: divided by its pivot (|D_k| > cutoff); False also for the columns never reached
# zeroed     per D entry: the solve returned 0 for that component (|D_i| <= tolerance)
# rel_zeroed per D entry: zeroed although |D_i| > 1/DBL_MAX -- the relative tolerance max|D| * eps did it, the floor alone would have kept it
# tol_floor  the tolerance of the solve was 1/DBL_MAX, not max|D| * eps
SolveRecord = collections.namedtuple("SolveRecord", "order ties stop_at scaled zeroed rel_zeroed tol_floor")


def solve3(A, b):
    """x, SolveRecord = A.ldlt().solve(b), Eigen 3.2's zero-pivot rule; only the lower triangle of A is read"""
    with np.errstate(all="ignore"):
        A = np.array(A, dtype=np.float64)
        n = A.shape[0]
        order = list(range(n))
        cutoff = F(0.0)
        stop_at = n
        ties = []
        for k in range(n):                       # selection sort of the original diagonal, with Eigen's stopping rule
            cand = [abs(A[order[j], order[j]]) for j in range(k, n)]
            best, bestv = k, cand[0]
            for j in range(k + 1, n):
                if cand[j - k] > bestv:
                    best, bestv = j, cand[j - k]
            if k == 0:
                cutoff = abs(EPS_DBL * bestv)
            if bestv < cutoff:
                stop_at = k
                break
            ties.append(sum(1 for v in cand if v == bestv) > 1)
            order[k], order[best] = order[best], order[k]
        a = np.empty((n, n))
        for i in range(n):                       # P A P^T from the lower triangle of A alone
            for j in range(i + 1):
                hi, lo = max(order[i], order[j]), min(order[i], order[j])
                a[i, j] = a[j, i] = A[hi, lo]
        L = np.tril(a, -1).copy()                # unprocessed columns keep the stored (raw) entries, like the in-place algorithm
        D = np.diag(a).copy()
        scaled = [False] * (n - 1)
        for k in range(stop_at):
            temp = [D[j] * L[k, j] for j in range(k)]
            if k > 0:
                acc = F(0.0)
                for j in range(k):
                    acc += L[k, j] * temp[j]
                D[k] = a[k, k] - acc
                for i in range(k + 1, n):
                    acc = F(0.0)
                    for j in range(k):
                        acc += L[i, j] * temp[j]
                    L[i, k] = a[i, k] - acc
            if k < n - 1 and abs(D[k]) > cutoff:
                scaled[k] = True
                for i in range(k + 1, n):
                    L[i, k] = L[i, k] / D[k]
        y = np.array([b[order[i]] for i in range(n)], dtype=np.float64)
        for i in range(n):
            for j in range(i):
                y[i] -= L[i, j] * y[j]
        maxd = abs(D[0])
        for i in range(1, n):
            if abs(D[i]) > maxd:
                maxd = abs(D[i])
        floor = not (maxd * EPS_DBL > TINY)
        tol = TINY if floor else maxd * EPS_DBL
        zeroed, rel_zeroed = [], []
        for i in range(n):
            keep = abs(D[i]) > tol
            zeroed.append(not keep)
            rel_zeroed.append(bool(not keep and abs(D[i]) > TINY))
            y[i] = y[i] / D[i] if keep else F(0.0)
        for i in range(n - 1, -1, -1):
            for j in range(i + 1, n):
                y[i] -= L[j, i] * y[j]
        x = np.empty(n)
        for i in range(n):
            x[order[i]] = y[i]
    return x, SolveRecord(tuple(order), tuple(ties), stop_at, tuple(scaled), tuple(zeroed), tuple(rel_zeroed), bool(floor))


def _rotation_matrix(q):
    """Sophus SE3::rotation_matrix() = Eigen::Quaternion::toRotationMatrix(), q = (x, y, z, w)"""
    x, y, z, w = (F(v) for v in q)
    tx, ty, tz = F(2.0) * x, F(2.0) * y, F(2.0) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[F(1.0) - (tyy + tzz), txy - twz, txz + twy],
            [txy + twz, F(1.0) - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, F(1.0) - (txx + tyy)]]


def _transform(T, v):
    """T_f_w * p: Eigen::Quaternion::_transformVector (uv = 2 q.vec x v; v + w uv + q.vec x uv), then + translation"""
    qx, qy, qz, qw = (F(t) for t in T[:4])
    ux, uy, uz = qy * v[2] - qz * v[1], qz * v[0] - qx * v[2], qx * v[1] - qy * v[0]
    ux, uy, uz = F(2.0) * ux, F(2.0) * uy, F(2.0) * uz
    r = [v[0] + qw * ux + (qy * uz - qz * uy), v[1] + qw * uy + (qz * ux - qx * uz), v[2] + qw * uz + (qx * uy - qy * ux)]
    return [r[0] + F(T[4]), r[1] + F(T[5]), r[2] + F(T[6])]


def _accumulate(T, f, pos, A, b):
    """one observation, feature3D_impl.cpp:52-58: returns e.squaredNorm(); A += J^T J, b -= J^T e in place"""
    p = _transform(T, pos)
    R = _rotation_matrix(T[:4])
    z_inv = F(1.0) / p[2]                                    # jacobian_xyz2uv, feature3D.h:131-139
    z_inv_sq = z_inv * z_inv
    P = [[z_inv, F(0.0), -p[0] * z_inv_sq], [F(0.0), z_inv, -p[1] * z_inv_sq]]
    J = [[(-P[r][0]) * R[0][c] + (-P[r][1]) * R[1][c] + (-P[r][2]) * R[2][c] for c in range(3)] for r in range(2)]   # (-point_jac) * R_f_w
    e = [F(f[0]) / F(f[2]) - p[0] / p[2], F(f[1]) / F(f[2]) - p[1] / p[2]]   # vk::project2d(f) - vk::project2d(p_in_f)
    for i in range(3):
        for j in range(3):
            A[i][j] = A[i][j] + (J[0][i] * J[0][j] + J[1][i] * J[1][j])
        b[i] = b[i] - (J[0][i] * e[0] + J[1][i] * e[1])
    return e[0] * e[0] + e[1] * e[1]


def _norm_max(v):
    """vk::norm_max: the largest |component|; a NaN never compares greater and is passed over"""
    m = F(0.0)
    for t in v:
        if abs(t) > m:
            m = abs(t)
    return m


# exit       one of EXITS
# ends       segments only: which end(s) triggered the roll-back or the stop: "s", "e" or "both" ("" for the exits without a trigger)
# solves     the SolveRecord of every solve, in call order (segments: start point, end point per iteration)
# nan_written  an accepted step had a non-NaN dp[0] and a NaN in dp[1] or dp[2] (the reference then writes the NaN into the position)
# nan_written_finite  ... and dp[0] was finite
OptRecord = collections.namedtuple("OptRecord", "exit ends solves nan_written nan_written_finite")
EXITS = ("n_iter_0", "no_obs", "max_iter", "converged_0", "converged_later", "chi2_rose", "nan_0", "nan_later")


def _nan_written(dp):
    other = bool(np.isnan(dp[1]) or np.isnan(dp[2]))
    return (not np.isnan(dp[0])) and other, bool(np.isfinite(dp[0])) and other


def point_optimize(frame_T, pos, obs_frame, obs_f, n_iter):
    """Point::optimize :36-95 -> (pos [3], residual evaluations executed, OptRecord)"""
    with np.errstate(all="ignore"):
        pos = [F(v) for v in pos]
        old_point = list(pos)
        chi2, iters, solves = F(0.0), 0, []
        exit_, nw, nwf = ("n_iter_0" if n_iter == 0 else "max_iter"), False, False
        for it in range(n_iter):
            A, b, new_chi2 = [[F(0.0)] * 3 for _ in range(3)], [F(0.0)] * 3, F(0.0)
            iters += 1
            for fr, f in zip(obs_frame, obs_f):
                new_chi2 = new_chi2 + _accumulate(frame_T[fr], f, pos, A, b)
            dp, rec = solve3(A, b)
            solves.append(rec)
            rose, nan = it > 0 and new_chi2 > chi2, bool(np.isnan(dp[0]))
            if rose or nan:
                # roll-back :71: old_point is the position from BEFORE the last accepted step, not the one that step produced -- a rise of
                # chi2 at iteration k undoes the step of iteration k-1; at iteration 0 it is the input
                pos = list(old_point)
                exit_ = ("nan_0" if it == 0 else "nan_later") if nan else "chi2_rose"
                break
            a, c = _nan_written(dp)
            nw, nwf = nw or a, nwf or c
            old_point = list(pos)
            pos = [pos[k] + dp[k] for k in range(3)]
            chi2 = new_chi2
            if _norm_max(dp) <= EPS_CONV:
                exit_ = "no_obs" if len(obs_frame) == 0 else ("converged_0" if it == 0 else "converged_later")
                break
    return np.array(pos), iters, OptRecord(exit_, "", tuple(solves), nw, nwf)


def segment_optimize(frame_T, spos, epos, obs_frame, obs_sf, obs_ef, n_iter):
    """LineSeg::optimize :97-174 -> (spos [3], epos [3], residual evaluations executed, OptRecord)"""
    def which(s, e):
        return "both" if s and e else ("s" if s else "e")
    with np.errstate(all="ignore"):
        sp, ep = [F(v) for v in spos], [F(v) for v in epos]
        old_s, old_e = list(sp), list(ep)
        chi2s, chi2e, iters, solves = F(0.0), F(0.0), 0, []
        exit_, ends, nw, nwf = ("n_iter_0" if n_iter == 0 else "max_iter"), "", False, False
        for it in range(n_iter):
            As, Ae = [[F(0.0)] * 3 for _ in range(3)], [[F(0.0)] * 3 for _ in range(3)]
            bs, be, ncs, nce = [F(0.0)] * 3, [F(0.0)] * 3, F(0.0), F(0.0)
            iters += 1
            for fr, sf, ef in zip(obs_frame, obs_sf, obs_ef):
                ncs = ncs + _accumulate(frame_T[fr], sf, sp, As, bs)
                nce = nce + _accumulate(frame_T[fr], ef, ep, Ae, be)
            dps, rs = solve3(As, bs)
            dpe, re_ = solve3(Ae, be)
            solves += [rs, re_]
            rose_s, rose_e = it > 0 and ncs > chi2s, it > 0 and nce > chi2e
            nan_s, nan_e = bool(np.isnan(dps[0])), bool(np.isnan(dpe[0]))
            if rose_s or nan_s or rose_e or nan_e:
                # roll-back :144-145: BOTH ends return to their positions from before the last accepted step, whichever end triggered
                sp, ep = list(old_s), list(old_e)
                if nan_s or nan_e:
                    exit_, ends = ("nan_0" if it == 0 else "nan_later"), which(nan_s, nan_e)
                else:
                    exit_, ends = "chi2_rose", which(rose_s, rose_e)
                break
            for dp in (dps, dpe):
                a, c = _nan_written(dp)
                nw, nwf = nw or a, nwf or c
            old_s, old_e = list(sp), list(ep)
            sp = [sp[k] + dps[k] for k in range(3)]
            ep = [ep[k] + dpe[k] for k in range(3)]
            chi2s, chi2e = ncs, nce
            cs, ce = _norm_max(dps) <= EPS_CONV, _norm_max(dpe) <= EPS_CONV
            if cs or ce:                                     # :167 either end at rest stops both
                exit_ = "no_obs" if len(obs_frame) == 0 else ("converged_0" if it == 0 else "converged_later")
                ends = which(cs, ce)
                break
    return np.array(sp), np.array(ep), iters, OptRecord(exit_, ends, tuple(solves), nw, nwf)


def optimize_batch(d, n_iter_pts=5, n_iter_segs=5):
    """the whole batch (the dict of plsvo_structopt_in arrays that synth.make_structure_batch returns) -> dict like the oracle's
    structure_optimize plus pt_rec / seg_rec, the OptRecords"""
    T = np.asarray(d["frame_T"], np.float64).reshape(-1, 7)
    n_pts, n_seg = len(d["pt_obs_off"]) - 1, len(d["seg_obs_off"]) - 1
    out = dict(pt_pos=np.zeros((n_pts, 3)), pt_iters=np.zeros(n_pts, np.int32), seg_spos=np.zeros((n_seg, 3)), seg_epos=np.zeros((n_seg, 3)),
               seg_iters=np.zeros(n_seg, np.int32), pt_rec=[], seg_rec=[])
    for i in range(n_pts):
        o0, o1 = d["pt_obs_off"][i], d["pt_obs_off"][i + 1]
        out["pt_pos"][i], out["pt_iters"][i], r = point_optimize(T, np.reshape(d["pt_pos"], (-1, 3))[i], d["pt_obs_frame"][o0:o1],
                                                                 np.reshape(d["pt_obs_f"], (-1, 3))[o0:o1], n_iter_pts)
        out["pt_rec"].append(r)
    for i in range(n_seg):
        o0, o1 = d["seg_obs_off"][i], d["seg_obs_off"][i + 1]
        out["seg_spos"][i], out["seg_epos"][i], out["seg_iters"][i], r = segment_optimize(
            T, np.reshape(d["seg_spos"], (-1, 3))[i], np.reshape(d["seg_epos"], (-1, 3))[i], d["seg_obs_frame"][o0:o1],
            np.reshape(d["seg_obs_sf"], (-1, 3))[o0:o1], np.reshape(d["seg_obs_ef"], (-1, 3))[o0:o1], n_iter_segs)
        out["seg_rec"].append(r)
    return out
