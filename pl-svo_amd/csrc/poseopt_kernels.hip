// poseopt_kernels.hip -- motion-only pose optimisation on gfx950: one workgroup per frame, the scale
// pass, all Gauss-Newton iterations, the covariance, the outlier cull and the medians run in ONE launch.
//
// Replaces (reference file:line):
//   plsvo::pose_optimizer::optimizeGaussNewton, 9-argument   src/pose_optimizer.cpp:38-260
//   plsvo::pose_optimizer::optimizeGaussNewton, 10-argument  src/pose_optimizer.cpp:262-582
//   [ext] vk::robust_cost::MADScaleEstimator / TukeyWeightFunction, vk::getMedian, Eigen ldlt()/inverse()
//
// Work per call is tiny (hundreds of features x ~100 flops x <=10 iterations): this kernel is
// latency-bound by construction; it exists so that a batch of frames is one launch and the pose never
// leaves the device between the alignment and the optimisation.  One lane per feature, lane-private
// 6x6 (upper) + 6x1 accumulators in double, fixed-shape reduction (butterfly reduce-scatter inside the DPP
// rows, rows and waves through LDS), wave-cooperative 6x6 solve.  The workgroup is ONE wave per frame for
// large batches (nothing to gain from cross-wave work on ~300 features: 8 frames per CU) and four waves for
// small ones (the Gauss-Newton loop of a single frame is then ~2x shorter).
// Medians (vk::getMedian = element floor(n/2) of the sorted vector) are exact: block-wide radix
// select over the IEEE bit patterns (all values are non-negative), 8 bits per pass.
#include <hip/hip_runtime.h>

#include "plsvo_dev.hpp"
#include "plsvo_math.hpp"
#include "plsvo_wave.hpp"
#include "poseopt_refill.hpp"
#include "poseopt_select.hpp"

// Waves per SIMD.  The wave-per-frame shape (64 threads) is capped at 168 VGPRs = THREE waves per SIMD: its feature loops stay spill-free
// (the 58 spilled registers are touched ~20 times per Gauss-Newton iteration, around the solve) and the f64 division chains of a third
// wave fill latency the other two leave: 500 + 200 features x 32768 frames 3.26 -> 3.19 ms.  The row shape LOSES 9 % at three waves
// (1.40 -> 1.53 ms at 200 + 80: four frames' serial code per wave meets the spills) and both lose 2x at four; measured on one MI355X box,
// profiles/r05_poseopt_experiments.log.  -DPLSVO_POSEOPT_WAVES=n / -DPLSVO_POSEOPT_ROWS_WAVES=n rebuild the experiment.
#ifndef PLSVO_POSEOPT_WAVES
#define PLSVO_POSEOPT_WAVES 3
#endif
#ifdef PLSVO_WAVE_EMU   // (the host emulation build, tests/host/: kernels are plain functions there)
#define PLSVO_PO_OCC(T)
#else
#define PLSVO_PO_OCC(T) __attribute__((amdgpu_waves_per_eu((T) == 64 ? PLSVO_POSEOPT_WAVES : 1, (T) == 64 ? PLSVO_POSEOPT_WAVES : 8)))
#endif
#if defined(PLSVO_POSEOPT_ROWS_WAVES) && !defined(PLSVO_WAVE_EMU)
#define PLSVO_PO_ROWS_OCC __attribute__((amdgpu_waves_per_eu(PLSVO_POSEOPT_ROWS_WAVES, PLSVO_POSEOPT_ROWS_WAVES)))
#else
#define PLSVO_PO_ROWS_OCC
#endif
namespace plsvo_hip {

// optional per-phase timing (compile with -DPLSVO_TIMING): thread 0 accumulates s_memtime deltas
#ifdef PLSVO_TIMING
#define PTICK(slot) do { if (threadIdx.x == 0) { const unsigned long long t__ = __builtin_amdgcn_s_memtime(); s_time[slot] += t__ - s_tlast; s_tlast = t__; } } while (0)
#else
#define PTICK(slot) do { } while (0)
#endif

#define PO_RED 32
#ifndef PO_RADIX_BITS
#define PO_RADIX_BITS 8    // bits per radix-select pass (measured on MI355X: 8 -> 0.72 ms, 11 -> 0.81 ms, 6 -> 0.74 ms per 8192 frames)
#endif
#define PO_BINS (1 << PO_RADIX_BITS)

// k-th smallest (0-based) of n non-negative IEEE values given as unsigned bit patterns of BITS bits.
// get(i) returns the pattern of element i (invalid elements must return all-ones).
template <int PO_T, int BITS, typename U, typename GET>
__device__ U block_radix_select(GET get, int n, int k, int* s_hist, int* s_sel) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  U prefix = 0, mask = 0;
  int shift = BITS;
  while (shift > 0) {
    const int bits = shift >= PO_RADIX_BITS ? PO_RADIX_BITS : shift;
    shift -= bits;
    const int nb = 1 << bits;
    for (int i = tid; i < PO_BINS; i += PO_T) s_hist[i] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += PO_T) {
      const U v = get(i);
      if ((v & mask) == prefix) atomicAdd(&s_hist[(int)((v >> shift) & (U)(nb - 1))], 1);
    }
    __syncthreads();
    // block scan over the bins: each thread owns PO_BINS/PO_T consecutive bins
    constexpr int PER = PO_BINS >= PO_T ? PO_BINS / PO_T : 1;   // more threads than bins: the surplus threads own no bin
    const bool owner = tid * PER < PO_BINS;
    int loc[PER]; int local = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) { loc[j] = owner ? s_hist[tid * PER + j] : 0; local += loc[j]; }
    int incl = local;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int v = __shfl_up(incl, d, 64); if (lane >= d) incl += v; }
    if (lane == 63) s_sel[4 + wave] = incl;
    __syncthreads();
    int wave_off = 0;
    for (int w = 0; w < wave; ++w) wave_off += s_sel[4 + w];
    int cum = wave_off + incl - local;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      if (owner && k >= cum && k < cum + loc[j]) { s_sel[0] = tid * PER + j; s_sel[1] = k - cum; s_sel[2] = loc[j]; }
      cum += loc[j];
    }
    __syncthreads();
    prefix |= ((U)s_sel[0]) << shift;
    mask |= ((U)(nb - 1)) << shift;
    k = s_sel[1];
    const int survivors = s_sel[2];
    __syncthreads();
    if (survivors == 1 && shift > 0) {
      // one candidate left: it is the answer, the remaining digits need no histogram (typical after 2-3 of the 4 / 8 passes)
      for (int i = tid; i < n; i += PO_T) {
        const U v = get(i);
        if ((v & mask) == prefix) { s_hist[0] = (int)(unsigned)(v & (U)0xffffffffu); s_hist[1] = (int)(unsigned)((unsigned long long)v >> 32); }
      }
      __syncthreads();
      const U r = (U)(((unsigned long long)(unsigned)s_hist[1] << 32) | (unsigned long long)(unsigned)s_hist[0]);
      __syncthreads();
      return r;
    }
  }
  return prefix;
}

// LDS roles: s_red 32*(PO_T/16) doubles (row partials); s_pose 0..8 R, 9..11 t, 12..18 model, 19..25 T_old, 26 chi2;
// s_ctl[0] break flag

// one GN loop (src/pose_optimizer.cpp:103-195 and the identical text at :469-563)
// sqrt(a*a + b*b) in float with every product and the sum rounded on its own (Eigen's Vector2f::norm() in the un-contracted build the
// oracle pins, src/pose_optimizer.cpp:84-87).  HIP's __fmul_rn / __fadd_rn are plain `*` / `+` and hipcc contracts by default: fused,
// the value is one ulp off for some inputs, and when that input is the median line error the MAD scale -- hence every Tukey weight --
// moves by a float ulp (found on the second config-5 seed set: chi2 of the first iteration 2.9e-8 off, tests/test_gpu_parity.py).
__device__ __forceinline__ float norm2_f32(float a, float b) {
#pragma clang fp contract(off)
  const float p = a * a, q = b * b;
  return sqrtf(p + q);
}

// ---- per-feature arithmetic, shared by the workgroup-per-frame kernel and the row-per-frame kernel ----------------------------------
// P[0..8] = R (row-major), P[9..11] = t of the current model.  obs[2f], obs[2f+1] = f.x / f.z, f.y / f.z of point f: the observation's
// normalised coordinates do not depend on the pose, so the scale pass divides once and the Gauss-Newton and cull passes read the two
// quotients back (same operands, same IEEE results: bit-identical, two f64 divisions less per point and pass).

// 1.0 / (1 << level) (the reference's scale of a pyramid level, :119-120): a power of two, written into the exponent -- exact
__device__ __forceinline__ double pow2_neg(int level) { return __hiloint2double((1023 - level) << 20, 0); }

// one feature of a Gauss-Newton iteration (src/pose_optimizer.cpp:107-166 / :473-533): residual, Jacobian, Tukey weight, accumulation
// into acc (0..20 A upper row-major, 21..26 b, 27 chi2, 28 #points, 29 #segments)
__device__ __forceinline__ void popt_accumulate_feature(const PoseBatchDev& b, const PoseJobDev& job, int f, const double (&P)[12], double scale_pt,
                                                        double scale_ls, bool first_iter, double* init_vec, const double* obs, double* acc) {
  const int np = job.n_pts;
  const double R0 = P[0], R1 = P[1], R2 = P[2], R3 = P[3], R4 = P[4], R5 = P[5], R6 = P[6], R7 = P[7], R8 = P[8], t0 = P[9], t1 = P[10], t2 = P[11];
  double J[12], e0, e1, weight, cnt_pt, cnt_ls;   // (the two counters are added at the common tail: `acc[28 + is_segment] += 1` would be a dynamically indexed private array, i.e. scratch)
  if (f < np) {
    const int i = job.pt_off + f;
    if (!b.pt_keep[i]) return;
    const double x = b.pt_pos[3 * i], y = b.pt_pos[3 * i + 1], z = b.pt_pos[3 * i + 2];
    const double xyz[3] = { R0 * x + R1 * y + R2 * z + t0, R3 * x + R4 * y + R5 * z + t1, R6 * x + R7 * y + R8 * z + t2 };
    jacobian_xyz2uv(xyz, J);
    e0 = obs[2 * f] - xyz[0] / xyz[2];
    e1 = obs[2 * f + 1] - xyz[1] / xyz[2];
    const double sic = pow2_neg(b.pt_level[i]);
    e0 *= sic; e1 *= sic;
    if (first_iter) init_vec[f] = e0 * e0 + e1 * e1;
#pragma unroll
    for (int k = 0; k < 12; ++k) J[k] *= sic;
    weight = (double)tukey_weight((float)(sqrt(e0 * e0 + e1 * e1) / scale_pt));
    cnt_pt = 1.0; cnt_ls = 0.0;
  } else {
    const int s = job.seg_off + (f - np);
    if (!b.seg_keep[s]) return;
    double Js[12], Je[12];
    const double sx = b.seg_spos[3 * s], sy = b.seg_spos[3 * s + 1], sz = b.seg_spos[3 * s + 2];
    const double ex = b.seg_epos[3 * s], ey = b.seg_epos[3 * s + 1], ez = b.seg_epos[3 * s + 2];
    const double xs[3] = { R0 * sx + R1 * sy + R2 * sz + t0, R3 * sx + R4 * sy + R5 * sz + t1, R6 * sx + R7 * sy + R8 * sz + t2 };
    const double xe[3] = { R0 * ex + R1 * ey + R2 * ez + t0, R3 * ex + R4 * ey + R5 * ez + t1, R6 * ex + R7 * ey + R8 * ez + t2 };
    jacobian_xyz2uv(xs, Js);
    jacobian_xyz2uv(xe, Je);
    const double l0 = b.seg_line[3 * s], l1 = b.seg_line[3 * s + 1], l2 = b.seg_line[3 * s + 2];
    const float ds = (float)(l0 * (xs[0] / xs[2]) + l1 * (xs[1] / xs[2]) + l2 * 1.0);
    const float de = (float)(l0 * (xe[0] / xe[2]) + l1 * (xe[1] / xe[2]) + l2 * 1.0);
    const double sic = pow2_neg(b.seg_level[s]);
    e0 = (double)ds * sic; e1 = (double)de * sic;
    if (first_iter) init_vec[f] = e0 * e0 + e1 * e1;
    const double en = sqrt(e0 * e0 + e1 * e1);
    const double ks = sic * (double)ds / en;  // same factor for both rows (:156-157)
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      J[c] = l0 * (Js[c] * ks) + l1 * (Js[6 + c] * ks);
      J[6 + c] = l0 * (Je[c] * ks) + l1 * (Je[6 + c] * ks);
    }
    weight = (double)tukey_weight((float)(en / scale_ls));
    cnt_pt = 0.0; cnt_ls = 1.0;
  }
  // A += J^T J w, b -= J^T e w (:163-165): the two rows of J are weighted once (12 products) and every entry is two fused multiply-adds
  // -- 21 x 2 + 6 x 2 + 12 double instructions where (J_i J_j + J'_i J'_j) w, written out, issues 21 x 4 + 6 x 4; the sums differ from the
  // reference's in the last bits of each term only (A, b agree with the oracle to 1e-15).  Measured -2 % per launch; sharing a refined
  // reciprocal between the quotients of one denominator (bit-identical, exponent-guarded) measured +11 % and is not in the tree
  // (profiles/r05_poseopt_experiments.log).
  double wJ[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) wJ[k] = J[k] * weight;
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int jj = i; jj < 6; ++jj) { acc[k] = fma(wJ[i], J[jj], fma(wJ[6 + i], J[6 + jj], acc[k])); ++k; }
#pragma unroll
  for (int i = 0; i < 6; ++i) acc[21 + i] = fma(-wJ[i], e0, fma(-wJ[6 + i], e1, acc[21 + i]));
  acc[27] += (e0 * e0 + e1 * e1) * weight;
  acc[28] += cnt_pt; acc[29] += cnt_ls;
}

// the float error of a feature in the scale pass (:57-87): points sqrt(e0^2 + e1^2) scaled by the level, lines the un-scaled float norm
__device__ __forceinline__ float popt_scale_error(const PoseBatchDev& b, const PoseJobDev& job, int f, const double (&P)[12], double* obs) {
  const int np = job.n_pts;
  const double R0 = P[0], R1 = P[1], R2 = P[2], R3 = P[3], R4 = P[4], R5 = P[5], R6 = P[6], R7 = P[7], R8 = P[8], t0 = P[9], t1 = P[10], t2 = P[11];
  if (f < np) {
    const int i = job.pt_off + f;
    const double x = b.pt_pos[3 * i], y = b.pt_pos[3 * i + 1], z = b.pt_pos[3 * i + 2];
    const double xc = R0 * x + R1 * y + R2 * z + t0, yc = R3 * x + R4 * y + R5 * z + t1, zc = R6 * x + R7 * y + R8 * z + t2;
    const double fz = b.pt_f[3 * i + 2];
    const double ox = b.pt_f[3 * i] / fz, oy = b.pt_f[3 * i + 1] / fz;
    obs[2 * f] = ox; obs[2 * f + 1] = oy;
    double e0 = ox - xc / zc, e1 = oy - yc / zc;
    const double sic = pow2_neg(b.pt_level[i]);
    e0 *= sic; e1 *= sic;
    return (float)sqrt(e0 * e0 + e1 * e1);
  }
  const int s = job.seg_off + (f - np);
  const double sx = b.seg_spos[3 * s], sy = b.seg_spos[3 * s + 1], sz = b.seg_spos[3 * s + 2];
  const double ex = b.seg_epos[3 * s], ey = b.seg_epos[3 * s + 1], ez = b.seg_epos[3 * s + 2];
  const double xs0 = R0 * sx + R1 * sy + R2 * sz + t0, xs1 = R3 * sx + R4 * sy + R5 * sz + t1, xs2 = R6 * sx + R7 * sy + R8 * sz + t2;
  const double xe0 = R0 * ex + R1 * ey + R2 * ez + t0, xe1 = R3 * ex + R4 * ey + R5 * ez + t1, xe2 = R6 * ex + R7 * ey + R8 * ez + t2;
  const double l0 = b.seg_line[3 * s], l1 = b.seg_line[3 * s + 1], l2 = b.seg_line[3 * s + 2];
  const float es = (float)(l0 * (xs0 / xs2) + l1 * (xs1 / xs2) + l2 * 1.0);   // not scaled by the level (:84-87)
  const float ee = (float)(l0 * (xe0 / xe2) + l1 * (xe1 / xe2) + l2 * 1.0);
  return norm2_f32(es, ee);
}

// the cull of one feature (:201-242): clears its keep flag when the error exceeds the threshold, returns the squared error;
// deleted = 1 (point) / 2 (segment) / 0
__device__ __forceinline__ double popt_cull_feature(const PoseBatchDev& b, const PoseJobDev& job, int f, const double (&P)[12], double thr_pt, double thr_ls,
                                                    const double* obs, int& deleted) {
  const int np = job.n_pts;
  const double R0 = P[0], R1 = P[1], R2 = P[2], R3 = P[3], R4 = P[4], R5 = P[5], R6 = P[6], R7 = P[7], R8 = P[8], t0 = P[9], t1 = P[10], t2 = P[11];
  double e0, e1;
  deleted = 0;
  if (f < np) {
    const int i = job.pt_off + f;
    const double x = b.pt_pos[3 * i], y = b.pt_pos[3 * i + 1], z = b.pt_pos[3 * i + 2];
    const double xc = R0 * x + R1 * y + R2 * z + t0, yc = R3 * x + R4 * y + R5 * z + t1, zc = R6 * x + R7 * y + R8 * z + t2;
    e0 = obs[2 * f] - xc / zc; e1 = obs[2 * f + 1] - yc / zc;
    const double sic = pow2_neg(b.pt_level[i]);
    e0 *= sic; e1 *= sic;
    if (sqrt(e0 * e0 + e1 * e1) > thr_pt) { b.pt_keep[i] = 0; deleted = 1; }
  } else {
    const int s = job.seg_off + (f - np);
    const double sx = b.seg_spos[3 * s], sy = b.seg_spos[3 * s + 1], sz = b.seg_spos[3 * s + 2];
    const double ex = b.seg_epos[3 * s], ey = b.seg_epos[3 * s + 1], ez = b.seg_epos[3 * s + 2];
    const double xs0 = R0 * sx + R1 * sy + R2 * sz + t0, xs1 = R3 * sx + R4 * sy + R5 * sz + t1, xs2 = R6 * sx + R7 * sy + R8 * sz + t2;
    const double xe0 = R0 * ex + R1 * ey + R2 * ez + t0, xe1 = R3 * ex + R4 * ey + R5 * ez + t1, xe2 = R6 * ex + R7 * ey + R8 * ez + t2;
    const double l0 = b.seg_line[3 * s], l1 = b.seg_line[3 * s + 1], l2 = b.seg_line[3 * s + 2];
    const double sic = pow2_neg(b.seg_level[s]);
    e0 = (l0 * (xs0 / xs2) + l1 * (xs1 / xs2) + l2 * 1.0) * sic;     // doubles here, no float truncation (:229)
    e1 = (l0 * (xe0 / xe2) + l1 * (xe1 / xe2) + l2 * 1.0) * sic;
    if (sqrt(e0 * e0 + e1 * e1) > thr_ls) { b.seg_keep[s] = 0; deleted = 2; }
  }
  return e0 * e0 + e1 * e1;
}

// ---- what every launch shape does once per frame or per iteration, written once ------------------------------------------------------
// A frame's pose block is 32 doubles of LDS (s_pose of the block shape, PoseRowLds::pose of the row shape): 0..8 R, 9..11 t, 12..18
// model, 19..25 T_old, 26 chi2, 27 point-iterations, 28 line-iterations.

// quat_to_matrix (plsvo_math.hpp) with its contractions WRITTEN OUT, for the row shape.  Every entry of R is a sum of two products, and
// which of the two hipcc fuses into the fma depends on the code around the call (the use counts of the products when the sum is
// visited): inside the single-launch row kernel it was the first one in all three places, inside a kernel that holds the Gauss-Newton
// loop alone it came out as the second for five of the nine entries -- R a last bit off, and with it every later iteration.  The three
// refill kernels must match pose_opt_rows_kernel bit for bit (tests/test_gpu_poseopt_refill.py holds the two together), so no row-shape
// code leaves the choice open.  The block shape (pose_opt_kernel) keeps quat_to_matrix.
#ifdef PLSVO_WAVE_EMU   // (the host emulation build contracts nothing anywhere)
__device__ __forceinline__ void quat_to_matrix_rows(const Quat& q, double* R) { quat_to_matrix(q, R); }
#else
__device__ __forceinline__ void quat_to_matrix_rows(const Quat& q, double* R) {
#pragma clang fp contract(off)
  const double tx = 2.0 * q.x, ty = 2.0 * q.y, tz = 2.0 * q.z;
  const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
  const double tyy = ty * q.y, tzz = tz * q.z;
  R[0] = 1.0 - fma(q.y, ty, tzz); R[1] = fma(q.x, ty, -twz);      R[2] = fma(q.x, tz, twy);
  R[3] = fma(q.x, ty, twz);       R[4] = 1.0 - fma(q.x, tx, tzz); R[5] = fma(q.y, tz, -twx);
  R[6] = fma(q.x, tz, -twy);      R[7] = fma(q.y, tz, twx);       R[8] = 1.0 - fma(q.x, tx, tyy);
}
#endif

// one frame of a launch as its lanes hold it
struct PoseFrame {
  PoseJobDev job;
  PoseStateDev* st;
  int job_id;
  bool valid;                  // row shape: the row's launch slot lies inside the batch
  // scratch: floats [0,np) point errors, [np, np+ns) line errors; doubles [0,nf) init (first loop), [nf,2nf) init (refinement),
  // [2nf,3nf) final, [3nf, 3nf + 2 np) the points' normalised observations
  float* errs;
  double* vec;
  double scale_pt, scale_ls;   // the MAD scales, once the scale pass has run
  int n_del_pt, n_del_ls;      // what the cull deleted, once it has run
};
__device__ __forceinline__ PoseFrame popt_frame(const PoseBatchDev& b, int job_id) {
  PoseFrame F;
  F.job = b.jobs[job_id]; F.st = b.state + job_id; F.job_id = job_id; F.valid = true;
  const size_t fbase = (size_t)F.job.pt_off + (size_t)F.job.seg_off;
  F.errs = b.scratch_f32 + fbase; F.vec = b.scratch_f64 + 5 * fbase;
  F.scale_pt = 1.0; F.scale_ls = 1.0; F.n_del_pt = 0; F.n_del_ls = 0;
  return F;
}

// R | t of `model` into pose[0..11]; ROWS: the pinned rotation rows.  (A template parameter, not an argument: with both calls in one
// function body the optimiser merges their common products ahead of inlining, and the merged ones have lost the right to contract.)
template <bool ROWS>
__device__ __forceinline__ void popt_store_Rt(const SE3d& model, double* pose) {
  if constexpr (ROWS) quat_to_matrix_rows(model.q, pose); else quat_to_matrix(model.q, pose);
  pose[9] = model.t[0]; pose[10] = model.t[1]; pose[11] = model.t[2];
}

// the block shape at one wave per frame, three waves per SIMD: the pose is re-read from LDS for every feature round -- twelve broadcast
// reads against ~250 f64 instructions -- instead of living in 24 registers across the loop; the laundered offset keeps the compiler from
// hoisting the reads
__device__ __forceinline__ void popt_pose_per_round(const double* s_pose, double (&P)[12]) {
  int off = 0;
#ifndef PLSVO_WAVE_EMU
  asm volatile("" : "+v"(off));
#endif
#pragma unroll
  for (int k = 0; k < 12; ++k) P[k] = s_pose[off + k];
}

// one lane, after the solve of iteration `iter` (:173-195): a step whose chi2 rose, or a NaN solve, rolls the model back to T_old and
// stops the loop; otherwise the left update, which stops the loop below EPS.  Writes the pose block.
struct PoseUpdate { SE3d model; int accepted, brk; };
template <bool ROWS>
__device__ __forceinline__ PoseUpdate popt_update_model(double* pose, const double (&dT)[6], double new_chi2, int iter) {
  SE3d model = se3_load(pose + 12);
  int accepted = 1, brk = 0;
  if ((iter > 0 && new_chi2 > pose[26]) || isnan(dT[0])) {            // :173-180
    model = se3_load(pose + 19); accepted = 0; brk = 1;
  } else {
    const SE3d Tn = se3_mul_dev(se3_exp_dev(dT), model);               // :183 left update
    se3_store(model, pose + 19);
    model = Tn; pose[26] = new_chi2;
    if (norm_max6(dT) <= 0.0000000001) brk = 1;                        // EPS, global.h:99
  }
  se3_store(model, pose + 12);
  popt_store_Rt<ROWS>(model, pose);
  return { model, accepted, brk };
}

// a frame's PoseStateDev at the start of a launch (one lane); phase_ticks are the caller's
__device__ __forceinline__ void popt_reset_state(const PoseJobDev& job, PoseStateDev* st) {
  st->log_count = 0; st->status = 0; st->iters = 0; st->iters_ref = 0; st->pt_iters = 0; st->seg_iters = 0;
  st->num_obs_pt = 0; st->num_obs_ls = 0; st->estimated_scale = 0; st->error_init = 0; st->error_final = 0;
  for (int k = 0; k < 36; ++k) st->cov[k] = 0.0;
  for (int k = 0; k < 7; ++k) st->T[k] = job.T0[k];
}

// a frame's results at the end of a launch (one lane).  mi, mf: the patterns of the two f64 medians (:244-249), mi read only where
// has_init; iters: the iteration counts of the two loops
__device__ __forceinline__ void popt_write_result(const PoseBatchDev& b, const PoseFrame& F, double* poses, const double* pose, bool has_init,
                                                  unsigned long long mi, unsigned long long mf, const int* iters) {
  const PoseJobDev& job = F.job;
  PoseStateDev* st = F.st;
  for (int k = 0; k < 7; ++k) st->T[k] = pose[12 + k];
  if (poses) for (int k = 0; k < 7; ++k) poses[7 * F.job_id + k] = pose[12 + k];
  st->error_init = has_init ? sqrt(__longlong_as_double((long long)mi)) * job.fx : 0.0;
  st->error_final = sqrt(__longlong_as_double((long long)mf)) * job.fx;
  st->estimated_scale = F.scale_pt * job.fx;
  st->num_obs_pt = (unsigned long long)(job.n_pts - F.n_del_pt);
  st->num_obs_ls = (unsigned long long)(job.n_seg - F.n_del_ls);
  st->iters = iters[0]; st->iters_ref = iters[1];
  st->pt_iters = (unsigned long long)(pose[27] + 0.5); st->seg_iters = (unsigned long long)(pose[28] + 0.5);
  if (b.work_key) b.work_key[F.job_id] = (int)fmin(pose[27] + pose[28] + 0.5, 2147483647.0);   // what this frame cost: the next launch's sort key
}

// ---- the block shape: one workgroup per frame ------------------------------------------------------------------------------------------
// LDS roles: s_red 32*(PO_T/16) doubles (row partials); s_pose the pose block; s_tot the totals of the last iteration; s_ctl 0 break
// flag, 1 / 2 iterations of the two loops

// one GN loop (src/pose_optimizer.cpp:103-195 and the identical text at :469-563); phase 0 the first loop, 1 the refinement
template <int PO_T>
__device__ void popt_gn_loop(const PoseBatchDev& b, const PoseFrame& F, double* s_red, double* s_pose, double* s_tot, int* s_ctl, int n_iter, int phase) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const PoseJobDev& job = F.job;
  PoseStateDev* st = F.st;
  const int nf = job.n_pts + job.n_seg;
  double* init_vec = F.vec + phase * nf;
  const double* obs = F.vec + 3 * nf;
  for (int iter = 0; iter < n_iter; ++iter) {
    double acc[32];   // 0..20 A (upper, row-major), 21..26 b, 27 chi2, 28 #points, 29 #segments, 30..31 unused
#pragma unroll
    for (int k = 0; k < 32; ++k) acc[k] = 0.0;
    if constexpr (PO_T == 64) {
      for (int f = tid; f < nf; f += PO_T) {
        double P[12];
        popt_pose_per_round(s_pose, P);
        popt_accumulate_feature(b, job, f, P, F.scale_pt, F.scale_ls, iter == 0, init_vec, obs, acc);
      }
    } else {
      double P[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) P[k] = s_pose[k];
      for (int f = tid; f < nf; f += PO_T) popt_accumulate_feature(b, job, f, P, F.scale_pt, F.scale_ls, iter == 0, init_vec, obs, acc);
    }
    {
      double out2[2];
      row_reduce_scatter32(acc, out2);
      *reinterpret_cast<double2*>(s_red + (tid >> 4) * 32 + row_reduce_scatter32_index(lane)) = make_double2(out2[0], out2[1]);
    }
    __syncthreads();
    if (wave == 0) {
      const double tot = reduce_rows_finish<PO_T / 16>(s_red);
      if (lane < 30) s_tot[lane] = tot;
      double dT[6];
      wave_solve6_reg(tot, dT, job.ldlt_flavour);                            // A.ldlt().solve(b) :170
      const double new_chi2 = readlane_f64(tot, 27), npt = readlane_f64(tot, 28), nls = readlane_f64(tot, 29);
      if (lane == 0) {
        s_pose[27] += npt; s_pose[28] += nls;
        s_ctl[1 + phase] += 1;
        const PoseUpdate u = popt_update_model<false>(s_pose, dT, new_chi2, iter);
        s_ctl[0] = u.brk;
        if (b.log) {
          const int lc = st->log_count;
          if (lc < b.log_cap) {
            plsvo_poseopt_iterlog* r = b.log + (size_t)F.job_id * b.log_cap + lc;
            r->phase = phase; r->iter = iter; r->accepted = u.accepted; r->reserved0 = 0; r->new_chi2 = new_chi2;
            for (int k = 0; k < 6; ++k) r->dT[k] = dT[k];
            se3_store(u.model, r->T_after);
          }
          st->log_count = lc + 1;
        }
      }
    }
    __syncthreads();
    if (b.log && tid == 0) {   // A and b of the trace come from s_tot (written by lanes 0..26 of wave 0 above)
      const int lc = st->log_count - 1;
      if (lc >= 0 && lc < b.log_cap) {
        plsvo_poseopt_iterlog* r = b.log + (size_t)F.job_id * b.log_cap + lc;
        for (int i = 0; i < 6; ++i) for (int jj = 0; jj < 6; ++jj) r->A[i * 6 + jj] = s_tot[sym6_index(i, jj)];
        for (int k = 0; k < 6; ++k) r->b[k] = s_tot[21 + k];
      }
    }
    if (s_ctl[0]) break;
  }
}

template <int PO_T>
__global__ __launch_bounds__(PO_T) PLSVO_PO_OCC(PO_T) void pose_opt_kernel(PoseBatchDev b, double* poses) {
  PoseFrame F = popt_frame(b, b.order ? b.order[blockIdx.x] : (int)blockIdx.x);
  const PoseJobDev& job = F.job;
  PoseStateDev* st = F.st;
  const int tid = threadIdx.x;
  if (tid == 0 && b.work_key) b.work_key[F.job_id] = 0;
  const int np = job.n_pts, ns = job.n_seg, nf = np + ns;
  float* errs = F.errs;
  double* vec = F.vec;

  __shared__ __align__(16) double s_red[32 * (PO_T / 16)];
  __shared__ double s_lu[36];     // covariance: the LU factors live in LDS (dynamic pivot indexing would put them in scratch)
  __shared__ int s_perm[8];
  __shared__ double s_pose[32];
  __shared__ double s_tot[32];
  __shared__ int s_ctl[32];
  __shared__ int s_hist[PO_BINS];                           // 8 KB: radix histogram, or staging for the rank select
  __shared__ int s_sel[16];

#ifdef PLSVO_TIMING
  __shared__ unsigned long long s_time[8];
  __shared__ unsigned long long s_tlast;
  if (tid == 0) { for (int k = 0; k < 8; ++k) s_time[k] = 0; s_tlast = __builtin_amdgcn_s_memtime(); }
#endif
  if (tid == 0) {
    SE3d m = se3_load(job.T0);
    se3_store(m, s_pose + 12); se3_store(m, s_pose + 19); s_pose[26] = 0.0; s_pose[27] = 0.0; s_pose[28] = 0.0;
    for (int k = 0; k < 32; ++k) s_tot[k] = 0.0;
    popt_store_Rt<false>(m, s_pose);
    s_ctl[0] = 0; s_ctl[1] = 0; s_ctl[2] = 0;
    popt_reset_state(job, st);
  }
  for (int i = tid; i < np; i += PO_T) b.pt_keep[job.pt_off + i] = 1;
  for (int s = tid; s < ns; s += PO_T) b.seg_keep[job.seg_off + s] = 1;
  __syncthreads();
  if (nf == 0) {                                                              // errors.empty() :88-89
    if (tid == 0) { st->status = 1; if (poses) for (int k = 0; k < 7; ++k) poses[7 * F.job_id + k] = job.T0[k]; }
    return;
  }

  // ---- scale pass :57-95 ----
  if constexpr (PO_T == 64) {
    for (int f = tid; f < nf; f += PO_T) {
      double P[12];
      popt_pose_per_round(s_pose, P);
      errs[f] = popt_scale_error(b, job, f, P, vec + 3 * nf);
    }
  } else {
    double P[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = s_pose[k];
    for (int f = tid; f < nf; f += PO_T) errs[f] = popt_scale_error(b, job, f, P, vec + 3 * nf);
  }
  __syncthreads();
  PTICK(0);
  // MAD scale = 1.48f * median (float).  Zero points: the reference is undefined (:70); we define 1.0.
  auto median_f32 = [&](const float* v, int n) -> float {
    return __uint_as_float(block_radix_select<PO_T, 32, uint32_t>([&](int i) { return (uint32_t)__float_as_uint(v[i]); }, n, n / 2, s_hist, s_sel));
  };
  if (np > 0) F.scale_pt = (double)__fmul_rn(1.48f, median_f32(errs, np));
  if (ns > 0) F.scale_ls = (double)__fmul_rn(1.48f, median_f32(errs + np, ns));

  PTICK(1);
  // ---- first GN loop ----
  if (job.n_iter <= 0) for (int f = tid; f < nf; f += PO_T) vec[f] = __longlong_as_double(0x7ff0000000000000LL);
  popt_gn_loop<PO_T>(b, F, s_red, s_pose, s_tot, s_ctl, job.n_iter, 0);

  PTICK(2);
  // ---- covariance :197-199 (from the last assembled A, even if that iteration was rolled back) ----
  if (tid < 64) {   // wave 0: lane 0 factorises, lanes 0..5 each solve for one column of the inverse
    const double f2 = job.fx * job.fx;
    if (tid < 36) s_lu[tid] = s_tot[sym6_index(tid / 6, tid % 6)] * f2;
    wave_lds_fence();
    if (tid == 0) lu6_lds(s_lu, s_perm);
    wave_lds_fence();
    if (tid < 6) inv6_column_lds(s_lu, s_perm, tid, st->cov);
  }

  // ---- cull :201-242 ----
  const double thr_pt = job.reproj_thresh / job.fx;
  const double thr_ls = thr_pt * F.scale_ls / F.scale_pt;
  int del_pt = 0, del_ls = 0;
  {
    double P[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = s_pose[k];
    for (int f = tid; f < nf; f += PO_T) {
      if constexpr (PO_T == 64) popt_pose_per_round(s_pose, P);
      int deleted;
      vec[2 * nf + f] = popt_cull_feature(b, job, f, P, thr_pt, thr_ls, vec + 3 * nf, deleted);
      del_pt += deleted == 1; del_ls += deleted == 2;
      vec[nf + f] = __longlong_as_double(0x7ff0000000000000LL);  // +inf sentinel for the refinement's init entries
    }
  }
  // deleted counts -> thread 0
  {
    const int lane = tid & 63, wave = tid >> 6;
    const double a = wave_sum_to_lane63((double)del_pt), c = wave_sum_to_lane63((double)del_ls);
    __syncthreads();
    if (lane == 63) { s_red[PO_RED * wave] = a; s_red[PO_RED * wave + 1] = c; }
    __syncthreads();
  }
  for (int w = 0; w < PO_T / 64; ++w) { F.n_del_pt += (int)(s_red[PO_RED * w] + 0.5); F.n_del_ls += (int)(s_red[PO_RED * w + 1] + 0.5); }
  __syncthreads();

  // ---- refinement with inliers :469-563 (10-argument overload) ----
  int n_init = job.n_iter > 0 ? nf : 0;
  if (job.n_iter_ref >= 0) {
    popt_gn_loop<PO_T>(b, F, s_red, s_pose, s_tot, s_ctl, job.n_iter_ref, 1);
    if (job.n_iter_ref > 0) n_init += nf - F.n_del_pt - F.n_del_ls;
  }
  __syncthreads();

  PTICK(3);
  // ---- medians :244-249 ----
  auto kth_f64 = [&](const double* v, int n, int k) -> unsigned long long {
    return block_radix_select<PO_T, 64, unsigned long long>([&](int i) { return (unsigned long long)__double_as_longlong(v[i]); }, n, k, s_hist, s_sel);
  };
  unsigned long long mi = 0;
  if (n_init > 0) mi = kth_f64(vec, (job.n_iter_ref > 0) ? 2 * nf : nf, n_init / 2);   // unwritten refinement entries hold +inf and sort last
  const unsigned long long mf = kth_f64(vec + 2 * nf, nf, nf / 2);
  if (tid == 0) {
    popt_write_result(b, F, poses, s_pose, true, mi, mf, s_ctl + 1);
#ifdef PLSVO_TIMING
    { const unsigned long long t__ = __builtin_amdgcn_s_memtime(); s_time[4] += t__ - s_tlast; }
    for (int k = 0; k < 8; ++k) st->phase_ticks[k] = s_time[k];
#endif
  }
}

// ================================================================================================================================
// Large batches: ONE 16-LANE DPP ROW PER FRAME, four frames per wave (pose_opt_rows_kernel).
//
// A frame is a few hundred features and a chain of serial steps (reduce -> 6x6 solve -> SE3 update -> medians): with a whole wave per
// frame the wave-cooperative solve and the update on lane 0 issue ~1400 wave-instructions per Gauss-Newton iteration for ONE frame --
// more than the feature pass itself (five 64-lane rounds) -- and the launch is bound by VALU issue, not by memory or occupancy
// (measured: 2.0 ms per 32768 frames at 198 VGPRs, two waves per SIMD).  Here a wave carries four frames:
//   * features: lane rl of a row takes features rl, rl + 16, ... of ITS frame (18 rounds for 280 features, 97 % of the lanes busy);
//   * reduction: row_reduce_scatter32 is a butterfly INSIDE the 16-lane DPP rows -- its result is already the per-frame total, no
//     cross-row combine, no workgroup barrier anywhere in the kernel;
//   * solve + update: lane 0 of every row solves its frame's 6x6 system serially in registers (lane_solve6: Eigen's pivot order is the
//     original diagonal sorted once, so the matrix is gathered from LDS already permuted and eliminated with static indices -- nothing
//     indexed at run time, no scratch) and applies the update: four frames per instruction stream instead of one;
//   * medians: per row, from the values held in the lanes' registers (row_select_regs, poseopt_select.hpp: minimum / maximum, histogram
//     passes over a 256-bin LDS histogram per frame, rank finish); rows above its cap: radix select over memory (row_radix_select).
// Rows of a wave run in lock step: a loop runs to the largest trip count of its four frames (same feature counts in practice; the
// Gauss-Newton loops differ by an iteration or two).
// ================================================================================================================================
#define DPP_ROW_SHR_(n) (0x110 + (n))
template <int N>
__device__ __forceinline__ int row_shr_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, DPP_ROW_SHR_(N), 0xf, 0xf, true); }   // lanes without a source receive 0
// inclusive prefix sum over the 16 lanes of a row
__device__ __forceinline__ int row_scan_incl_i32(int v) {
  v += row_shr_i32<1>(v); v += row_shr_i32<2>(v); v += row_shr_i32<4>(v); v += row_shr_i32<8>(v);
  return v;
}
// sum over the 16 lanes of a row, result in every lane of the row
__device__ __forceinline__ int row_sum_i32(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, DPP_QUAD_XOR1, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, DPP_QUAD_XOR2, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_HALF_MIRROR, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, DPP_ROW_MIRROR, 0xf, 0xf, true);
  return v;
}

struct PoseRowLds {        // per frame (row) of the workgroup
  double pose[32];         // 0..8 R, 9..11 t, 12..18 model, 19..25 T_old, 26 chi2, 27 point-iterations, 28 line-iterations
  double tot[32];          // totals of the last iteration: 21 A, 6 b, chi2, #points, #segments
  double lu[36];           // covariance: LU factors
  double x[8];             // lane_solve6: un-permuted result
  int perm[8];
  int ctl[8];              // 0 break, 1 / 2 iterations of the two loops
  int sel[8];              // radix select: chosen bin, rank inside it, its count, (4,5) the surviving value
  int hist[PO_BINS];
};

// k-th smallest (0-based) of n non-negative IEEE values given as unsigned bit patterns of BITS bits, by the 16 lanes of ONE ROW; every
// row of the wave calls it together (`active`: this row takes part).  get(i) returns the pattern of element i.
template <int BITS, typename U, typename GET>
__device__ __forceinline__ U row_radix_select(GET get, int n, int k, bool active, int* hist, int* sel) {
  static_assert(PO_RADIX_BITS == 8 && BITS % 8 == 0, "16 lanes x 16 bins");
  const int rl = threadIdx.x & 15;
  U prefix = 0, mask = 0, result = 0;
  bool done = !active;
  for (int shift = BITS - 8; shift >= 0; shift -= 8) {
    if (!__any(!done)) break;
#pragma unroll
    for (int j = 0; j < 16; j += 4) *reinterpret_cast<uint4*>(hist + rl * 16 + j) = make_uint4(0u, 0u, 0u, 0u);
    wave_lds_fence();
    if (!done) for (int i = rl; i < n; i += 16) {
      const U v = get(i);
      if ((v & mask) == prefix) atomicAdd(&hist[(int)((v >> shift) & (U)255)], 1);
    }
    wave_lds_fence();
    int loc[16], local = 0;
#pragma unroll
    for (int j = 0; j < 16; j += 4) {
      const uint4 h4 = *reinterpret_cast<const uint4*>(hist + rl * 16 + j);
      loc[j] = (int)h4.x; loc[j + 1] = (int)h4.y; loc[j + 2] = (int)h4.z; loc[j + 3] = (int)h4.w;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) local += loc[j];
    int cum = row_scan_incl_i32(local) - local;
    if (!done) {
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (k >= cum && k < cum + loc[j]) { sel[0] = rl * 16 + j; sel[1] = k - cum; sel[2] = loc[j]; }
        cum += loc[j];
      }
    }
    wave_lds_fence();
    bool single = false;
    if (!done) {
      prefix |= ((U)(unsigned)sel[0]) << shift;
      mask |= ((U)255) << shift;
      k = sel[1];
      single = sel[2] == 1 && shift > 0;   // one candidate left: it is the answer, the remaining digits need no histogram
      if (single) for (int i = rl; i < n; i += 16) {
        const U v = get(i);
        if ((v & mask) == prefix) { sel[4] = (int)(unsigned)(v & (U)0xffffffffu); sel[5] = (int)(unsigned)((unsigned long long)v >> 32); }
      }
    }
    wave_lds_fence();
    if (single) { result = (U)(((unsigned long long)(unsigned)sel[5] << 32) | (unsigned long long)(unsigned)sel[4]); done = true; }
    wave_lds_fence();   // sel is rewritten by the next pass
  }
  return done ? result : prefix;
}

// ---- the row select from registers (poseopt_select.hpp: what it is for, the paths) -----------------------------------------------------
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_mov_bits(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true); }
template <int CTRL>
__device__ __forceinline__ unsigned long long dpp_mov_bits(unsigned long long v) {
  const uint32_t lo = dpp_mov_bits<CTRL>((uint32_t)v), hi = dpp_mov_bits<CTRL>((uint32_t)(v >> 32));
  return ((unsigned long long)hi << 32) | (unsigned long long)lo;
}
// minimum / maximum / bitwise OR over the 16 lanes of a row, result in every lane of the row
template <typename U>
__device__ __forceinline__ void row_min_max_bits(U& mn, U& mx) {
  U a, c;
  a = dpp_mov_bits<DPP_QUAD_XOR1>(mn); c = dpp_mov_bits<DPP_QUAD_XOR1>(mx); mn = a < mn ? a : mn; mx = c > mx ? c : mx;
  a = dpp_mov_bits<DPP_QUAD_XOR2>(mn); c = dpp_mov_bits<DPP_QUAD_XOR2>(mx); mn = a < mn ? a : mn; mx = c > mx ? c : mx;
  a = dpp_mov_bits<DPP_ROW_HALF_MIRROR>(mn); c = dpp_mov_bits<DPP_ROW_HALF_MIRROR>(mx); mn = a < mn ? a : mn; mx = c > mx ? c : mx;
  a = dpp_mov_bits<DPP_ROW_MIRROR>(mn); c = dpp_mov_bits<DPP_ROW_MIRROR>(mx); mn = a < mn ? a : mn; mx = c > mx ? c : mx;
}
template <typename U>
__device__ __forceinline__ U row_or_bits(U v) {
  v |= dpp_mov_bits<DPP_QUAD_XOR1>(v); v |= dpp_mov_bits<DPP_QUAD_XOR2>(v);
  v |= dpp_mov_bits<DPP_ROW_HALF_MIRROR>(v); v |= dpp_mov_bits<DPP_ROW_MIRROR>(v);
  return v;
}
__device__ __forceinline__ uint32_t po_bits(float x) { return (uint32_t)__float_as_uint(x); }
__device__ __forceinline__ unsigned long long po_bits(double x) { return (unsigned long long)__double_as_longlong(x); }
__device__ __forceinline__ uint32_t po_bits(uint32_t x) { return x; }
__device__ __forceinline__ unsigned long long po_bits(unsigned long long x) { return x; }

// k-th smallest (0-based) of n <= kRowSelectCap unsigned patterns of BITS bits by the 16 lanes of ONE ROW, the values in registers: lane rl
// holds elements rl, rl + 16, ... in v[0], v[1], ... (entries at or past n are never looked at).  Every row of the wave calls it
// together.  `hist`: the row's 256 histogram words (the first 32 double as the candidates' staging).  `path`: kRowSelect* bits.
template <int BITS, typename U>
__device__ __forceinline__ U row_select_regs(const U (&v)[kRowSelectChunks], int n, int k, bool active, int* hist, int& path) {
  static_assert(PO_RADIX_BITS == 8 && kRowSelectCap < 1024, "16 lanes x 16 bins; bin, count and rank share one word");
  const int rl = threadIdx.x & 15;
  constexpr U ONES = ~(U)0;
  U mn = ONES, mx = 0;
#pragma unroll
  for (int c = 0; c < kRowSelectChunks; ++c) if (rl + 16 * c < n) { mn = v[c] < mn ? v[c] : mn; mx = v[c] > mx ? v[c] : mx; }
  row_min_max_bits(mn, mx);
  U result = 0;
  bool done = !active;
  path = 0;
  if (active && mn == mx) { result = mn; done = true; path = kRowSelectEqual; }   // (identical values: also n == 1)
  // the bits above the highest bit in which minimum and maximum differ are common to every value: the first digit starts there
  const U diff = mn ^ mx;
  const int hb = diff ? 63 - __builtin_clzll((unsigned long long)diff) : 0;
  U mask = hb + 1 >= BITS ? (U)0 : (U)(ONES << (hb + 1));
  U prefix = mn & mask;
  int shift = hb >= 7 ? hb - 7 : 0;
  int passes = 0, cnt = 0;
  while (__any(!done)) {
#pragma unroll
    for (int j = 0; j < 16; j += 4) *reinterpret_cast<uint4*>(hist + rl * 16 + j) = make_uint4(0u, 0u, 0u, 0u);
    wave_lds_fence();
    if (!done) {
#pragma unroll
      for (int c = 0; c < kRowSelectChunks; ++c)
        if (rl + 16 * c < n && (v[c] & mask) == prefix) atomicAdd(&hist[(int)(((v[c] & ~mask) >> shift) & (U)255)], 1);
    }
    wave_lds_fence();
    int loc[16], local = 0;
#pragma unroll
    for (int j = 0; j < 16; j += 4) {
      const uint4 h4 = *reinterpret_cast<const uint4*>(hist + rl * 16 + j);
      loc[j] = (int)h4.x; loc[j + 1] = (int)h4.y; loc[j + 2] = (int)h4.z; loc[j + 3] = (int)h4.w;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) local += loc[j];
    int cum = row_scan_incl_i32(local) - local;
    int pack = 0;   // the lane that owns the bin of rank k: bin << 20 | its count << 10 | the rank inside it
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (!done && k >= cum && k < cum + loc[j]) pack = ((rl * 16 + j) << 20) | (loc[j] << 10) | (k - cum);
      cum += loc[j];
    }
    pack = row_sum_i32(pack);
    bool rank = false;
    if (!done) {
      ++passes;
      prefix |= (U)(unsigned)(pack >> 20) << shift;
      mask |= (U)255 << shift;
      cnt = (pack >> 10) & 1023; k = pack & 1023;
      if (shift == 0) { result = prefix; done = true; path = kRowSelectDigits | (passes > 1 ? kRowSelectExtraPass : 0); }   // every bit is decided
      else if (cnt <= 16) rank = true;
      else shift = shift >= 8 ? shift - 8 : 0;   // (heavy duplicates, or a crowded bin: another digit)
    }
    if (__any(rank)) {
      // at most 16 values are left: one per lane through LDS, every lane counts how many are below / not above its own, and the lane
      // with less <= k < leq holds the answer (equal values: several lanes, the same pattern)
      // (the candidates are staged in the row's first histogram words, which the rest of the pass reads and writes as int / uint4: what
      //  orders the two views is the wave_lds_fence() in front of the bin reads above, the one between these stores and the reads of
      //  cand[], and the one behind them, ahead of the next pass's zeroing -- keep all three when editing)
      U* const cand = reinterpret_cast<U*>(hist);
      int mine = 0;
#pragma unroll
      for (int c = 0; c < kRowSelectChunks; ++c) mine += (rank && rl + 16 * c < n && (v[c] & mask) == prefix) ? 1 : 0;
      int off = row_scan_incl_i32(mine) - mine;
      if (rank) {
#pragma unroll
        for (int c = 0; c < kRowSelectChunks; ++c) if (rl + 16 * c < n && (v[c] & mask) == prefix) cand[off++] = v[c];
      }
      wave_lds_fence();
      const bool holds = rank && rl < cnt;
      const U me = holds ? cand[rl] : ONES;
      int less = 0, leq = 0;
      if (rank) {
#pragma unroll
        for (int j = 0; j < 16; ++j) if (j < cnt) { const U o = cand[j]; less += o < me ? 1 : 0; leq += o <= me ? 1 : 0; }
      }
      const U r = row_or_bits((holds && less <= k && k < leq) ? me : (U)0);
      if (rank) { result = r; done = true; path = kRowSelectRank | (passes > 1 ? kRowSelectExtraPass : 0); }
      wave_lds_fence();   // the histogram words are zeroed again by the next pass
    }
  }
  return result;
}

// The select of the row kernels' four call sites: p[0..n) are the row's values (float / double / their patterns).  use_regs (wave-uniform)
// and no active row of the wave above the cap: every lane fetches its values ONCE, all loads issued before the first wait, and
// row_select_regs finishes from registers; otherwise the whole wave takes row_radix_select (rows share a program counter).
template <int BITS, typename U, typename T>
__device__ __forceinline__ U row_select(const T* p, int n, int k, bool active, bool use_regs, int* hist, int* sel, int& path) {
  if (use_regs && !__any(active && n > kRowSelectCap)) {
    const int rl = threadIdx.x & 15;
    U v[kRowSelectChunks];
#pragma unroll
    for (int c = 0; c < kRowSelectChunks; ++c) { v[c] = ~(U)0; if (active && rl + 16 * c < n) v[c] = po_bits(p[rl + 16 * c]); }
    return row_select_regs<BITS, U>(v, n, k, active, hist, path);
  }
  path = active ? kRowSelectFallback : 0;
  return row_radix_select<BITS, U>([&](int i) { return (U)po_bits(p[i]); }, n, k, active, hist, sel);
}

// H x = rhs for a symmetric 6x6 H by ONE LANE: the arithmetic of wave_solve6_core (Gauss-Jordan in the pivot order of Eigen's LDLT, the
// zero-pivot rule selected by `flavour`, NaN / Inf propagation -- see there) with the system held in this lane's registers.  Eigen's
// order is the original |diagonal| sorted once (selection sort with Eigen's own transpositions: first maximum wins, numbers beat NaN),
// so the 27 inputs are gathered from LDS already permuted and every index below is a compile-time constant.  Columns already
// eliminated are dead (they never reach x) and are not updated.  tot: 21 A (upper, row-major) + 6 b in LDS; xs: 6 doubles of LDS.
__device__ __forceinline__ void lane_solve6(const double* tot, double* xs, double* x, int flavour) {
  double key[6]; int idx[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) { key[i] = fabs(tot[sym6_index(i, i)]); idx[i] = i; }
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    double bk = key[k]; int bi = idx[k], bp = k;
#pragma unroll
    for (int j = k + 1; j < 6; ++j) {
      const bool better = key[j] > bk || (bk != bk && key[j] == key[j]);
      if (better) { bk = key[j]; bi = idx[j]; bp = j; }
    }
    const double ok_ = key[k]; const int oi = idx[k];
#pragma unroll
    for (int j = k + 1; j < 6; ++j) if (bp == j) { key[j] = ok_; idx[j] = oi; }
    key[k] = bk; idx[k] = bi;
  }
  double M[6][6], r[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) {
#pragma unroll
    for (int c = 0; c < 6; ++c) M[a][c] = tot[sym6_index(idx[a], idx[c])];
    r[a] = tot[21 + idx[a]];
  }
  unsigned zero_piv = 0u;
  const double cutoff = flavour == 330 ? 0.0 : fabs(2.220446049250313e-16 * key[0]);
#pragma unroll
  for (int p = 0; p < 6; ++p) {
    const double piv = M[p][p];
    // Eigen 3.2: stop at "biggest_in_corner < cutoff"; no scaling unless |pivot| > cutoff; D^+ drops |d| <= max|D| eps
    if (!(key[p] < cutoff) && fabs(piv) > cutoff) {
      const double rinv = fast_rcp(piv);
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        if (i == p) continue;
        const double f = M[i][p];
#pragma unroll
        for (int j = p + 1; j < 6; ++j) M[i][j] = fma(-(f * M[p][j]), rinv, M[i][j]);
        r[i] = fma(-(f * r[p]), rinv, r[i]);
      }
    } else {
      zero_piv |= 1u << p;
    }
  }
  const double tolerance = 1.0 / 1.7976931348623157e308;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const double dgi = M[a][a], m = r[a];
    double xi = (((zero_piv >> a) & 1u) || !(fabs(dgi) > tolerance)) ? ((dgi != dgi || m != m) ? (m + dgi) : 0.0) : m / dgi;
    if (cutoff > 1.7976931348623157e308) xi = (a == 5 || fabs(dgi) <= 1.7976931348623157e308) ? 0.0 : __builtin_nan("");   // infinite diagonal: see wave_solve6_core
    xs[idx[a]] = xi;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");   // same lane: LDS keeps program order
#pragma unroll
  for (int c = 0; c < 6; ++c) x[c] = xs[c];
}

// ---- the phases of a row's frame: begin, Gauss-Newton step, finish.  pose_opt_rows_kernel and the three refill kernels below are
// compositions of them; what differs between the kernels is an argument here, never a second copy. ---------------------------------------

// the frame of this lane's row: launch slot 4 * workgroup + row, taken through b.order where `ordered`; a row past the batch holds the
// batch's last frame with `valid` false
__device__ __forceinline__ PoseFrame rows_frame(const PoseBatchDev& b, bool ordered) {
  const int slot = blockIdx.x * 4 + ((threadIdx.x & 63) >> 4);
  const bool valid = slot < b.n_jobs;
  PoseFrame F = popt_frame(b, valid ? ((ordered && b.order) ? b.order[slot] : slot) : b.n_jobs - 1);
  F.valid = valid;
  return F;
}

// begin: state reset, the empty-frame result, keep flags, scale pass :57-95, the two MAD scales, the +inf fill of a frame without
// iterations.  to_carry: the row's pose block goes to a PoseRefillCarry next, which is copied whole (words 29..31 are cleared) and gets
// a zero tot of its own; otherwise the Gauss-Newton loop follows in this launch (L.tot and L.ctl are cleared)
__device__ __forceinline__ void rows_begin(const PoseBatchDev& b, PoseFrame& F, PoseRowLds& L, double* poses, int select, bool to_carry) {
  const int rl = threadIdx.x & 15;
  const PoseJobDev& job = F.job;
  PoseStateDev* st = F.st;
  const int np = job.n_pts, ns = job.n_seg, nf = np + ns;
  float* errs = F.errs;
  double* vec = F.vec;
  if (F.valid && rl == 0) {
    SE3d m = se3_load(job.T0);
    se3_store(m, L.pose + 12); se3_store(m, L.pose + 19); L.pose[26] = 0.0; L.pose[27] = 0.0; L.pose[28] = 0.0;
    if (to_carry) { L.pose[29] = 0.0; L.pose[30] = 0.0; L.pose[31] = 0.0; }
    else for (int k = 0; k < 32; ++k) L.tot[k] = 0.0;
    popt_store_Rt<true>(m, L.pose);
    if (!to_carry) { L.ctl[0] = 0; L.ctl[1] = 0; L.ctl[2] = 0; }
    popt_reset_state(job, st);
    for (int k = 0; k < 8; ++k) st->phase_ticks[k] = 0;
    if (nf == 0) { st->status = 1; if (poses) for (int k = 0; k < 7; ++k) poses[7 * F.job_id + k] = job.T0[k]; }   // errors.empty() :88-89
    if (b.work_key) b.work_key[F.job_id] = 0;
  }
  const bool row_on = F.valid && nf > 0;
  if (row_on) {
    for (int i = rl; i < np; i += 16) b.pt_keep[job.pt_off + i] = 1;
    for (int s = rl; s < ns; s += 16) b.seg_keep[job.seg_off + s] = 1;
  }
  wave_lds_fence();

  if (row_on) {
    double P[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = L.pose[k];
    for (int f = rl; f < nf; f += 16) errs[f] = popt_scale_error(b, job, f, P, vec + 3 * nf);
  }
  wave_lds_fence();   // (global scratch written and read by lanes of this wave only)
  // MAD scale = 1.48f * median (float).  Zero points: the reference is undefined (:70); we define 1.0.
  {
    int path;
    const uint32_t m_pt = row_select<32, uint32_t>(errs, np, np / 2, row_on && np > 0, select != 0, L.hist, L.sel, path);
    const uint32_t m_ls = row_select<32, uint32_t>(errs + np, ns, ns / 2, row_on && ns > 0, select != 0, L.hist, L.sel, path);
    if (np > 0) F.scale_pt = (double)__fmul_rn(1.48f, __uint_as_float(m_pt));
    if (ns > 0) F.scale_ls = (double)__fmul_rn(1.48f, __uint_as_float(m_ls));
  }
  if (row_on && job.n_iter <= 0) for (int f = rl; f < nf; f += 16) vec[f] = __longlong_as_double(0x7ff0000000000000LL);
}

// one Gauss-Newton iteration (:103-195 / :469-563) of the rows that are `running`: iteration `iter` of `n_iter` of the row's own frame,
// phase 0 the first loop, 1 the refinement.  Afterwards L.ctl[0] says whether the row's loop has stopped.  TRACE: the iteration trace
// (b.log) is compiled in
template <bool TRACE>
__device__ __forceinline__ void rows_gn_step(const PoseBatchDev& b, const PoseFrame& F, PoseRowLds& L, bool running, int iter, int n_iter, int phase) {
  const int lane = threadIdx.x & 63, rl = lane & 15;
  const PoseJobDev& job = F.job;
  const int nf = job.n_pts + job.n_seg;
  double acc[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) acc[k] = 0.0;
  if (running) {
    double P[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = L.pose[k];
    for (int f = rl; f < nf; f += 16) popt_accumulate_feature(b, job, f, P, F.scale_pt, F.scale_ls, iter == 0, F.vec + phase * nf, F.vec + 3 * nf, acc);
  }
  double out2[2];
  row_reduce_scatter32(acc, out2);     // every lane of the wave takes part (DPP); the row's totals are the frame's
  if (running) *reinterpret_cast<double2*>(L.tot + row_reduce_scatter32_index(lane)) = make_double2(out2[0], out2[1]);
  wave_lds_fence();
  if (running && rl == 0) {
    double dT[6];
    lane_solve6(L.tot, L.x, dT, job.ldlt_flavour);                          // A.ldlt().solve(b) :170
    const double new_chi2 = L.tot[27];
    L.pose[27] += L.tot[28]; L.pose[28] += L.tot[29];
    L.ctl[1 + phase] += 1;
    const PoseUpdate u = popt_update_model<true>(L.pose, dT, new_chi2, iter);
    L.ctl[0] = iter + 1 >= n_iter ? 1 : u.brk;
    if constexpr (TRACE) if (b.log) {
      PoseStateDev* st = F.st;
      const int lc = st->log_count;
      if (lc < b.log_cap) {
        plsvo_poseopt_iterlog* r = b.log + (size_t)F.job_id * b.log_cap + lc;
        r->phase = phase; r->iter = iter; r->accepted = u.accepted; r->reserved0 = 0; r->new_chi2 = new_chi2;
        for (int k = 0; k < 6; ++k) r->dT[k] = dT[k];
        se3_store(u.model, r->T_after);
        for (int i = 0; i < 6; ++i) for (int jj = 0; jj < 6; ++jj) r->A[i * 6 + jj] = L.tot[sym6_index(i, jj)];
        for (int k = 0; k < 6; ++k) r->b[k] = L.tot[21 + k];
      }
      st->log_count = lc + 1;
    }
  }
  wave_lds_fence();
}

// one GN loop for the four frames of the wave, in lock step until the last of them stops
__device__ __forceinline__ void rows_gn_loop(const PoseBatchDev& b, const PoseFrame& F, PoseRowLds& L, bool row_on, int n_iter, int phase) {
  bool running = row_on && n_iter > 0;
  for (int iter = 0; __any(running); ++iter) {
    rows_gn_step<true>(b, F, L, running, iter, n_iter, phase);
    if (running && L.ctl[0]) running = false;
  }
}

// finish, first part: covariance :197-199 (from the last assembled A, even if that iteration was rolled back) and cull :201-242
__device__ __forceinline__ void rows_finish_cull(const PoseBatchDev& b, PoseFrame& F, PoseRowLds& L) {
  const int rl = threadIdx.x & 15;
  const PoseJobDev& job = F.job;
  const int nf = job.n_pts + job.n_seg;
  double* vec = F.vec;
  const bool row_on = F.valid && nf > 0;
  if (row_on) {
    const double f2 = job.fx * job.fx;
    for (int t = rl; t < 36; t += 16) L.lu[t] = L.tot[sym6_index(t / 6, t % 6)] * f2;
  }
  wave_lds_fence();
  if (row_on && rl == 0) lu6_lds(L.lu, L.perm);
  wave_lds_fence();
  if (row_on && rl < 6) inv6_column_lds(L.lu, L.perm, rl, F.st->cov);

  const double thr_pt = job.reproj_thresh / job.fx;
  const double thr_ls = thr_pt * F.scale_ls / F.scale_pt;
  int del_pt = 0, del_ls = 0;
  if (row_on) {
    double P[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = L.pose[k];
    for (int f = rl; f < nf; f += 16) {
      int deleted;
      vec[2 * nf + f] = popt_cull_feature(b, job, f, P, thr_pt, thr_ls, vec + 3 * nf, deleted);
      del_pt += deleted == 1; del_ls += deleted == 2;
      vec[nf + f] = __longlong_as_double(0x7ff0000000000000LL);  // +inf sentinel for the refinement's init entries
    }
  }
  F.n_del_pt = row_sum_i32(del_pt); F.n_del_ls = row_sum_i32(del_ls);
  wave_lds_fence();   // keep flags and vec visible to the row
}

// finish, second part: the two f64 medians :244-249 and the final write.  n_iter_ref: the refinement loop's bound where one ran in this
// launch -- its init entries then join the first median -- and 0 where none can have (the refill).  iters: see popt_write_result
__device__ __forceinline__ void rows_finish_write(const PoseBatchDev& b, const PoseFrame& F, PoseRowLds& L, double* poses, int select, int n_iter_ref, const int* iters) {
  const int rl = threadIdx.x & 15;
  const int nf = F.job.n_pts + F.job.n_seg;
  double* vec = F.vec;
  const bool row_on = F.valid && nf > 0;
  int n_init = F.job.n_iter > 0 ? nf : 0;
  if (n_iter_ref > 0) n_init += nf - F.n_del_pt - F.n_del_ls;
  int path;
  const unsigned long long mi = row_select<64, unsigned long long>(vec, (n_iter_ref > 0) ? 2 * nf : nf, n_init / 2, row_on && n_init > 0, select != 0, L.hist, L.sel, path);   // unwritten refinement entries hold +inf and sort last
  const unsigned long long mf = row_select<64, unsigned long long>(vec + 2 * nf, nf, nf / 2, row_on, select != 0, L.hist, L.sel, path);
  if (row_on && rl == 0) popt_write_result(b, F, poses, L.pose, n_init > 0, mi, mf, iters);
}

__device__ __forceinline__ void rows_finish(const PoseBatchDev& b, PoseFrame& F, PoseRowLds& L, double* poses, int select, int n_iter_ref, const int* iters) {
  rows_finish_cull(b, F, L);
  rows_finish_write(b, F, L, poses, select, n_iter_ref, iters);
}

// a re-run staged batch comes sorted by the feature-iterations of its last launch (plsvo_capi.hip::plsvo_poseopt_run): the four frames of a
// wave run in lock step until the LAST of them stops, and the iteration counts are bimodal (4-6, or all 10) -- in an arbitrary order three
// waves of four hold a ten-iteration frame and run ten; sorted, the rows of a wave stop together
__global__ __launch_bounds__(64) PLSVO_PO_ROWS_OCC void pose_opt_rows_kernel(PoseBatchDev b, double* poses, int select) {
  __shared__ __align__(16) PoseRowLds s_rows[4];
  PoseRowLds& L = s_rows[(threadIdx.x & 63) >> 4];
  PoseFrame F = rows_frame(b, true);
  const int nf = F.job.n_pts + F.job.n_seg;
  const bool row_on = F.valid && nf > 0;
  rows_begin(b, F, L, poses, select, false);
  rows_gn_loop(b, F, L, row_on, F.job.n_iter, 0);
  rows_finish_cull(b, F, L);
  // refinement with inliers :469-563 (10-argument overload)
  rows_gn_loop(b, F, L, row_on && F.job.n_iter_ref >= 0, F.job.n_iter_ref, 1);
  wave_lds_fence();
  rows_finish_write(b, F, L, poses, select, F.job.n_iter_ref, L.ctl + 1);
}

// ================================================================================================================================
// The row shape as THREE launches: rows of the Gauss-Newton loop are refilled from a queue of frames.
//
// The four frames of a pose_opt_rows_kernel wave iterate until the LAST of them stops, and iteration counts are bimodal (4-6, or all
// ten): in an arbitrary launch order almost every wave runs ten.  Rows share a program counter, so a row cannot start its next frame's
// scale pass while its neighbours iterate -- the kernel is therefore cut at the loop's borders:
//   * pose_refill_prologue_kernel: rows_begin, four frames per wave in lock step (uniform work, so in index order), then the carry;
//   * pose_refill_gn_kernel: persistent.  A row without a running frame takes the next launch slot from one device counter, loads that
//     frame's carry (PoseRefillCarry) into its PoseRowLds and joins rows_gn_step at ITS iteration 0; when the frame stops the row
//     writes the carry back.  A row either gets a slot or is done: nothing polls, nothing waits for another workgroup;
//   * pose_refill_epilogue_kernel: the carry, then rows_finish, four frames per wave in lock step.
// The phases are the functions pose_opt_rows_kernel is made of, so per frame the arithmetic, the sums and their order are the same
// and every output is bit-identical.  Batches with a refinement loop (n_iter_ref > 0), an iteration trace or a -DPLSVO_TIMING build
// keep pose_opt_rows_kernel (plsvo_capi.hip decides).
// ================================================================================================================================
__global__ __launch_bounds__(64) PLSVO_PO_ROWS_OCC void pose_refill_prologue_kernel(PoseBatchDev b, PoseRefillDev q, double* poses, int select) {
  __shared__ __align__(16) PoseRowLds s_rows[4];
  const int rl = threadIdx.x & 15;
  PoseRowLds& L = s_rows[(threadIdx.x & 63) >> 4];
  PoseFrame F = rows_frame(b, false);
  rows_begin(b, F, L, poses, select, true);
  if (F.valid) {
    PoseRefillCarry& c = q.carry[F.job_id];
    *reinterpret_cast<double2*>(c.pose + 2 * rl) = *reinterpret_cast<const double2*>(L.pose + 2 * rl);
    *reinterpret_cast<double2*>(c.tot + 2 * rl) = make_double2(0.0, 0.0);
    if (rl == 0) { c.scale_pt = F.scale_pt; c.scale_ls = F.scale_ls; c.iters = 0; }
  }
}

__global__ __launch_bounds__(64) PLSVO_PO_ROWS_OCC void pose_refill_gn_kernel(PoseBatchDev b, PoseRefillDev q) {
  __shared__ __align__(16) PoseRowLds s_rows[4];
  const int rl = threadIdx.x & 15;
  PoseRowLds& L = s_rows[(threadIdx.x & 63) >> 4];
  // per row, in plain lane registers: the frame (what of its job the feature pass reads) and its iteration index
  PoseFrame F;
  PoseJobDev& job = F.job;
  job.n_pts = 0; job.n_seg = 0; job.pt_off = 0; job.seg_off = 0; job.n_iter = 0; job.ldlt_flavour = 320;
  F.job_id = 0; F.scale_pt = 1.0; F.scale_ls = 1.0; F.vec = b.scratch_f64;
  int iter = 0;
  bool running = false, want = true;
  for (;;) {
    // ---- refill: a row without a frame takes the next launch slot; frames without iterations to run are passed over ----
    while (__any(want)) {
      if (want && rl == 0) L.sel[6] = atomicAdd(q.next, 1);
      wave_lds_fence();
      if (want) {
        const int slot = L.sel[6];
        if (slot >= b.n_jobs) {
          want = false;
        } else {
          F.job_id = b.order ? b.order[slot] : slot;
          const PoseJobDev* J = b.jobs + F.job_id;
          job.n_pts = J->n_pts; job.n_seg = J->n_seg; job.pt_off = J->pt_off; job.seg_off = J->seg_off; job.n_iter = J->n_iter; job.ldlt_flavour = J->ldlt_flavour;
          if (job.n_pts + job.n_seg > 0 && job.n_iter > 0) {
            const PoseRefillCarry& c = q.carry[F.job_id];
            *reinterpret_cast<double2*>(L.pose + 2 * rl) = *reinterpret_cast<const double2*>(c.pose + 2 * rl);
            if (rl == 0) { L.ctl[0] = 0; L.ctl[1] = 0; }
            F.scale_pt = c.scale_pt; F.scale_ls = c.scale_ls;
            F.vec = b.scratch_f64 + 5 * ((size_t)job.pt_off + (size_t)job.seg_off);
            iter = 0; running = true; want = false;
          }
        }
      }
      wave_lds_fence();
    }
    if (!__any(running)) break;

    rows_gn_step<false>(b, F, L, running, iter, job.n_iter, 0);
    if (running) {
      ++iter;
      if (L.ctl[0]) {   // the frame has stopped: its carry goes back, the row is free
        PoseRefillCarry& c = q.carry[F.job_id];
        *reinterpret_cast<double2*>(c.pose + 2 * rl) = *reinterpret_cast<const double2*>(L.pose + 2 * rl);
        *reinterpret_cast<double2*>(c.tot + 2 * rl) = *reinterpret_cast<const double2*>(L.tot + 2 * rl);
        if (rl == 0) c.iters = L.ctl[1];
        running = false; want = true;
      }
    }
  }
}

__global__ __launch_bounds__(64) PLSVO_PO_ROWS_OCC void pose_refill_epilogue_kernel(PoseBatchDev b, PoseRefillDev q, double* poses, int select) {
  __shared__ __align__(16) PoseRowLds s_rows[4];
  const int rl = threadIdx.x & 15;
  PoseRowLds& L = s_rows[(threadIdx.x & 63) >> 4];
  PoseFrame F = rows_frame(b, false);
  const PoseRefillCarry& c = q.carry[F.job_id];
  *reinterpret_cast<double2*>(L.pose + 2 * rl) = *reinterpret_cast<const double2*>(c.pose + 2 * rl);
  *reinterpret_cast<double2*>(L.tot + 2 * rl) = *reinterpret_cast<const double2*>(c.tot + 2 * rl);
  F.scale_pt = c.scale_pt; F.scale_ls = c.scale_ls;
  const int iters[2] = { c.iters, 0 };   // (no batch with a refinement loop comes here)
  wave_lds_fence();
  rows_finish(b, F, L, poses, select, 0, iters);
}

bool pose_opt_refill_built() {
#ifdef PLSVO_TIMING
  return false;
#else
  return true;
#endif
}

hipError_t launch_pose_opt_refill(const PoseBatchDev& b, const PoseRefillDev& q, double* d_poses, int gn_grid, int select, hipStream_t stream) {
  const int wgs = (b.n_jobs + 3) / 4;
  if (gn_grid < 1 || gn_grid > wgs) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pose_refill_prologue_kernel, dim3(wgs), dim3(64), 0, stream, b, q, d_poses, select);
  hipLaunchKernelGGL(pose_refill_gn_kernel, dim3(gn_grid), dim3(64), 0, stream, b, q);
  hipLaunchKernelGGL(pose_refill_epilogue_kernel, dim3(wgs), dim3(64), 0, stream, b, q, d_poses, select);
  return hipGetLastError();
}

// plsvo_poseopt_row_select (tests): row_select -- the function of the three row kernels above -- on rows of patterns, four rows per workgroup
struct RowSelectLds { int hist[PO_BINS]; int sel[8]; };
template <int BITS, typename U>
__global__ __launch_bounds__(64) void pose_row_select_kernel(RowSelectDev t) {
  __shared__ __align__(16) RowSelectLds s_rows[4];
  const int lane = threadIdx.x & 63, rl = lane & 15;
  const int row_raw = blockIdx.x * 4 + (lane >> 4);
  const bool valid = row_raw < t.n_rows;
  const int row = valid ? row_raw : t.n_rows - 1;
  const int n = t.row_n[row];
  RowSelectLds& L = s_rows[lane >> 4];
  int path;
  const U r = row_select<BITS, U>(reinterpret_cast<const U*>(t.patterns) + t.row_off[row], n, t.row_k[row], valid && t.row_active[row] != 0 && n > 0,
                                  t.select != 0, L.hist, L.sel, path);
  if (valid && rl == 0) { reinterpret_cast<U*>(t.selected)[row] = r; t.path[row] = path; }
}

hipError_t launch_pose_row_select(const RowSelectDev& t, hipStream_t stream) {
  if (t.n_rows < 1) return hipErrorInvalidValue;
  const dim3 grid((t.n_rows + 3) / 4);
  if (t.bits == 32) hipLaunchKernelGGL((pose_row_select_kernel<32, uint32_t>), grid, dim3(64), 0, stream, t);
  else if (t.bits == 64) hipLaunchKernelGGL((pose_row_select_kernel<64, unsigned long long>), grid, dim3(64), 0, stream, t);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_pose_opt(const PoseBatchDev& b, double* d_poses, int threads, int select, hipStream_t stream) {
  switch (threads) {
    case 16: hipLaunchKernelGGL(pose_opt_rows_kernel, dim3((b.n_jobs + 3) / 4), dim3(64), 0, stream, b, d_poses, select); break;   // a 16-lane row per frame
    case 64: hipLaunchKernelGGL((pose_opt_kernel<64>), dim3(b.n_jobs), dim3(64), 0, stream, b, d_poses); break;
    case 256: hipLaunchKernelGGL((pose_opt_kernel<256>), dim3(b.n_jobs), dim3(256), 0, stream, b, d_poses); break;
    case 512: hipLaunchKernelGGL((pose_opt_kernel<512>), dim3(b.n_jobs), dim3(512), 0, stream, b, d_poses); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace plsvo_hip
