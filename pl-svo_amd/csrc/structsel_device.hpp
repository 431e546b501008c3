// structsel_device.hpp -- FrameHandlerBase::optimizeStructure (src/frame_handler_base.cpp:192-237, called at src/frame_handler_mono.cpp:340)
// on the resident map tables on gfx950: one WAVE per stream, four waves per workgroup, no LDS, nothing synchronised across waves; an
// inactive stream returns at once.  Included by seeds_kernels.hip (compiled with -ffp-contract=off: positions are bit-identical to
// structopt_kernel's on the gathered job and to tests/np_structsel.py).
//
//   collect   the new frame's features whose keep byte is set (feat3D != NULL behind the pose optimiser's cull), points and segments; a
//             segment that won both of its cells is a feature twice and is in the reference's deque twice
//   select    the min(max_n, count) entries with the smallest last_structure_optim_ (signed).  std::nth_element leaves open which of
//             several equal keys at the cut are taken -- PINNED: ties go to the earlier feature.  No sort: the key of rank max_n is found by
//             a wave-minimum walk over the distinct keys (at most max_n of them are visited), every entry below it is taken and the
//             remainder is filled with the first entries AT it, in feature order (ballot + popcount prefix carried across rounds of 64).
//             The selected entries are listed in feature order
//   optimise  one lane per selected entry, points and segments in the same rounds of 64: Point::optimize / LineSeg::optimize of
//             structopt_device.hpp on kf_T and the landmark's observation list, the position written in place, the key set to the frame id
//             (also when the optimiser rolled back, :221).  A landmark listed twice is run twice IN SEQUENCE by the lane of its first
//             entry -- the second run starts from the first's result with fresh chi2 -- and the lane of its second entry stands by.
#pragma once
#include <hip/hip_runtime.h>

#include "select_device.hpp"
#include "structopt_device.hpp"

namespace plsvo_hip {

#pragma clang fp contract(off)

constexpr int kStsWaves = kSelWaves;

// last_structure_optim_ as an unsigned key of the same order (signed 32-bit compare)
__device__ __forceinline__ kf_u64 sts_key(const int* last_optim, int lm) { return (kf_u64)((unsigned int)last_optim[lm] ^ 0x80000000u); }

// One kind's choice: the landmarks of the chosen entries into r_lm (at most max_n rows), in feature order.  Returns their number.
__device__ __forceinline__ int sts_select(const int* f_lm, const uint8_t* keep, int n_feat, const int* last_optim, int max_n, int* r_lm) {
  const int lane = threadIdx.x & 63;
  const kf_u64 below = ((kf_u64)1 << lane) - 1;
  int count = 0;
  for (int base = 0; base < n_feat; base += 64) {
    const int i = base + lane;
    count += __popcll(__ballot(i < n_feat && keep[i] != 0));
  }
  const int n_take = count < max_n ? count : max_n;
  if (n_take <= 0) return 0;                         // (wave-uniform)
  kf_u64 thr = kKfOnes;                              // every entry is taken: each key is below it
  int tie_take = 0;
  if (count > max_n) {
    kf_u64 prev = 0;
    bool first = true;
    int cum = 0;
    for (;;) {
      kf_u64 m = kKfOnes;                            // the smallest key above the last one
      for (int base = 0; base < n_feat; base += 64) {
        const int i = base + lane;
        if (i < n_feat && keep[i] != 0) {
          const kf_u64 u = sts_key(last_optim, f_lm[i]);
          if ((first || u > prev) && u < m) m = u;
        }
      }
      m = kf_wave_min(m);
      if (m == kKfOnes) break;                       // (cannot happen while cum < count: the walk ends at the latest with the largest key)
      int cnt = 0;
      for (int base = 0; base < n_feat; base += 64) {
        const int i = base + lane;
        cnt += __popcll(__ballot(i < n_feat && keep[i] != 0 && sts_key(last_optim, f_lm[i]) == m));
      }
      if (cum + cnt >= n_take) { thr = m; tie_take = n_take - cum; break; }
      cum += cnt; prev = m; first = false;
    }
  }
  int n_sel = 0, tie_seen = 0;
  for (int base = 0; base < n_feat; base += 64) {
    const int i = base + lane;
    int lm = -1;
    bool lt = false, tie = false;
    if (i < n_feat && keep[i] != 0) {
      lm = f_lm[i];
      const kf_u64 u = sts_key(last_optim, lm);
      lt = u < thr; tie = u == thr;
    }
    const kf_u64 tmask = __ballot(tie);
    const bool take = lt || (tie && tie_seen + __popcll(tmask & below) < tie_take);
    const kf_u64 smask = __ballot(take);
    const int slot = n_sel + __popcll(smask & below);
    if (take && slot < n_take) r_lm[slot] = lm;      // (slot < n_take always: the rows of the report are never overrun)
    n_sel += __popcll(smask); tie_seen += __popcll(tmask);
  }
  return n_sel < n_take ? n_sel : n_take;
}

// Entry k of one kind's list, by its own lane: every run of its landmark, in sequence, unless an earlier entry holds the same landmark
template <bool SEG>
__device__ __forceinline__ void sts_optimize_entry(const StructSelBatchDev& b, const CandMapDev& M, int job, int k, int n_sel, int frame_id) {
  const CandBatchDev& c = b.s.c;
  const size_t row0 = (size_t)job * (size_t)(SEG ? b.max_n_segs : b.max_n_pts);
  const int* r_lm = (SEG ? b.r_seg_lm : b.r_pt_lm) + row0;
  int* r_iters = (SEG ? b.r_seg_iters : b.r_pt_iters) + row0;
  const int lm = r_lm[k];
  for (int j = 0; j < k; ++j) if (r_lm[j] == lm) return;
  const double* kf_T = c.kf_T + 7 * M.kf_off;
  if (SEG) {
    const int* obs_off = c.seg_obs_off + M.seg_off + M.stream;
    const int o0 = obs_off[lm], o1 = obs_off[lm + 1];
    double* S = const_cast<double*>(c.seg_spos) + 3 * (M.seg_off + lm); double* E = const_cast<double*>(c.seg_epos) + 3 * (M.seg_off + lm);
    double sp[3] = { S[0], S[1], S[2] }, ep[3] = { E[0], E[1], E[2] };
    for (int j = k; j < n_sel; ++j) {
      if (r_lm[j] != lm) continue;
      r_iters[j] = segment_optimize(kf_T, c.seg_obs_kf + M.segobs_off, c.seg_obs_sf + 3 * M.segobs_off, c.seg_obs_ef + 3 * M.segobs_off, o0, o1, b.n_iter_segs, sp, ep);
#pragma unroll
      for (int d = 0; d < 3; ++d) { b.r_seg_spos[3 * (row0 + j) + d] = sp[d]; b.r_seg_epos[3 * (row0 + j) + d] = ep[d]; }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) { S[d] = sp[d]; E[d] = ep[d]; }
    b.seg_last_optim[M.seg_off + lm] = frame_id;
  } else {
    const int* obs_off = c.pt_obs_off + M.pt_off + M.stream;
    const int o0 = obs_off[lm], o1 = obs_off[lm + 1];
    double* P = const_cast<double*>(c.pt_pos) + 3 * (M.pt_off + lm);
    double pos[3] = { P[0], P[1], P[2] };
    for (int j = k; j < n_sel; ++j) {
      if (r_lm[j] != lm) continue;
      r_iters[j] = point_optimize(kf_T, c.pt_obs_kf + M.ptobs_off, c.pt_obs_f + 3 * M.ptobs_off, o0, o1, b.n_iter_pts, pos);
#pragma unroll
      for (int d = 0; d < 3; ++d) b.r_pt_pos[3 * (row0 + j) + d] = pos[d];
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) P[d] = pos[d];
    b.pt_last_optim[M.pt_off + lm] = frame_id;
  }
}

__global__ __launch_bounds__(64 * kStsWaves) void map_optimize_structure_kernel(const StructSelBatchDev b) {
  const int lane = threadIdx.x & 63;
  const int job = blockIdx.x * kStsWaves + (int)(threadIdx.x >> 6);
  if (job >= b.s.c.n_jobs) return;                  // whole waves leave: nothing below synchronises across waves
  const StructSelJobDev& J = b.jobs[job];
  if (!J.active) {
    if (lane == 0) { b.r_counts[2 * job] = 0; b.r_counts[2 * job + 1] = 0; }
    return;
  }
  const CandMapDev& M = b.s.c.maps[job];
  // -- collect and select: both kinds' keys are read before any is written
  const int n_sel_pt = sts_select(b.s.f_pt_lm + M.opt_off, J.pt_keep + M.opt_off, b.s.scalars[3 * job], b.pt_last_optim + M.pt_off, b.max_n_pts,
                                  b.r_pt_lm + (size_t)job * (size_t)b.max_n_pts);
  const int n_sel_seg = sts_select(b.s.f_seg_lm + 2 * M.oseg_off, J.seg_keep + 2 * M.oseg_off, b.s.scalars[3 * job + 1], b.seg_last_optim + M.seg_off, b.max_n_segs,
                                   b.r_seg_lm + (size_t)job * (size_t)b.max_n_segs);
  if (lane == 0) { b.r_counts[2 * job] = n_sel_pt; b.r_counts[2 * job + 1] = n_sel_seg; }
  cand_wave_sync();                                 // the lists, read back by other lanes
  // -- optimise: one lane per entry, the points' entries first
  const int total = n_sel_pt + n_sel_seg;
  for (int base = 0; base < total; base += 64) {
    const int k = base + lane;
    if (k < n_sel_pt) sts_optimize_entry<false>(b, M, job, k, n_sel_pt, J.frame_id);
    else if (k < total) sts_optimize_entry<true>(b, M, job, k - n_sel_pt, n_sel_seg, J.frame_id);
  }
}

}  // namespace plsvo_hip
