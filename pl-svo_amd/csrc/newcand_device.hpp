// newcand_device.hpp -- converged depth-filter seeds become candidate landmarks of the resident map tables on gfx950: one WAVE per
// stream, four waves per workgroup, no LDS, no atomics, nothing synchronised across waves; a stream without new landmarks returns at
// once.  Included by seeds_kernels.hip like the other map kernels (the kernel copies, it computes nothing).
//
//   map_add_candidates_kernel
//     `new Point(xyz_world, ftr)` / `new LineSeg(xyz_world_s, xyz_world_e, ftr)`     src/depth_filter.cpp:334-355, :439-462
//     the constructors: obs_.push_front(ftr), both reprojection counters 0           src/point.cpp:41-55, :198-212
//     newCandidatePoint / newCandidateSegment: TYPE_CANDIDATE, push_back             src/map.cpp:285-290, :377-382
//
// All of it is an append behind the used part of rows that were laid out by capacity (plsvo_candidates_reserve_landmarks for the
// landmark rows and the candidate lists, plsvo_candidates_reserve for the observation entries): per kind, in rounds of 64, lane j writes
// landmark n_lm + j -- position(s), type, zeroed counters, the event byte, the end of its one-entry observation list, the observation,
// its entry at the back of the candidate list.  The candidate count is read from the stream's record ON THE DEVICE: the selection and the
// insertion shorten the list there.  No lane reads what another lane writes, so the wave needs no barrier; one lane stores the new counts
// last.  The host has checked the room against its mirrors before the launch; nothing here can refuse.
#pragma once
#include <hip/hip_runtime.h>

#include "insert_device.hpp"

namespace plsvo_hip {

constexpr int kNewWaves = kInsWaves;
constexpr uint8_t kNewCand = 64;                    // event bit: a landmark appended since the last selection (reported as PLSVO_LM_EVENT_NEW)

__device__ __forceinline__ void new_copy2(double* dst, const double* src) {          // 16-byte rows: one vector load, one vector store
  *reinterpret_cast<double2*>(dst) = *reinterpret_cast<const double2*>(src);
}
__device__ __forceinline__ void new_copy3(double* dst, const double* src) {
#pragma unroll
  for (int d = 0; d < 3; ++d) dst[d] = src[d];
}

__global__ __launch_bounds__(64 * kNewWaves) void map_add_candidates_kernel(const NewCandBatchDev b) {
  const CandBatchDev& c = b.c;
  const int lane = threadIdx.x & 63;
  const int job = blockIdx.x * kNewWaves + (int)(threadIdx.x >> 6);
  if (job >= c.n_jobs) return;                      // whole waves leave: nothing below synchronises across waves
  const NewCandJobDev J = b.jobs[job];
  if (J.n_pt + J.n_seg == 0) return;
  CandMapDev& M = const_cast<CandMapDev&>(c.maps[job]);
  const int n_pt = M.n_pt, n_seg = M.n_seg, n_ptc = M.n_pt_cand, n_segc = M.n_seg_cand;
  const long long stream = M.stream;

  // -- points
  if (J.n_pt > 0) {
    int* const obs_off = const_cast<int*>(c.pt_obs_off) + M.pt_off + stream;
    const int old_end = obs_off[n_pt];
    for (int base = 0; base < J.n_pt; base += 64) {
      const int j = base + lane;
      if (j >= J.n_pt) continue;
      const long long src = J.pt_at + j, lm = M.pt_off + n_pt + j, ob = M.ptobs_off + old_end + j;
      new_copy3(const_cast<double*>(c.pt_pos) + 3 * lm, b.pt_pos + 3 * src);
      const_cast<int*>(c.pt_type)[lm] = PLSVO_LM_CANDIDATE;
      b.pt_nfail[lm] = 0; b.pt_nsucc[lm] = 0; b.pt_event[lm] = kNewCand;
      obs_off[n_pt + j + 1] = old_end + j + 1;
      const_cast<int*>(c.pt_obs_kf)[ob] = b.pt_obs_kf[src];
      new_copy2(const_cast<double*>(c.pt_obs_px) + 2 * ob, b.pt_obs_px + 2 * src);
      new_copy3(const_cast<double*>(c.pt_obs_f) + 3 * ob, b.pt_obs_f + 3 * src);
      const_cast<int*>(c.pt_obs_level)[ob] = b.pt_obs_level[src];
      const_cast<uint8_t*>(c.pt_obs_type)[ob] = b.pt_obs_type[src];
      new_copy2(const_cast<double*>(c.pt_obs_grad) + 2 * ob, b.pt_obs_grad + 2 * src);
      const_cast<int*>(c.pt_cand)[M.ptc_off + n_ptc + j] = n_pt + j;
    }
  }

  // -- segments
  if (J.n_seg > 0) {
    int* const obs_off = const_cast<int*>(c.seg_obs_off) + M.seg_off + stream;
    const int old_end = obs_off[n_seg];
    for (int base = 0; base < J.n_seg; base += 64) {
      const int j = base + lane;
      if (j >= J.n_seg) continue;
      const long long src = J.seg_at + j, lm = M.seg_off + n_seg + j, ob = M.segobs_off + old_end + j;
      new_copy3(const_cast<double*>(c.seg_spos) + 3 * lm, b.seg_spos + 3 * src);
      new_copy3(const_cast<double*>(c.seg_epos) + 3 * lm, b.seg_epos + 3 * src);
      const_cast<int*>(c.seg_type)[lm] = PLSVO_LM_CANDIDATE;
      b.seg_nfail[lm] = 0; b.seg_nsucc[lm] = 0; b.seg_event[lm] = kNewCand;
      obs_off[n_seg + j + 1] = old_end + j + 1;
      const_cast<int*>(c.seg_obs_kf)[ob] = b.seg_obs_kf[src];
      new_copy2(const_cast<double*>(c.seg_obs_spx) + 2 * ob, b.seg_obs_spx + 2 * src);
      new_copy2(const_cast<double*>(c.seg_obs_epx) + 2 * ob, b.seg_obs_epx + 2 * src);
      new_copy3(const_cast<double*>(c.seg_obs_sf) + 3 * ob, b.seg_obs_sf + 3 * src);
      new_copy3(const_cast<double*>(c.seg_obs_ef) + 3 * ob, b.seg_obs_ef + 3 * src);
      const_cast<int*>(c.seg_obs_level)[ob] = b.seg_obs_level[src];
      const_cast<int*>(c.seg_cand)[M.segc_off + n_segc + j] = n_seg + j;
    }
  }

  // -- the stream's record, last: every lane has read the old counts above
  if (lane == 0) {
    M.n_pt = n_pt + J.n_pt; M.n_seg = n_seg + J.n_seg; M.n_pt_cand = n_ptc + J.n_pt; M.n_seg_cand = n_segc + J.n_seg;
  }
}

}  // namespace plsvo_hip
