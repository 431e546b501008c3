// seedlist_device.hpp -- the depth filter's seed lists as resident tables on gfx950.  Included by seeds_kernels.hip like
// the other map kernels; update_seeds_resident_kernel, which shares the per-seed bodies of update_seeds_kernel, sits beside it there.
//
//   seeds_commit_kernel      what DepthFilter::updatePointSeeds / updateLineSeeds do with a seed after its body ran
//                            (src/depth_filter.cpp:289-292 age, :334-360 / :439-467 converged and NaN seeds erased, the converged ones
//                            handed to newCandidatePoint / newCandidateSegment, src/map.cpp:285-290, :377-382)
//   seeds_keyframe_kernel    DepthFilter::initializeSeeds (:177-191) and removeKeyframe (:199-216)
//   seeds_occupancy_kernel, seeds_start_kernel    initializeSeeds' creating half (:151-191) from the detector's cell keys (below)
//
// One WAVE per stream, four per workgroup, no LDS, no atomics, nothing synchronised across waves.  A list is compacted in place, stably,
// in rounds of 64 rows: every lane loads its row (and its shadow row) into registers, a ballot gives it its rank among the rows that
// stay, and it stores the row at that rank.  The destination never lies above the source and everything at or below the current round is
// already in registers, so no row is overwritten before it was read (within a round a store of one array waits for the round's load of
// the same array: it stores what that load returned).  A converged row is written as map_add_candidates_kernel writes a landmark, at its
// rank among the converged rows.  One lane stores the counts last.
#pragma once
#include <hip/hip_runtime.h>

#include "newcand_device.hpp"

namespace plsvo_hip {

constexpr int kSeedWaves = kNewWaves;
constexpr int kSeedAged = 5;                        // PLSVO_SEED_AGED

__device__ __forceinline__ int seed_rank(unsigned long long mask, int lane) {   // set bits below this lane
  return __popcll(mask & ((1ull << lane) - 1ull));
}
// a 16-byte row between global memory and registers
__device__ __forceinline__ void seed_ld2(double* d, const double* g) { const double2 v = *reinterpret_cast<const double2*>(g); d[0] = v.x; d[1] = v.y; }
__device__ __forceinline__ void seed_st2(double* g, const double* d) { *reinterpret_cast<double2*>(g) = make_double2(d[0], d[1]); }

struct PtSeedRow { int ref_kf, batch_id, level; uint8_t type; double px[2], f[3], grad[2]; float a, b, mu, z_range, sigma2; };
struct SegSeedRow { int ref_kf, batch_id, level; double px[2], f[3], sf[3], ef[3], spx[2], epx[2]; float a, b, mu_s, mu_e, z_range_s, z_range_e, sigma2_s, sigma2_e; };

template <typename T> __device__ __forceinline__ T* seed_mut(const T* p) { return const_cast<T*>(p); }

__device__ __forceinline__ PtSeedRow pt_seed_load(const SeedListBatchDev& b, long long r) {
  const SeedsBatchDev& s = b.s;
  PtSeedRow R;
  R.ref_kf = s.pt_ref_frame[r]; R.batch_id = b.pt_batch_id[r]; R.level = s.pt_level[r]; R.type = s.pt_type[r];
  seed_ld2(R.px, s.pt_px + 2 * r); new_copy3(R.f, s.pt_f + 3 * r); seed_ld2(R.grad, s.pt_grad + 2 * r);
  R.a = s.pt_a[r]; R.b = s.pt_b[r]; R.mu = s.pt_mu[r]; R.z_range = s.pt_z_range[r]; R.sigma2 = s.pt_sigma2[r];
  return R;
}
__device__ __forceinline__ void pt_seed_store(const SeedListBatchDev& b, long long r, const PtSeedRow& R) {
  const SeedsBatchDev& s = b.s;
  seed_mut(s.pt_ref_frame)[r] = R.ref_kf; b.pt_batch_id[r] = R.batch_id; seed_mut(s.pt_level)[r] = R.level; seed_mut(s.pt_type)[r] = R.type;
  seed_st2(seed_mut(s.pt_px) + 2 * r, R.px); new_copy3(seed_mut(s.pt_f) + 3 * r, R.f); seed_st2(seed_mut(s.pt_grad) + 2 * r, R.grad);
  seed_mut(s.pt_a)[r] = R.a; seed_mut(s.pt_b)[r] = R.b; seed_mut(s.pt_mu)[r] = R.mu; seed_mut(s.pt_z_range)[r] = R.z_range; seed_mut(s.pt_sigma2)[r] = R.sigma2;
}
__device__ __forceinline__ SegSeedRow seg_seed_load(const SeedListBatchDev& b, long long r) {
  const SeedsBatchDev& s = b.s;
  SegSeedRow R;
  R.ref_kf = s.seg_ref_frame[r]; R.batch_id = b.seg_batch_id[r]; R.level = s.seg_level[r];
  seed_ld2(R.px, s.seg_px + 2 * r); new_copy3(R.f, s.seg_f + 3 * r); new_copy3(R.sf, s.seg_sf + 3 * r); new_copy3(R.ef, s.seg_ef + 3 * r);
  seed_ld2(R.spx, b.seg_spx + 2 * r); seed_ld2(R.epx, b.seg_epx + 2 * r);
  R.a = s.seg_a[r]; R.b = s.seg_b[r]; R.mu_s = s.seg_mu_s[r]; R.mu_e = s.seg_mu_e[r]; R.z_range_s = s.seg_z_range_s[r]; R.z_range_e = s.seg_z_range_e[r];
  R.sigma2_s = s.seg_sigma2_s[r]; R.sigma2_e = s.seg_sigma2_e[r];
  return R;
}
__device__ __forceinline__ void seg_seed_store(const SeedListBatchDev& b, long long r, const SegSeedRow& R) {
  const SeedsBatchDev& s = b.s;
  seed_mut(s.seg_ref_frame)[r] = R.ref_kf; b.seg_batch_id[r] = R.batch_id; seed_mut(s.seg_level)[r] = R.level;
  seed_st2(seed_mut(s.seg_px) + 2 * r, R.px); new_copy3(seed_mut(s.seg_f) + 3 * r, R.f); new_copy3(seed_mut(s.seg_sf) + 3 * r, R.sf);
  new_copy3(seed_mut(s.seg_ef) + 3 * r, R.ef); seed_st2(b.seg_spx + 2 * r, R.spx); seed_st2(b.seg_epx + 2 * r, R.epx);
  seed_mut(s.seg_a)[r] = R.a; seed_mut(s.seg_b)[r] = R.b; seed_mut(s.seg_mu_s)[r] = R.mu_s; seed_mut(s.seg_mu_e)[r] = R.mu_e;
  seed_mut(s.seg_z_range_s)[r] = R.z_range_s; seed_mut(s.seg_z_range_e)[r] = R.z_range_e; seed_mut(s.seg_sigma2_s)[r] = R.sigma2_s; seed_mut(s.seg_sigma2_e)[r] = R.sigma2_e;
}

__device__ __forceinline__ bool seed_stays(int status) { return status == PLSVO_SEED_NOT_VISIBLE || status == PLSVO_SEED_NO_MATCH || status == PLSVO_SEED_UPDATED; }

// rows of each status among the n live rows from `status` (ballot and popcount over rounds of 64)
__device__ __forceinline__ void seed_count(const int* status, int n, int lane, int* cnt) {
#pragma unroll
  for (int k = 0; k < 6; ++k) cnt[k] = 0;
  for (int base = 0; base < n; base += 64) {
    const int st = base + lane < n ? status[base + lane] : -1;
#pragma unroll
    for (int k = 0; k < 6; ++k) cnt[k] += __popcll(__ballot(st == k));
  }
}

__global__ __launch_bounds__(64 * kSeedWaves) void seeds_commit_kernel(const SeedListBatchDev b) {
  const CandBatchDev& c = b.m.c;
  const SeedsBatchDev& s = b.s;
  const int lane = threadIdx.x & 63;
  const int job = blockIdx.x * kSeedWaves + (int)(threadIdx.x >> 6);
  if (job >= b.n_jobs) return;                      // whole waves leave: nothing below synchronises across waves
  SeedStreamDev& S = b.streams[job];
  CandMapDev& M = const_cast<CandMapDev&>(c.maps[job]);
  const int n_sp = S.n_pt, n_ss = S.n_seg;
  const int n_pt = M.n_pt, n_seg = M.n_seg, n_ptc = M.n_pt_cand, n_segc = M.n_seg_cand;
  const long long stream = M.stream;
  int* const pt_obs_off = const_cast<int*>(c.pt_obs_off) + M.pt_off + stream;
  int* const seg_obs_off = const_cast<int*>(c.seg_obs_off) + M.seg_off + stream;
  const int pt_end = pt_obs_off[n_pt], seg_end = seg_obs_off[n_seg];
  SeedReportDev R;
#pragma unroll
  for (int k = 0; k < 6; ++k) { R.pt[k] = 0; R.seg[k] = 0; }
  R.first_pt = -1; R.first_seg = -1; R.n_pt_seeds = n_sp; R.n_seg_seeds = n_ss; R.n_pt = n_pt; R.n_seg = n_seg; R.n_pt_cand = n_ptc; R.n_seg_cand = n_segc;
  R.n_pt_obs = pt_end; R.n_seg_obs = seg_end; R.no_room = 0; R.batch_counter = S.batch_counter;
  if (!b.frames[job].active) { if (lane == 0) b.report[job] = R; return; }
  seed_count(s.o_pt_status + S.pt_off, n_sp, lane, R.pt);
  seed_count(s.o_seg_status + S.seg_off, n_ss, lane, R.seg);
  const int cp = R.pt[PLSVO_SEED_CONVERGED], cs = R.seg[PLSVO_SEED_CONVERGED];
  // -- room for ALL of them or nothing: landmark rows, observation entries, the candidate lists
  if (n_pt + cp > S.rows_pt || n_seg + cs > S.rows_seg || pt_end + cp > S.cap_pt_obs || seg_end + cs > S.cap_seg_obs || n_ptc + cp > S.rows_pt_cand ||
      n_segc + cs > S.rows_seg_cand) {
    R.no_room = 1;
    if (lane == 0) b.report[job] = R;
    return;
  }

  // -- points
  int kept = 0, conv = 0;
  for (int base = 0; base < n_sp; base += 64) {
    const int j = base + lane;
    const long long r = S.pt_off + j;
    int st = -1;
    PtSeedRow Q;
    if (j < n_sp) {
      Q = pt_seed_load(b, r);
      st = s.o_pt_status[r];
      Q.a = s.o_pt_a[r]; Q.b = s.o_pt_b[r]; Q.mu = s.o_pt_mu[r]; Q.sigma2 = s.o_pt_sigma2[r];
    }
    const bool is_conv = st == PLSVO_SEED_CONVERGED, stays = seed_stays(st);
    const unsigned long long mc = __ballot(is_conv), mk = __ballot(stays);
    if (is_conv) {
      const int k = conv + seed_rank(mc, lane);
      const long long lm = M.pt_off + n_pt + k, ob = M.ptobs_off + pt_end + k;
      new_copy3(const_cast<double*>(c.pt_pos) + 3 * lm, s.o_pt_xyz + 3 * r);
      const_cast<int*>(c.pt_type)[lm] = PLSVO_LM_CANDIDATE;
      b.m.pt_nfail[lm] = 0; b.m.pt_nsucc[lm] = 0; b.m.pt_event[lm] = kNewCand;
      pt_obs_off[n_pt + k + 1] = pt_end + k + 1;
      const_cast<int*>(c.pt_obs_kf)[ob] = Q.ref_kf;
      seed_st2(const_cast<double*>(c.pt_obs_px) + 2 * ob, Q.px);
      new_copy3(const_cast<double*>(c.pt_obs_f) + 3 * ob, Q.f);
      const_cast<int*>(c.pt_obs_level)[ob] = Q.level;
      const_cast<uint8_t*>(c.pt_obs_type)[ob] = Q.type;
      seed_st2(const_cast<double*>(c.pt_obs_grad) + 2 * ob, Q.grad);
      const_cast<int*>(c.pt_cand)[M.ptc_off + n_ptc + k] = n_pt + k;
    }
    if (stays) pt_seed_store(b, S.pt_off + kept + seed_rank(mk, lane), Q);
    conv += __popcll(mc); kept += __popcll(mk);
  }
  const int kept_pt = kept;

  // -- segments
  kept = 0; conv = 0;
  for (int base = 0; base < n_ss; base += 64) {
    const int j = base + lane;
    const long long r = S.seg_off + j;
    int st = -1;
    SegSeedRow Q;
    if (j < n_ss) {
      Q = seg_seed_load(b, r);
      st = s.o_seg_status[r];
      Q.a = s.o_seg_a[r]; Q.b = s.o_seg_b[r]; Q.mu_s = s.o_seg_mu_s[r]; Q.mu_e = s.o_seg_mu_e[r]; Q.sigma2_s = s.o_seg_sigma2_s[r]; Q.sigma2_e = s.o_seg_sigma2_e[r];
    }
    const bool is_conv = st == PLSVO_SEED_CONVERGED, stays = seed_stays(st);
    const unsigned long long mc = __ballot(is_conv), mk = __ballot(stays);
    if (is_conv) {
      const int k = conv + seed_rank(mc, lane);
      const long long lm = M.seg_off + n_seg + k, ob = M.segobs_off + seg_end + k;
      new_copy3(const_cast<double*>(c.seg_spos) + 3 * lm, s.o_seg_xyz_s + 3 * r);
      new_copy3(const_cast<double*>(c.seg_epos) + 3 * lm, s.o_seg_xyz_e + 3 * r);
      const_cast<int*>(c.seg_type)[lm] = PLSVO_LM_CANDIDATE;
      b.m.seg_nfail[lm] = 0; b.m.seg_nsucc[lm] = 0; b.m.seg_event[lm] = kNewCand;
      seg_obs_off[n_seg + k + 1] = seg_end + k + 1;
      const_cast<int*>(c.seg_obs_kf)[ob] = Q.ref_kf;
      seed_st2(const_cast<double*>(c.seg_obs_spx) + 2 * ob, Q.spx);
      seed_st2(const_cast<double*>(c.seg_obs_epx) + 2 * ob, Q.epx);
      new_copy3(const_cast<double*>(c.seg_obs_sf) + 3 * ob, Q.sf);
      new_copy3(const_cast<double*>(c.seg_obs_ef) + 3 * ob, Q.ef);
      const_cast<int*>(c.seg_obs_level)[ob] = Q.level;
      const_cast<int*>(c.seg_cand)[M.segc_off + n_segc + k] = n_seg + k;
    }
    if (stays) seg_seed_store(b, S.seg_off + kept + seed_rank(mk, lane), Q);
    conv += __popcll(mc); kept += __popcll(mk);
  }

  // -- the counts and the report, last: every lane has read the old counts above
  if (lane == 0) {
    S.n_pt = kept_pt; S.n_seg = kept;
    M.n_pt = n_pt + cp; M.n_seg = n_seg + cs; M.n_pt_cand = n_ptc + cp; M.n_seg_cand = n_segc + cs;
    R.first_pt = cp ? n_pt : -1; R.first_seg = cs ? n_seg : -1; R.n_pt_seeds = kept_pt; R.n_seg_seeds = kept;
    R.n_pt = n_pt + cp; R.n_seg = n_seg + cs; R.n_pt_cand = n_ptc + cp; R.n_seg_cand = n_segc + cs; R.n_pt_obs = pt_end + cp; R.n_seg_obs = seg_end + cs;
    b.report[job] = R;
  }
}

// removeKeyframe (:199-216) on one stream's lists, by its wave: the removed keyframe's seeds go, later keyframes move down one row in the
// table.  n_sp / n_ss: the live rows, in and out
__device__ __forceinline__ void seed_remove_keyframe(const SeedListBatchDev& b, const SeedStreamDev& S, int removed_kf, int lane, int& n_sp, int& n_ss) {
  int kept = 0;
  for (int base = 0; base < n_sp; base += 64) {
    const int j = base + lane;
    PtSeedRow Q; Q.ref_kf = removed_kf;
    if (j < n_sp) Q = pt_seed_load(b, S.pt_off + j);
    const bool stays = j < n_sp && Q.ref_kf != removed_kf;
    const unsigned long long mk = __ballot(stays);
    if (Q.ref_kf > removed_kf) --Q.ref_kf;
    if (stays) pt_seed_store(b, S.pt_off + kept + seed_rank(mk, lane), Q);
    kept += __popcll(mk);
  }
  n_sp = kept; kept = 0;
  for (int base = 0; base < n_ss; base += 64) {
    const int j = base + lane;
    SegSeedRow Q; Q.ref_kf = removed_kf;
    if (j < n_ss) Q = seg_seed_load(b, S.seg_off + j);
    const bool stays = j < n_ss && Q.ref_kf != removed_kf;
    const unsigned long long mk = __ballot(stays);
    if (Q.ref_kf > removed_kf) --Q.ref_kf;
    if (stays) seg_seed_store(b, S.seg_off + kept + seed_rank(mk, lane), Q);
    kept += __popcll(mk);
  }
  n_ss = kept;
}

// initializeSeeds' line seeds (:187-190): n uploaded segments from row `at` of the k_seg_* arrays, behind the n_ss live rows
__device__ __forceinline__ void seed_append_segments(const SeedListBatchDev& b, const SeedStreamDev& S, int lane, int n_ss, int n, long long at, int new_kf, int counter,
                                                     float mu, float z_range, float sigma2) {
  const SeedsBatchDev& s = b.s;
  for (int base = 0; base < n; base += 64) {
    const int j = base + lane;
    if (j >= n) continue;
    const long long src = at + j, r = S.seg_off + n_ss + j;
    seed_mut(s.seg_ref_frame)[r] = new_kf; b.seg_batch_id[r] = counter; seed_mut(s.seg_level)[r] = b.k_seg_level[src];
    new_copy2(seed_mut(s.seg_px) + 2 * r, b.k_seg_px + 2 * src); new_copy3(seed_mut(s.seg_f) + 3 * r, b.k_seg_f + 3 * src);
    new_copy3(seed_mut(s.seg_sf) + 3 * r, b.k_seg_sf + 3 * src); new_copy3(seed_mut(s.seg_ef) + 3 * r, b.k_seg_ef + 3 * src);
    new_copy2(b.seg_spx + 2 * r, b.k_seg_spx + 2 * src); new_copy2(b.seg_epx + 2 * r, b.k_seg_epx + 2 * src);
    seed_mut(s.seg_a)[r] = 10.0f; seed_mut(s.seg_b)[r] = 10.0f; seed_mut(s.seg_mu_s)[r] = mu; seed_mut(s.seg_mu_e)[r] = mu;
    seed_mut(s.seg_z_range_s)[r] = z_range; seed_mut(s.seg_z_range_e)[r] = z_range; seed_mut(s.seg_sigma2_s)[r] = sigma2; seed_mut(s.seg_sigma2_e)[r] = sigma2;
  }
}

__global__ __launch_bounds__(64 * kSeedWaves) void seeds_keyframe_kernel(const SeedListBatchDev b) {
  const int lane = threadIdx.x & 63;
  const int job = blockIdx.x * kSeedWaves + (int)(threadIdx.x >> 6);
  if (job >= b.n_jobs) return;
  const SeedKfJobDev J = b.kf_jobs[job];
  if (J.removed_kf < 0 && !J.new_batch && J.n_pt + J.n_seg == 0) return;
  SeedStreamDev& S = b.streams[job];
  int n_sp = S.n_pt, n_ss = S.n_seg;
  const int counter = S.batch_counter + (J.new_batch ? 1 : 0);
  const SeedsBatchDev& s = b.s;

  if (J.removed_kf >= 0) seed_remove_keyframe(b, S, J.removed_kf, lane, n_sp, n_ss);

  // -- initializeSeeds: the new seeds behind the live rows, in the uploaded order (the host has checked the room)
  for (int base = 0; base < J.n_pt; base += 64) {
    const int j = base + lane;
    if (j >= J.n_pt) continue;
    const long long src = J.pt_at + j, r = S.pt_off + n_sp + j;
    seed_mut(s.pt_ref_frame)[r] = J.new_kf; b.pt_batch_id[r] = counter; seed_mut(s.pt_level)[r] = b.k_pt_level[src]; seed_mut(s.pt_type)[r] = b.k_pt_type[src];
    new_copy2(seed_mut(s.pt_px) + 2 * r, b.k_pt_px + 2 * src); new_copy3(seed_mut(s.pt_f) + 3 * r, b.k_pt_f + 3 * src);
    new_copy2(seed_mut(s.pt_grad) + 2 * r, b.k_pt_grad + 2 * src);
    seed_mut(s.pt_a)[r] = 10.0f; seed_mut(s.pt_b)[r] = 10.0f; seed_mut(s.pt_mu)[r] = J.mu; seed_mut(s.pt_z_range)[r] = J.z_range; seed_mut(s.pt_sigma2)[r] = J.sigma2;
  }
  seed_append_segments(b, S, lane, n_ss, J.n_seg, J.seg_at, J.new_kf, counter, J.mu, J.z_range, J.sigma2);
  if (lane == 0) { S.n_pt = n_sp + J.n_pt; S.n_seg = n_ss + J.n_seg; S.batch_counter = counter; }
}

// ---- a keyframe's point seeds from its FAST corners: DepthFilter::initializeSeeds' first half (:151-191) ----
//   seeds_occupancy_kernel   the detector's grid of every active stream: the caller's bytes, FastDetector::setExistingFeatures of the
//                            features the last selection wrote (:161), setGridOccpuancy of the last update's matches (:327-331); and
//                            the detection's slot table entry, from the stream's resident frame_slot row
//   seeds_start_kernel       removeKeyframe, then one PointSeed per cell key the detection left (src/feature_detection.cpp:95-101 and
//                            PointFeat's constructor, src/depth_filter.cpp:184-186), then the uploaded line seeds; re-arms the keys
// One wave per ACTIVE stream in both.  The occupancy rows are zeroed by a memset ahead of the launch: the kernel only ever stores a 1,
// so lanes that mark the same cell store the same byte and no order among them matters.

// the cell of a level-0 position, plsvo_detect_cell's rule; -1 for a position that is not finite, negative or outside the image (pin)
__device__ __forceinline__ int seed_cell_of(const SeedStartBatchDev& b, double px, double py) {
  if (!(px >= 0.0 && px < (double)b.width && py >= 0.0 && py < (double)b.height)) return -1;   // (a NaN fails every comparison)
  return (int)(py / (double)b.cell) * b.cols + (int)(px / (double)b.cell);
}

__global__ __launch_bounds__(64 * kSeedWaves) void seeds_occupancy_kernel(const SeedStartBatchDev b) {
  const int lane = threadIdx.x & 63;
  const int pos = blockIdx.x * kSeedWaves + (int)(threadIdx.x >> 6);
  if (pos >= b.n_act) return;
  const SeedStartJobDev J = b.jobs[pos];
  const SeedStreamDev& S = b.l.streams[J.stream];
  const CandMapDev& M = b.l.m.c.maps[J.stream];
  uint8_t* const occ = b.occ + (size_t)pos * (size_t)b.n_cells;
  if (J.d_occ)
    for (int i = lane; i < b.n_cells; i += 64) if (J.d_occ[i]) occ[i] = 1;
  if (J.occ_sources & PLSVO_SEED_OCC_SELECTED) {
    const int n = b.scalars[3 * J.stream];
    for (int i = lane; i < n; i += 64) {
      const long long o = M.opt_off + i;
      const int k = seed_cell_of(b, b.f_pt_px[2 * o], b.f_pt_px[2 * o + 1]);
      if (k >= 0) occ[k] = 1;
    }
  }
  if (J.occ_sources & PLSVO_SEED_OCC_UPDATED)
    for (int i = lane; i < J.n_upd_rows; i += 64) {
      const long long r = S.pt_off + i;
      const int st = b.l.s.o_pt_status[r];
      if (st != PLSVO_SEED_UPDATED && st != PLSVO_SEED_CONVERGED && st != PLSVO_SEED_NAN) continue;
      const int k = seed_cell_of(b, b.l.s.o_pt_px[2 * r], b.l.s.o_pt_px[2 * r + 1]);
      if (k >= 0) occ[k] = 1;
    }
  if (lane == 0) b.slots[pos] = b.l.m.c.frame_slot[M.f_off + J.new_kf];
}

__global__ __launch_bounds__(64 * kSeedWaves) void seeds_start_kernel(const SeedStartBatchDev b) {
  const int lane = threadIdx.x & 63;
  const int pos = blockIdx.x * kSeedWaves + (int)(threadIdx.x >> 6);
  if (pos >= b.n_act) return;
  const SeedStartJobDev J = b.jobs[pos];
  const SeedListBatchDev& l = b.l;
  const SeedsBatchDev& s = l.s;
  SeedStreamDev& S = l.streams[J.stream];
  int n_sp = S.n_pt, n_ss = S.n_seg;
  const int counter = S.batch_counter + (J.new_batch ? 1 : 0);

  // -- 1. removeKeyframe
  if (J.removed_kf >= 0) seed_remove_keyframe(l, S, J.removed_kf, lane, n_sp, n_ss);

  // -- 2. the cells that hold a corner (and, for the report, the cells that were occupied)
  unsigned long long* const keys = b.keys + (size_t)pos * (size_t)b.n_cells;
  const uint8_t* const occ = b.occ + (size_t)pos * (size_t)b.n_cells;
  int n_new = 0, n_occ = 0;
  for (int base = 0; base < b.n_cells; base += 64) {
    const int i = base + lane;
    const bool in = i < b.n_cells;
    n_new += __popcll(__ballot(in && keys[i] != 0ull));
    n_occ += __popcll(__ballot(in && occ[i] != 0));
  }

  // -- 3. room for all of them or for none: the rows the stream was laid out with
  const bool room = n_sp + n_new <= J.lim_pt;

  // -- 4. one seed per key, in cell order, behind the live rows; every key that was read is armed again
  int at = 0;
  for (int base = 0; base < b.n_cells; base += 64) {
    const int i = base + lane;
    unsigned long long key = 0ull;
    if (i < b.n_cells) { key = keys[i]; if (key) keys[i] = 0ull; }
    const unsigned long long m = __ballot(key != 0ull);
    if (key && room) {
      const uint32_t p = ~(uint32_t)key;
      const int L = (int)(p >> 26), y = (int)((p >> 13) & 8191u), x = (int)(p & 8191u);
      const long long r = S.pt_off + n_sp + at + seed_rank(m, lane);
      const double px[2] = { (double)(x << L), (double)(y << L) };
      // cam2world of the seed tables' camera: sel_bearing's expressions (select_device.hpp), uncontracted
      const double bx = (px[0] - s.cx) / s.fx, by = (px[1] - s.cy) / s.fy;
      const double bn = sqrt((bx * bx + by * by) + 1.0);
      const double f[3] = { bx / bn, by / bn, 1.0 / bn };
      const double grad[2] = { 1.0, 0.0 };
      seed_mut(s.pt_ref_frame)[r] = J.new_kf; l.pt_batch_id[r] = counter; seed_mut(s.pt_level)[r] = L; seed_mut(s.pt_type)[r] = PLSVO_FTR_CORNER;
      seed_st2(seed_mut(s.pt_px) + 2 * r, px); new_copy3(seed_mut(s.pt_f) + 3 * r, f); seed_st2(seed_mut(s.pt_grad) + 2 * r, grad);
      seed_mut(s.pt_a)[r] = 10.0f; seed_mut(s.pt_b)[r] = 10.0f; seed_mut(s.pt_mu)[r] = J.mu; seed_mut(s.pt_z_range)[r] = J.z_range; seed_mut(s.pt_sigma2)[r] = J.sigma2;
    }
    at += __popcll(m);
  }

  // -- 5. the uploaded line seeds
  if (room) seed_append_segments(l, S, lane, n_ss, J.n_seg, J.seg_at, J.new_kf, counter, J.mu, J.z_range, J.sigma2);

  // -- 6. the counts and the report, last
  if (lane == 0) {
    SeedStartReportDev R;
    R.n_new_pt = room ? n_new : 0; R.n_new_seg = room ? J.n_seg : 0;
    R.n_pt_seeds = n_sp + R.n_new_pt; R.n_seg_seeds = n_ss + R.n_new_seg; R.batch_counter = counter; R.no_room = room ? 0 : 1; R.n_occupied = n_occ; R.reserved0 = 0;
    S.n_pt = R.n_pt_seeds; S.n_seg = R.n_seg_seeds; S.batch_counter = counter;
    b.report[J.stream] = R;
  }
}


}  // namespace plsvo_hip
