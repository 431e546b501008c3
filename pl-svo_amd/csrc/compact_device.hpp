// compact_device.hpp -- the resident map tables close up over their deleted landmark rows on gfx950: one WAVE per
// stream, four waves per workgroup, no LDS, no atomics, nothing synchronised across waves; a stream that stands by returns at once.
// Included by seeds_kernels.hip like the other map kernels (the kernel moves rows, it computes nothing).
//
//   map_compact_kernel       Map::emptyTrash (src/map.cpp:259-275, :361-367, :453-459) as list surgery on rows: the landmarks whose type is TYPE_DELETED
//                            leave, every reference to a landmark follows its row (tests/np_compact.py)
//
// The sequential loops become order-independent forms, all in place -- a destination never lies above its source, and a round has
// everything at or below it in registers before its first store (seedlist_device.hpp's rule):
//   * a live row's new index is its rank among the live rows: ballot prefix in rounds of 64; the remap goes to per-landmark scratch;
//   * the per-landmark arrays (position(s), type, both counters, event byte, last_structure_optim_ key) close up in those rounds;
//   * the new observation offsets are a __shfl_up scan of the surviving lengths, carried across the rounds;
//   * the observation entries of a round's 64 landmarks are one contiguous range of the old arrays: the wave walks it 64 ENTRIES at a
//     time, a lane finds its entry's landmark among the round's 64 by a six-step search over their (non-decreasing) list ends, and the
//     entry moves to new start + position in its list.  Lanes are full whatever the list lengths are, and no staging copy is needed:
//     every entry travels once (the insertion stages because its lists GROW at the front; here they only move down);
//   * the keyframes' feature lists are rewritten through the remap, the candidate lists with the insertion's stable compaction.
// One lane stores the counts and the report last.
#pragma once
#include <hip/hip_runtime.h>

#include "newcand_device.hpp"

namespace plsvo_hip {

#pragma clang fp contract(off)

constexpr int kCmpWaves = kInsWaves;

__device__ __forceinline__ void cmp_ld2(double* d, const double* g) { const double2 v = *reinterpret_cast<const double2*>(g); d[0] = v.x; d[1] = v.y; }
__device__ __forceinline__ void cmp_st2(double* g, const double* d) { *reinterpret_cast<double2*>(g) = make_double2(d[0], d[1]); }

// One kind of landmark of one stream.  out: rows after, observation entries before / after, candidate entries after, features
// re-pointed to -1, candidate entries erased
template <bool SEG>
__device__ __forceinline__ void cmp_kind(const CompactBatchDev& b, const CandMapDev& M, int* out) {
  const CandBatchDev& c = b.c;
  const int lane = threadIdx.x & 63;
  const kf_u64 below = ((kf_u64)1 << lane) - 1;
  const long long lm_off = SEG ? M.seg_off : M.pt_off, kf_ftr = SEG ? M.kfseg_off : M.kfpt_off, obs = SEG ? M.segobs_off : M.ptobs_off;
  const long long cnd = SEG ? M.segc_off : M.ptc_off;
  const int n_lm = SEG ? M.n_seg : M.n_pt, n_cand = SEG ? M.n_seg_cand : M.n_pt_cand;
  int* const type = const_cast<int*>(SEG ? c.seg_type : c.pt_type) + lm_off;
  double* const pos0 = const_cast<double*>(SEG ? c.seg_spos : c.pt_pos) + 3 * lm_off;
  double* const pos1 = SEG ? const_cast<double*>(c.seg_epos) + 3 * lm_off : nullptr;
  int* const nfail = (SEG ? b.seg_nfail : b.pt_nfail) + lm_off; int* const nsucc = (SEG ? b.seg_nsucc : b.pt_nsucc) + lm_off;
  uint8_t* const event = (SEG ? b.seg_event : b.pt_event) + lm_off;
  int* const key = (SEG ? b.seg_key : b.pt_key) + lm_off; int* const remap = (SEG ? b.seg_remap : b.pt_remap) + lm_off;
  int* const obs_off = const_cast<int*>(SEG ? c.seg_obs_off : c.pt_obs_off) + lm_off + M.stream;
  int* const obs_kf = const_cast<int*>(SEG ? c.seg_obs_kf : c.pt_obs_kf) + obs; int* const obs_level = const_cast<int*>(SEG ? c.seg_obs_level : c.pt_obs_level) + obs;
  double* const oa = const_cast<double*>(SEG ? c.seg_obs_spx : c.pt_obs_px) + 2 * obs;                  // 2
  double* const ob = SEG ? const_cast<double*>(c.seg_obs_epx) + 2 * obs : const_cast<double*>(c.pt_obs_grad) + 2 * obs;   // 2
  double* const oc = const_cast<double*>(SEG ? c.seg_obs_sf : c.pt_obs_f) + 3 * obs;                    // 3
  double* const od = SEG ? const_cast<double*>(c.seg_obs_ef) + 3 * obs : nullptr;                       // 3
  uint8_t* const otype = SEG ? nullptr : const_cast<uint8_t*>(c.pt_obs_type) + obs;

  // -- the landmark rows and their observation lists, in rounds of 64 rows
  const int obs_end = obs_off[n_lm];
  int kept = 0, total = 0;                          // live rows, surviving entries below the round
  for (int base = 0; base < n_lm; base += 64) {
    const int lm = base + lane;
    const bool in = lm < n_lm;
    int t = PLSVO_LM_DELETED, o0 = obs_end, o1 = obs_end, nf = 0, ns = 0, ky = 0;
    uint8_t ev = 0;
    double p0[3] = { 0.0, 0.0, 0.0 }, p1[3] = { 0.0, 0.0, 0.0 };
    if (in) {
      t = type[lm]; o0 = obs_off[lm]; o1 = obs_off[lm + 1]; nf = nfail[lm]; ns = nsucc[lm]; ky = key[lm]; ev = event[lm];
      new_copy3(p0, pos0 + 3 * lm);
      if (SEG) new_copy3(p1, pos1 + 3 * lm);
    }
    const bool live = in && t != PLSVO_LM_DELETED;
    const kf_u64 mask = __ballot(live);             // every lane's row is in registers before the first store of the round
    const int rank = kept + __popcll(mask & below);
    const int len = live ? o1 - o0 : 0;
    const int incl = ins_wave_scan(len, lane);
    const int d0 = total + incl - len;              // where the row's list starts now
    // the round's entries: 64 at a time, each to its list's new start + its place in the list
    const int e_lo = __shfl(o0, 0, 64), e_hi = __shfl(o1, 63, 64);
    for (int e0 = e_lo; e0 < e_hi; e0 += 64) {
      const int e = e0 + lane;
      int own = 0;                                  // the round's lanes whose list ends at or below e: the lane that owns e
#pragma unroll
      for (int step = 32; step > 0; step >>= 1) { const int v = __shfl(o1, own + step - 1, 64); if (v <= e) own += step; }
      const int s0 = __shfl(o0, own, 64), dd = __shfl(d0, own, 64), lv = __shfl((int)live, own, 64);
      const bool mv = e < e_hi && lv != 0;
      const int dst = dd + (e - s0);
      int kf = 0, level = 0;
      uint8_t ty = 0;
      double a[2], bb[2], cc[3], dv[3];
      if (mv) {
        kf = obs_kf[e]; level = obs_level[e];
        cmp_ld2(a, oa + 2 * e); cmp_ld2(bb, ob + 2 * e); new_copy3(cc, oc + 3 * e);
        if (SEG) new_copy3(dv, od + 3 * e); else ty = otype[e];
      }
      cand_wave_sync();                             // every lane's entry is in registers before the first store of the round
      if (mv) {
        obs_kf[dst] = kf; obs_level[dst] = level;
        cmp_st2(oa + 2 * dst, a); cmp_st2(ob + 2 * dst, bb); new_copy3(oc + 3 * dst, cc);
        if (SEG) new_copy3(od + 3 * dst, dv); else otype[dst] = ty;
      }
    }
    if (in) remap[lm] = live ? rank : -1;
    if (live) {
      type[rank] = t; obs_off[rank] = d0; nfail[rank] = nf; nsucc[rank] = ns; key[rank] = ky; event[rank] = ev;
      new_copy3(pos0 + 3 * rank, p0);
      if (SEG) new_copy3(pos1 + 3 * rank, p1);
    }
    kept += __popcll(mask); total += __shfl(incl, 63, 64);
  }
  if (lane == 0) obs_off[kept] = total;
  // -- a freed row reads as one that was never used: its key is 0 (structsel_device.hpp relies on it), its event byte clear
  for (int lm = kept + lane; lm < n_lm; lm += 64) { key[lm] = 0; event[lm] = 0; }
  cand_wave_sync();                                 // the remap, read back by other lanes
  // -- the keyframes' feature lists through the remap; a feature on a deleted landmark has none (ftr->feat3D = NULL)
  const int* const kf_off = (SEG ? c.kf_seg_off : c.kf_pt_off) + M.kf_off + M.stream;
  int* const kf_lm = const_cast<int*>(SEG ? c.kf_seg_lm : c.kf_pt_lm) + kf_ftr;
  const int n_ftr = kf_off[M.n_kf];
  int repointed = 0;
  for (int base = 0; base < n_ftr; base += 64) {
    const int j = base + lane;
    bool dead = false;
    if (j < n_ftr) {
      const int lm = kf_lm[j];
      if (lm >= 0) { const int r = remap[lm]; dead = r < 0; kf_lm[j] = r; }
    }
    repointed += __popcll(__ballot(dead));
  }
  // -- the candidate list through the remap; an entry on a deleted landmark is erased (deleteCandidate), the list closes up
  int* const cand = const_cast<int*>(SEG ? c.seg_cand : c.pt_cand) + cnd;
  int left = 0;
  for (int base = 0; base < n_cand; base += 64) {
    const int j = base + lane;
    int r = -1;
    if (j < n_cand) r = remap[cand[j]];
    const kf_u64 mask = __ballot(r >= 0);           // every lane's load is back before the first store of the round
    if (r >= 0) cand[left + __popcll(mask & below)] = r;
    left += __popcll(mask);
  }
  out[0] = kept; out[1] = obs_end; out[2] = total; out[3] = left; out[4] = repointed; out[5] = n_cand - left;
}

__global__ __launch_bounds__(64 * kCmpWaves) void map_compact_kernel(const CompactBatchDev b) {
  const CandBatchDev& c = b.c;
  const int lane = threadIdx.x & 63;
  const int job = blockIdx.x * kCmpWaves + (int)(threadIdx.x >> 6);
  if (job >= c.n_jobs) return;                      // whole waves leave: nothing below synchronises across waves
  const CompactJobDev J = b.jobs[job];
  CandMapDev& M = const_cast<CandMapDev&>(c.maps[job]);
  const int n_pt = M.n_pt, n_seg = M.n_seg, n_ptc = M.n_pt_cand, n_segc = M.n_seg_cand;
  const int pt_end = (c.pt_obs_off + M.pt_off + M.stream)[n_pt], seg_end = (c.seg_obs_off + M.seg_off + M.stream)[n_seg];
  // the room is the device's to know: mode 2 closes a kind up only where its free rows are fewer than the caller's threshold
  const bool run_pt = J.mode == 1 || (J.mode == 2 && J.rows_pt - n_pt < J.min_room_pt);
  const bool run_seg = J.mode == 1 || (J.mode == 2 && J.rows_seg - n_seg < J.min_room_seg);
  int p[6] = { n_pt, pt_end, pt_end, n_ptc, 0, 0 }, s[6] = { n_seg, seg_end, seg_end, n_segc, 0, 0 };
  if (run_pt) cmp_kind<false>(b, M, p);
  if (run_seg) cmp_kind<true>(b, M, s);
  if (lane == 0) {
    CompactReportDev R;
    R.ran_pt = run_pt ? 1 : 0; R.ran_seg = run_seg ? 1 : 0;
    R.n_pt_before = n_pt; R.n_pt_after = p[0]; R.n_seg_before = n_seg; R.n_seg_after = s[0];
    R.n_pt_obs_before = p[1]; R.n_pt_obs_after = p[2]; R.n_seg_obs_before = s[1]; R.n_seg_obs_after = s[2];
    R.n_pt_cand_before = n_ptc; R.n_pt_cand_after = p[3]; R.n_seg_cand_before = n_segc; R.n_seg_cand_after = s[3];
    R.n_repointed_pt = p[4]; R.n_repointed_seg = s[4]; R.n_erased_pt_cand = p[5]; R.n_erased_seg_cand = s[5];
    b.report[job] = R;
    if (run_pt) { M.n_pt = p[0]; M.n_pt_cand = p[3]; }
    if (run_seg) { M.n_seg = s[0]; M.n_seg_cand = s[3]; }
  }
}

}  // namespace plsvo_hip
