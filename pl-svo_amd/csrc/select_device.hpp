// select_device.hpp -- the second half of Reprojector::reprojectMap on gfx950: one candidate per grid cell, the landmark quality that
// refine() maintains, the new frame's features and the pose optimiser's input, in place on the resident tables of the candidate stage.
// One WAVE per stream, four waves per workgroup, no LDS.  Included by seeds_kernels.hip (compiled with -ffp-contract=off: every output
// is bit-identical to tests/np_select.py; the stage has no transcendental call).
//
//   map_select_kernel   setMapCandidates' failures (src/reprojector.cpp:116-131), the two loops over the cells (:185-216),
//                       refineBestCandidate (:236-276), refine (:278-387), Map::safeDeletePoint / safeDeleteSegment (src/map.cpp:116-139),
//                       MapPointCandidates::deleteCandidatePoint and its segment twin (:311-324, :403-416), LineFeat's line (src/feature.cpp:103-104)
//   [ext] Eigen's normalize() of a 2-vector (two divisions by sqrt(x*x + y*y)), vk::PinholeCamera::cam2world
//
// The points' loop becomes order-independent, because all entries of a point lie in one cell and a trial changes its own landmark only:
//   * the winner of a cell is the lowest output index (= the cell's order after cell.sort) among its entries that succeed: atomicMin on the
//     cell's word, all ones before every launch;
//   * the stop is a prefix over the visit order: the cell at visit position v is visited iff at most max_fts cells before it have a
//     winner; the feature index of a winner is that prefix (ballots over rounds of 64 positions);
//   * an entry is tried iff its cell is visited and it does not come after the winner.
// The segments' loop stays sequential over the non-empty cells in visit order (a segment sits in two cells, and its first trial changes
// what the second sees: a promotion re-orders the second cell, a deletion silences it); inside a cell the wave works in parallel:
// the order at visit time is the key (descending type, filing index, end), the winner the lowest key that succeeds.
#pragma once
#include <hip/hip_runtime.h>

#include "candidates_device.hpp"
#include "match_device.hpp"

namespace plsvo_hip {

#pragma clang fp contract(off)

constexpr int kSelWaves = kCandWaves;
// per-landmark event bits of one launch; the first two are what plsvo_candidates_fetch_quality reports
constexpr uint8_t kSelPromoted = 1, kSelDeleted = 2, kSelInList = 4, kSelSafeDel = 8, kSelErase = 16;
constexpr unsigned int kSelNone = 0xffffffffu;

__device__ __forceinline__ int sel_wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

// refine()'s quality logic (src/reprojector.cpp:293-308, :354-370) on a landmark's registers
__device__ __forceinline__ void sel_failure(int& type, int& nf, uint8_t& ev) {
  ++nf;
  if (type == PLSVO_LM_UNKNOWN && nf > 15) { type = PLSVO_LM_DELETED; ev |= kSelDeleted | kSelSafeDel; }             // safeDeletePoint / safeDeleteSegment
  else if (type == PLSVO_LM_CANDIDATE && nf > 30 && (ev & kSelInList)) { type = PLSVO_LM_DELETED; ev |= kSelDeleted | kSelErase; }   // deleteCandidatePoint: only a listed one
}
__device__ __forceinline__ void sel_success(int& type, int& ns, uint8_t& ev) {
  ++ns;
  if (type == PLSVO_LM_UNKNOWN && ns > 10) { type = PLSVO_LM_GOOD; ev |= kSelPromoted; }
}

// unit bearing of a pixel ([ext] vk::PinholeCamera::cam2world, normalised as Feature's constructor does)
__device__ __forceinline__ void sel_bearing(const CandBatchDev& c, const double* px, double* f) {
  const double x = (px[0] - c.cx) / c.fx, y = (px[1] - c.cy) / c.fy;
  const double n = sqrt((x * x + y * y) + 1.0);
  f[0] = x / n; f[1] = y / n; f[2] = 1.0 / n;
}

// Matcher::A_cur_ref_ of matcher entry m, as match_direct_kernel computes it (match_kernels.hip: the same calls in the same order)
__device__ __forceinline__ void sel_warp_matrix(const SelectBatchDev& b, long long m, double* A) {
  const CandBatchDev& c = b.c;
  CamDev cam; cam.fx = c.fx; cam.fy = c.fy; cam.cx = c.cx; cam.cy = c.cy; cam.width = c.cam_width; cam.height = c.cam_height;
  const SE3d T_ref = se3_load(c.frame_T + 7 * c.m_ref_frame[m]), T_cur = se3_load(c.frame_T + 7 * c.m_cur_frame[m]);
  const SE3d T_ref_inv = se3_inv(T_ref);
  const SE3d T_cur_ref = se3_mul(T_cur, T_ref_inv);
  const double d0 = T_ref_inv.t[0] - c.m_pos[3 * m], d1 = T_ref_inv.t[1] - c.m_pos[3 * m + 1], d2 = T_ref_inv.t[2] - c.m_pos[3 * m + 2];
  const double depth_ref = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
  warp_matrix_affine(cam, c.m_ref_px[2 * m], c.m_ref_px[2 * m + 1], c.m_ref_f + 3 * m, depth_ref, T_cur_ref, c.m_ref_level[m], A);
}

// setMapCandidates' bookkeeping for one candidate list (src/reprojector.cpp:116-131): every listed landmark is marked, a failed projection
// costs three failures and above 30 the candidate is deleted and erased.  Returns whether an entry is to be erased (wave-uniform).
__device__ __forceinline__ bool sel_map_candidates(const int* list, int len, const uint8_t* failed, int* type, int* nfail, uint8_t* event) {
  const int lane = threadIdx.x & 63;
  bool erase = false;
  for (int base = 0; base < len; base += 64) {
    const int j = base + lane;
    bool del = false;
    if (j < len) {
      const int lm = list[j];
      uint8_t ev = kSelInList;
      if (failed[j]) {
        const int nf = nfail[lm] + 3;
        nfail[lm] = nf;
        if (nf > 30) { type[lm] = PLSVO_LM_DELETED; ev |= kSelDeleted | kSelErase; del = true; }
      }
      event[lm] = ev;
    }
    erase = erase || __ballot(del) != 0ull;
  }
  return erase;
}

// after the cells: a landmark deleted through safeDelete* leaves the keyframes' feature lists (ftr->feat3D = NULL), an erased candidate its list
__device__ __forceinline__ void sel_unlink(int* kf_lm, int n_kf_ftr, const uint8_t* event) {
  const int lane = threadIdx.x & 63;
  for (int j = lane; j < n_kf_ftr; j += 64) {
    const int lm = kf_lm[j];
    if (lm >= 0 && (event[lm] & kSelSafeDel)) kf_lm[j] = -1;
  }
}
__device__ __forceinline__ int sel_compact(int* list, int len, const uint8_t* event) {
  const int lane = threadIdx.x & 63;
  int kept = 0;
  for (int base = 0; base < len; base += 64) {
    const int j = base + lane;
    int lm = -1;
    if (j < len) lm = list[j];
    const bool keep = lm >= 0 && !(event[lm] & kSelErase);
    const kf_u64 mask = __ballot(keep);               // every lane's load is back before the first store of the round
    if (keep) list[kept + __popcll(mask & (((kf_u64)1 << lane) - 1))] = lm;
    kept += __popcll(mask);
  }
  return kept;
}

__global__ __launch_bounds__(64 * kSelWaves) void map_select_kernel(const SelectBatchDev b) {
  const CandBatchDev& c = b.c;
  const int lane = threadIdx.x & 63;
  const int job = blockIdx.x * kSelWaves + (int)(threadIdx.x >> 6);
  if (job >= c.n_jobs) return;                      // whole waves leave: nothing below synchronises across waves
  CandMapDev& M = const_cast<CandMapDev&>(c.maps[job]);
  const kf_u64 below = ((kf_u64)1 << lane) - 1;
  const int n_pt = c.counts[2 * job], n_seg = c.counts[2 * job + 1];
  int* const pt_type = const_cast<int*>(c.pt_type) + M.pt_off;
  int* const seg_type = const_cast<int*>(c.seg_type) + M.seg_off;
  int* const pt_nfail = b.pt_nfail + M.pt_off; int* const pt_nsucc = b.pt_nsucc + M.pt_off;
  int* const seg_nfail = b.seg_nfail + M.seg_off; int* const seg_nsucc = b.seg_nsucc + M.seg_off;
  uint8_t* const pt_event = b.pt_event + M.pt_off; uint8_t* const seg_event = b.seg_event + M.seg_off;
  int* const pt_cand = const_cast<int*>(c.pt_cand) + M.ptc_off;
  int* const seg_cand = const_cast<int*>(c.seg_cand) + M.segc_off;
  const long long m_pt = M.m_off, m_s = M.m_off + n_pt, m_e = M.m_off + n_pt + n_seg;

  // -- the map's candidates that did not project, in list order, before the cells
  const bool erase_pt0 = sel_map_candidates(pt_cand, M.n_pt_cand, c.pt_cand_failed + M.ptc_off, pt_type, pt_nfail, pt_event);
  const bool erase_seg0 = sel_map_candidates(seg_cand, M.n_seg_cand, c.seg_cand_failed + M.segc_off, seg_type, seg_nfail, seg_event);
  cand_wave_sync();

  // -- points: the winner of every cell
  unsigned int* const win = b.cell_win + (long long)job * b.n_cells;
  const int* const o_lm = c.o_pt_lm + M.opt_off; const int* const o_cell = c.o_pt_cell + M.opt_off; const uint8_t* const o_view = c.o_pt_view + M.opt_off;
  for (int i = lane; i < n_pt; i += 64)
    if (pt_type[o_lm[i]] != PLSVO_LM_DELETED && o_view[i] && b.found[m_pt + i]) atomicMin(&win[o_cell[i]], (unsigned int)i);
  cand_wave_sync();

  // -- points: the cells in visit order; the winners become features until the count exceeds max_fts
  int n_win = 0, v_stop = 0x7fffffff;
  for (int base = 0; base < b.n_cells && v_stop == 0x7fffffff; base += 64) {
    const int v = base + lane;
    unsigned int w = kSelNone;
    if (v < b.n_cells) w = cand_visit_load(&win[b.cell_order[v]]);
    const bool has = w != kSelNone;
    const kf_u64 mask = __ballot(has);
    const int k = n_win + __popcll(mask & below);
    if (has && k <= b.max_fts) {                    // feature k of the new frame
      const long long m = m_pt + w, o = M.opt_off + k;
      const double px[2] = { b.px_out[2 * m], b.px_out[2 * m + 1] };
      const int level = b.search_level[m];
      uint8_t ftype = PLSVO_FTR_CORNER;
      double g0 = 1.0, g1 = 0.0;                    // PointFeat's constructor (src/feature.cpp:56)
      if (c.m_ref_type[m] == PLSVO_FTR_EDGELET) {   // new_feature->grad = A_cur_ref * ref grad, normalised (:319-327)
        double A[4];
        sel_warp_matrix(b, m, A);
        const double r0 = c.m_ref_grad[2 * m], r1 = c.m_ref_grad[2 * m + 1];
        g0 = A[0] * r0 + A[1] * r1; g1 = A[2] * r0 + A[3] * r1;
        const double n = sqrt(g0 * g0 + g1 * g1);
        g0 /= n; g1 /= n;
        ftype = PLSVO_FTR_EDGELET;
      }
      b.f_pt_lm[o] = o_lm[w]; b.f_pt_px[2 * o] = px[0]; b.f_pt_px[2 * o + 1] = px[1]; b.f_pt_level[o] = level; b.f_pt_type[o] = ftype;
      b.f_pt_grad[2 * o] = g0; b.f_pt_grad[2 * o + 1] = g1;
      double f[3];
      sel_bearing(c, px, f);
#pragma unroll
      for (int d = 0; d < 3; ++d) { b.pt_f[3 * o + d] = f[d]; b.pt_pos[3 * o + d] = c.m_pos[3 * m + d]; }
      b.pt_level[o] = max(level, 0);
    }
    const kf_u64 stop = __ballot(has && k == b.max_fts);
    if (stop) v_stop = base + (int)__builtin_ctzll(stop);
    n_win += __popcll(mask);
  }
  const int n_matches = n_win <= b.max_fts ? n_win : b.max_fts + 1;

  // -- points: every entry of a visited cell up to and including its winner is a trial
  int n_trials = 0;
  bool unlink_pt = false, erase_pt = erase_pt0;
  for (int base = 0; base < n_pt; base += 64) {
    const int i = base + lane;
    bool trial = false;
    uint8_t ev = 0;
    if (i < n_pt) {
      const int cell = o_cell[i];
      const unsigned int w = cand_visit_load(&win[cell]);
      trial = b.cell_pos[cell] <= v_stop && (unsigned int)i <= w;
      if (trial) {
        const int lm = o_lm[i];
        int type = pt_type[lm];
        if (type != PLSVO_LM_DELETED) {             // refine(): TYPE_DELETED returns false at once
          ev = pt_event[lm];
          if ((unsigned int)i == w) { int ns = pt_nsucc[lm]; sel_success(type, ns, ev); pt_nsucc[lm] = ns; }
          else { int nf = pt_nfail[lm]; sel_failure(type, nf, ev); pt_nfail[lm] = nf; }
          pt_type[lm] = type; pt_event[lm] = ev;
        }
      }
    }
    n_trials += __popcll(__ballot(trial));
    unlink_pt = unlink_pt || __ballot(ev & kSelSafeDel) != 0ull;
    erase_pt = erase_pt || __ballot(ev & kSelErase) != 0ull;
  }

  // -- segments: output index of every filed landmark (the first-visit words are free until the next candidate run re-arms them)
  unsigned int* const s_idx = c.visit + M.vis_seg_off;
  const int* const os_lm = c.o_seg_lm + M.oseg_off; const uint8_t* const os_view = c.o_seg_view + M.oseg_off;
  const int* const ts_lm = c.t_seg_lm + M.oseg_off; const int* const ts_cell = c.t_seg_cell + 2 * M.oseg_off;
  for (int i = lane; i < n_seg; i += 64) s_idx[os_lm[i]] = (unsigned int)i;
  cand_wave_sync();

  // -- segments: the non-empty cells in visit order
  int n_ls = 0, cur = -1;
  bool unlink_seg = false, erase_seg = erase_seg0;
  while (true) {                                    // (wave-uniform)
    int nxt = 0x7fffffff, best = 0x7fffffff;
    for (int base = 0; base < n_seg; base += 64) {
      const int f = base + lane;
      if (f < n_seg) {
        const int p0 = b.seg_cell_pos[ts_cell[2 * f]], p1 = b.seg_cell_pos[ts_cell[2 * f + 1]];
        if (p0 > cur) nxt = min(nxt, p0);
        if (p1 > cur) nxt = min(nxt, p1);
      }
    }
    nxt = sel_wave_min(nxt);
    if (nxt == 0x7fffffff) break;
    cur = nxt;
    // the cell's order after cell.sort(lineQualityComparator): descending type_ at this moment, then filing order; its first success
    for (int base = 0; base < n_seg; base += 64) {
      const int f = base + lane;
      if (f < n_seg) {
        const int e = b.seg_cell_pos[ts_cell[2 * f]] == cur ? 0 : (b.seg_cell_pos[ts_cell[2 * f + 1]] == cur ? 1 : -1);
        if (e >= 0) {
          const int lm = ts_lm[f], type = seg_type[lm];
          const unsigned int i = s_idx[lm];
          if (type != PLSVO_LM_DELETED && os_view[i] && b.found[m_s + i] && b.found[m_e + i]) best = min(best, (3 - type) * 2 * n_seg + 2 * f + e);
        }
      }
    }
    best = sel_wave_min(best);
    for (int base = 0; base < n_seg; base += 64) {
      const int f = base + lane;
      bool trial0 = false, trial1 = false;
      uint8_t ev = 0;
      if (f < n_seg) {
        const bool in0 = b.seg_cell_pos[ts_cell[2 * f]] == cur, in1 = b.seg_cell_pos[ts_cell[2 * f + 1]] == cur;
        if (in0 || in1) {
          const int lm = ts_lm[f];
          const unsigned int i = s_idx[lm];
          int type = seg_type[lm], nf = seg_nfail[lm], ns = seg_nsucc[lm];
          const int key = (3 - type) * 2 * n_seg + 2 * f;
          ev = seg_event[lm];
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            if (!(e ? in1 : in0) || key + e > best) continue;
            if (e) trial1 = true; else trial0 = true;
            if (type == PLSVO_LM_DELETED) continue; // refine(): no counter changes; deleted by the trial before counts here too
            if (key + e == best) {
              sel_success(type, ns, ev);
              const long long o = 2 * M.oseg_off + n_ls;   // LineFeat of the new frame (:373-374)
              const double spx[2] = { b.px_out[2 * (m_s + i)], b.px_out[2 * (m_s + i) + 1] }, epx[2] = { b.px_out[2 * (m_e + i)], b.px_out[2 * (m_e + i) + 1] };
              const int level = b.search_level[m_e + i];    // Matcher::search_level_ after findMatchDirect(LineSeg): the end point's
              b.f_seg_lm[o] = lm; b.f_seg_level[o] = level;
              b.f_seg_px[4 * o] = spx[0]; b.f_seg_px[4 * o + 1] = spx[1]; b.f_seg_px[4 * o + 2] = epx[0]; b.f_seg_px[4 * o + 3] = epx[1];
              double sf[3], ef[3];
              sel_bearing(c, spx, sf); sel_bearing(c, epx, ef);
              const double l[3] = { sf[1] * ef[2] - sf[2] * ef[1], sf[2] * ef[0] - sf[0] * ef[2], sf[0] * ef[1] - sf[1] * ef[0] };
              const double n = sqrt(l[0] * l[0] + l[1] * l[1]);
#pragma unroll
              for (int d = 0; d < 3; ++d) { b.seg_line[3 * o + d] = l[d] / n; b.seg_spos[3 * o + d] = c.m_pos[3 * (m_s + i) + d]; b.seg_epos[3 * o + d] = c.m_pos[3 * (m_e + i) + d]; }
              b.seg_level[o] = max(level, 0);
            } else {
              sel_failure(type, nf, ev);
            }
          }
          if (trial0 || trial1) { seg_type[lm] = type; seg_nfail[lm] = nf; seg_nsucc[lm] = ns; seg_event[lm] = ev; }
        }
      }
      n_trials += __popcll(__ballot(trial0)) + __popcll(__ballot(trial1));
      unlink_seg = unlink_seg || __ballot(ev & kSelSafeDel) != 0ull;
      erase_seg = erase_seg || __ballot(ev & kSelErase) != 0ull;
    }
    if (best != 0x7fffffff && ++n_ls > b.max_fts_segs) break;
    cand_wave_sync();                               // the next cell reads the types this one wrote
  }
  cand_wave_sync();

  // -- the map after the frame
  const int n_kf = M.n_kf;
  if (unlink_pt) sel_unlink(const_cast<int*>(c.kf_pt_lm) + M.kfpt_off, (c.kf_pt_off + M.kf_off + M.stream)[n_kf], pt_event);
  if (unlink_seg) sel_unlink(const_cast<int*>(c.kf_seg_lm) + M.kfseg_off, (c.kf_seg_off + M.kf_off + M.stream)[n_kf], seg_event);
  int n_ptc = M.n_pt_cand, n_segc = M.n_seg_cand;
  if (erase_pt) n_ptc = sel_compact(pt_cand, n_ptc, pt_event);
  if (erase_seg) n_segc = sel_compact(seg_cand, n_segc, seg_event);
  if (lane == 0) {
    if (erase_pt) M.n_pt_cand = n_ptc;
    if (erase_seg) M.n_seg_cand = n_segc;
    b.scalars[3 * job] = n_matches; b.scalars[3 * job + 1] = n_ls; b.scalars[3 * job + 2] = n_trials;
    PoseJobDev& P = b.po_jobs[job];
    const double* T = c.frame_T + 7 * (M.f_off + n_kf);     // the new frame's pose, as the candidate stage left it
#pragma unroll
    for (int d = 0; d < 7; ++d) P.T0[d] = T[d];
    P.fx = fabs(c.fx); P.reproj_thresh = b.reproj_thresh; P.n_iter = b.po_n_iter; P.n_iter_ref = -1;
    P.pt_off = (int)M.opt_off; P.n_pts = n_matches; P.seg_off = (int)(2 * M.oseg_off); P.n_seg = n_ls;
    P.ldlt_flavour = b.ldlt_flavour; P.reserved0 = 0;
  }
}

}  // namespace plsvo_hip
