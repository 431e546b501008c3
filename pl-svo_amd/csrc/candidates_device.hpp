// candidates_device.hpp -- the candidate set of Reprojector::reprojectMap on gfx950: one WAVE per stream, four waves per workgroup, no
// host round trip inside a call.  Included by seeds_kernels.hip (compiled with -ffp-contract=off: every output is bit-identical to
// tests/np_candidates.py; the stage has no transcendental call).
//
//   map_candidates_kernel     the loop over the overlap keyframes of Reprojector::reprojectMap (src/reprojector.cpp:157-172) with
//                             setKfCandidates (:92-109), setMapCandidates (:111-133, :180-182) and reproject (:389-423);
//                             Point::getCloseViewObs / LineSeg::getCloseViewObs (src/feature3D.cpp:80-125), which the matcher calls
//                             first (src/matcher.cpp:165, :239); the order cell.sort(pointQualityComparator) leaves (:219-276)
//   [ext] Eigen's normalize() (three divisions by the norm), dot() and norm() as (x*x + y*y) + z*z
//
// The sequential loops of the reference become order-independent forms:
//   * "project a landmark once" (last_projected_kf_id_): every visit offers its index to the landmark's word of the stream's scratch row
//     with atomicMin; the visit that finds its own index there afterwards is the first one.  The row is all ones before every launch;
//   * filing order: the visits are taken again in rounds of 64 in visit order, a filed landmark's place is the count so far plus the
//     filed lanes below it (ballot prefix);
//   * stable descending order of type_: a landmark's place is the number of filed landmarks of a higher type plus the landmarks of its
//     own type filed before it -- four class counts from the filing pass, four ballots per round in the second;
//   * the counts per keyframe are sums of the ballots' population counts;
//   * the closest view is the reference's own loop, one lane per filed landmark over its observation list.
#pragma once
#include <hip/hip_runtime.h>

#include "keyframe_device.hpp"

namespace plsvo_hip {

#pragma clang fp contract(off)

constexpr int kCandWaves = kKfWaves;              // streams per workgroup
constexpr int kCandTypes = 4;                     // TYPE_DELETED < TYPE_CANDIDATE < TYPE_UNKNOWN < TYPE_GOOD (include/plsvo/feature3D.h:55-59)

// a landmark's first-visit word after the atomics of the wave: read past the vector cache, which the atomics do not go through
__device__ __forceinline__ unsigned int cand_visit_load(const unsigned int* p) {
#if defined(PLSVO_WAVE_EMU)
  return *p;
#else
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}

// everything the wave has sent to memory -- atomics included -- has arrived, and the compiler keeps the order
__device__ __forceinline__ void cand_wave_sync() {
#if !defined(PLSVO_WAVE_EMU)
  __builtin_amdgcn_s_waitcnt(0);
#endif
  wave_lds_fence();
}

// Reprojector::reproject for one position: the arithmetic and the tests of match_kernels.hip::reproject_kernel
__device__ __forceinline__ int cand_project(const CandBatchDev& b, const SE3d& T, const double* pos, int cell_size, int n_cols, double* px) {
  double c[3];
  se3_act(T, pos, c);
  const double u = c[0] / c[2], v = c[1] / c[2];
  const double px0 = b.fx * u + b.cx, px1 = b.fy * v + b.cy;
  int cell = -1;
  if (px0 == px0 && px1 == px1 && fabs(px0) < 1e9 && fabs(px1) < 1e9) {
    const int ox = (int)px0, oy = (int)px1;
    if (ox >= b.boundary && ox < b.cam_width - b.boundary && oy >= b.boundary && oy < b.cam_height - b.boundary)
      cell = (int)(px1 / cell_size) * n_cols + (int)(px0 / cell_size);
  }
  px[0] = px0; px[1] = px1;
  return cell;
}

// one kind of landmark (points or segments) of one stream
struct CandKind {
  const int* kf_off; const int* kf_lm;            // the keyframes' feature lists: CSR offsets (n_kf + 1) and landmark indices (-1 = no landmark)
  const double* pos0; const double* pos1;         // pos_ (points) / spos_, epos_ (segments)
  const int* type;
  const int* obs_off; const int* obs_kf;
  unsigned int* visit;
  int* t_lm; double* t_px; int* t_cell;           // filing order
  int cell_size, n_cols;
};

// setKfCandidates' offers: every feature of the list that has a landmark offers its visit index
__device__ __forceinline__ void cand_offer_list(const CandKind& K, const int* list, int len, unsigned int vbase) {
  const int lane = threadIdx.x & 63;
  for (int j = lane; j < len; j += 64) {
    const int lm = list[j];
    if (lm >= 0) atomicMin(&K.visit[lm], vbase + (unsigned int)j);
  }
}

// One list in order: a keyframe's features (first_visit: only the visit that won its landmark projects) or the map's candidates
// (every entry projects; failed: a flag per entry).  Files the landmarks that project inside the frame at n_filed .., counts them per
// type, returns how many.  Control flow is wave-uniform.
template <bool SEG>
__device__ __forceinline__ int cand_file_list(const CandBatchDev& b, const CandKind& K, const SE3d& T, const int* list, int len, unsigned int vbase,
                                              bool first_visit, uint8_t* failed, int& n_filed, int* cls) {
  const int lane = threadIdx.x & 63;
  int ok = 0;
  for (int base = 0; base < len; base += 64) {
    const int j = base + lane;
    bool filed = false;
    int lm = -1, t = -1, cell0 = -1, cell1 = -1;
    double px[4] = { 0.0, 0.0, 0.0, 0.0 };
    if (j < len) {
      lm = list[j];
      if (lm >= 0 && (!first_visit || cand_visit_load(&K.visit[lm]) == vbase + (unsigned int)j)) {
        cell0 = cand_project(b, T, K.pos0 + 3 * lm, K.cell_size, K.n_cols, px);
        if (SEG) cell1 = cand_project(b, T, K.pos1 + 3 * lm, K.cell_size, K.n_cols, px + 2);
        filed = cell0 >= 0 && (!SEG || cell1 >= 0);
      }
      if (failed) failed[j] = filed ? 0 : 1;
      if (filed) t = K.type[lm];
    }
    const kf_u64 mask = __ballot(filed);
    if (filed) {
      const int at = n_filed + __popcll(mask & (((kf_u64)1 << lane) - 1));
      K.t_lm[at] = lm;
      if (SEG) {
        K.t_px[4 * at] = px[0]; K.t_px[4 * at + 1] = px[1]; K.t_px[4 * at + 2] = px[2]; K.t_px[4 * at + 3] = px[3];
        K.t_cell[2 * at] = cell0; K.t_cell[2 * at + 1] = cell1;
      } else {
        K.t_px[2 * at] = px[0]; K.t_px[2 * at + 1] = px[1];
        K.t_cell[at] = cell0;
      }
    }
#pragma unroll
    for (int c = 0; c < kCandTypes; ++c) cls[c] += __popcll(__ballot(t == c));
    const int n = __popcll(mask);
    n_filed += n; ok += n;
  }
  return ok;
}

// getCloseViewObs: the observation (index into the stream's observation arrays) with the largest cosine above 0, the first of the list
// when none is, -1 for an empty list; has_view = !(best < 0.5).  A NaN cosine never wins.
__device__ __forceinline__ int cand_close_view(const double* framepos, const double* p, const int* obs_kf, int o_begin, int o_end, const double* kf_pos,
                                               bool* has_view) {
  double ox = framepos[0] - p[0], oy = framepos[1] - p[1], oz = framepos[2] - p[2];
  const double on = sqrt((ox * ox + oy * oy) + oz * oz);
  ox /= on; oy /= on; oz /= on;
  double best = 0.0;
  int at = o_begin;
  for (int o = o_begin; o < o_end; ++o) {
    const double* kp = kf_pos + 3 * obs_kf[o];
    double dx = kp[0] - p[0], dy = kp[1] - p[1], dz = kp[2] - p[2];
    const double dn = sqrt((dx * dx + dy * dy) + dz * dz);
    dx /= dn; dy /= dn; dz /= dn;
    const double cos_angle = (ox * dx + oy * dy) + oz * dz;
    if (cos_angle > best) { best = cos_angle; at = o; }
  }
  if (o_begin >= o_end) { *has_view = false; return -1; }
  *has_view = !(best < 0.5);
  return at;
}

__global__ __launch_bounds__(64 * kCandWaves) void map_candidates_kernel(const CandBatchDev b) {
  const int lane = threadIdx.x & 63;
  const int job = blockIdx.x * kCandWaves + (int)(threadIdx.x >> 6);
  if (job >= b.n_jobs) return;                      // whole waves leave: nothing below synchronises across waves
  const CandMapDev& M = b.maps[job];
  const CandJobDev& J = b.jobs[job];
  const SE3d T = se3_load(J.d_T ? J.d_T : J.T);
  const int n_kf = M.n_kf, n_ov = J.n_ov;
  const int* ov = b.overlap_idx + J.ov_off;

  CandKind P, S;
  P.kf_off = b.kf_pt_off + M.kf_off + M.stream; P.kf_lm = b.kf_pt_lm + M.kfpt_off;
  P.pos0 = b.pt_pos + 3 * M.pt_off; P.pos1 = nullptr; P.type = b.pt_type + M.pt_off;
  P.obs_off = b.pt_obs_off + M.pt_off + M.stream; P.obs_kf = b.pt_obs_kf + M.ptobs_off;
  P.visit = b.visit + M.vis_pt_off;
  P.t_lm = b.t_pt_lm + M.opt_off; P.t_px = b.t_pt_px + 2 * M.opt_off; P.t_cell = b.t_pt_cell + M.opt_off;
  P.cell_size = b.cell_size; P.n_cols = b.grid_n_cols;
  S.kf_off = b.kf_seg_off + M.kf_off + M.stream; S.kf_lm = b.kf_seg_lm + M.kfseg_off;
  S.pos0 = b.seg_spos + 3 * M.seg_off; S.pos1 = b.seg_epos + 3 * M.seg_off; S.type = b.seg_type + M.seg_off;
  S.obs_off = b.seg_obs_off + M.seg_off + M.stream; S.obs_kf = b.seg_obs_kf + M.segobs_off;
  S.visit = b.visit + M.vis_seg_off;
  S.t_lm = b.t_seg_lm + M.oseg_off; S.t_px = b.t_seg_px + 4 * M.oseg_off; S.t_cell = b.t_seg_cell + 2 * M.oseg_off;
  S.cell_size = b.seg_cell_size; S.n_cols = b.seg_grid_n_cols;

  // -- Frame::pos() of every keyframe of the table, once; the matcher's frame table gets the new frame behind the keyframes
  double* kf_pos = b.kf_pos + 3 * M.kf_off;
  for (int i = lane; i < n_kf; i += 64) {
    const SE3d Ki = se3_inv(se3_load(b.kf_T + 7 * (M.kf_off + i)));
    kf_pos[3 * i] = Ki.t[0]; kf_pos[3 * i + 1] = Ki.t[1]; kf_pos[3 * i + 2] = Ki.t[2];
  }
  if (lane == 0) {
    se3_store(T, b.frame_T + 7 * (M.f_off + n_kf));
    b.frame_slot[M.f_off + n_kf] = J.cur_slot;
  }

  // -- visits: every feature with a landmark offers its index in visit order (points and segments are separate landmark spaces)
  {
    unsigned int vp = 0, vs = 0;
    for (int r = 0; r < n_ov; ++r) {
      const int k = ov[r];
      const int p0 = P.kf_off[k], p1 = P.kf_off[k + 1], s0 = S.kf_off[k], s1 = S.kf_off[k + 1];
      cand_offer_list(P, P.kf_lm + p0, p1 - p0, vp);
      cand_offer_list(S, S.kf_lm + s0, s1 - s0, vs);
      vp += (unsigned int)(p1 - p0); vs += (unsigned int)(s1 - s0);
    }
  }
  cand_wave_sync();                                 // the wave's own atomics and stores to kf_pos, read back by all of its lanes

  // -- projection of the winning visits and of the map's candidates, filed in order
  int n_pt = 0, n_seg = 0;
  int cls_pt[kCandTypes] = { 0, 0, 0, 0 }, cls_seg[kCandTypes] = { 0, 0, 0, 0 };
  {
    unsigned int vp = 0, vs = 0;
    for (int r = 0; r < n_ov; ++r) {
      const int k = ov[r];
      const int p0 = P.kf_off[k], p1 = P.kf_off[k + 1], s0 = S.kf_off[k], s1 = S.kf_off[k + 1];
      int ok = cand_file_list<false>(b, P, T, P.kf_lm + p0, p1 - p0, vp, true, nullptr, n_pt, cls_pt);
      ok += cand_file_list<true>(b, S, T, S.kf_lm + s0, s1 - s0, vs, true, nullptr, n_seg, cls_seg);
      vp += (unsigned int)(p1 - p0); vs += (unsigned int)(s1 - s0);
      if (lane == 0) b.kf_count[J.ov_off + r] = ok;
    }
  }
  cand_file_list<false>(b, P, T, b.pt_cand + M.ptc_off, M.n_pt_cand, 0u, false, b.pt_cand_failed + M.ptc_off, n_pt, cls_pt);
  cand_file_list<true>(b, S, T, b.seg_cand + M.segc_off, M.n_seg_cand, 0u, false, b.seg_cand_failed + M.segc_off, n_seg, cls_seg);
  cand_wave_sync();                                 // the filing-order rows, read back by other lanes

  // -- closest view and output order
  const SE3d Tinv = se3_inv(T);
  const int cur_frame = (int)M.f_off + n_kf;
  for (int kind = 0; kind < 2; ++kind) {            // points, then segments
    const bool seg = kind != 0;
    const CandKind& K = seg ? S : P;
    const int n_filed = seg ? n_seg : n_pt;
    const int* cls = seg ? cls_seg : cls_pt;
    int place[kCandTypes];                          // descending type: GOOD first, DELETED last
    place[3] = 0; place[2] = cls[3]; place[1] = cls[3] + cls[2]; place[0] = cls[3] + cls[2] + cls[1];
    for (int base = 0; base < n_filed; base += 64) {
      const int f = base + lane;
      int lm = -1, t = -1, obs = -1;
      bool has_view = false;
      double p[3] = { 0.0, 0.0, 0.0 };
      if (f < n_filed) {
        lm = K.t_lm[f]; t = K.type[lm];
        if (seg) {
#pragma unroll
          for (int k = 0; k < 3; ++k) p[k] = 0.5 * (K.pos0[3 * lm + k] + K.pos1[3 * lm + k]);
        } else {
#pragma unroll
          for (int k = 0; k < 3; ++k) p[k] = K.pos0[3 * lm + k];
        }
        obs = cand_close_view(Tinv.t, p, K.obs_kf, K.obs_off[lm], K.obs_off[lm + 1], kf_pos, &has_view);
      }
      int rank = 0;
#pragma unroll
      for (int c = 0; c < kCandTypes; ++c) {
        const kf_u64 mask = __ballot(t == c);
        if (t == c) rank = place[c] + __popcll(mask & (((kf_u64)1 << lane) - 1));
        place[c] += __popcll(mask);
      }
      if (f >= n_filed) continue;
      const uint8_t active = (t != 0 && has_view) ? 1 : 0;
      const int obs_local = obs < 0 ? -1 : obs - K.obs_off[lm];
      const int ref_frame = (int)M.f_off + (obs < 0 ? 0 : K.obs_kf[obs]);
      if (!seg) {
        const long long o = M.opt_off + rank;
        b.o_pt_lm[o] = lm; b.o_pt_px[2 * o] = K.t_px[2 * f]; b.o_pt_px[2 * o + 1] = K.t_px[2 * f + 1]; b.o_pt_cell[o] = K.t_cell[f];
        b.o_pt_obs[o] = obs_local; b.o_pt_view[o] = has_view ? 1 : 0; b.o_pt_active[o] = active;
        const long long m = M.m_off + rank;
        double rf[3] = { 0.0, 0.0, 0.0 }, rpx[2] = { 0.0, 0.0 }, rgrad[2] = { 0.0, 0.0 };
        int rlevel = 0;
        uint8_t rtype = 0;
        if (obs >= 0) {                             // an empty observation list: no address in the observation tables is formed
          const long long g = M.ptobs_off + obs;
#pragma unroll
          for (int k = 0; k < 3; ++k) rf[k] = b.pt_obs_f[3 * g + k];
#pragma unroll
          for (int k = 0; k < 2; ++k) { rpx[k] = b.pt_obs_px[2 * g + k]; rgrad[k] = b.pt_obs_grad[2 * g + k]; }
          rlevel = b.pt_obs_level[g]; rtype = b.pt_obs_type[g];
        }
        b.m_cur_frame[m] = cur_frame; b.m_ref_frame[m] = ref_frame; b.m_active[m] = active;
        b.m_px_cur[2 * m] = K.t_px[2 * f]; b.m_px_cur[2 * m + 1] = K.t_px[2 * f + 1];
#pragma unroll
        for (int k = 0; k < 3; ++k) { b.m_pos[3 * m + k] = p[k]; b.m_ref_f[3 * m + k] = rf[k]; }
#pragma unroll
        for (int k = 0; k < 2; ++k) { b.m_ref_px[2 * m + k] = rpx[k]; b.m_ref_grad[2 * m + k] = rgrad[k]; }
        b.m_ref_level[m] = rlevel; b.m_ref_type[m] = rtype;
      } else {
        const long long o = M.oseg_off + rank;
        b.o_seg_lm[o] = lm;
#pragma unroll
        for (int k = 0; k < 4; ++k) b.o_seg_px[4 * o + k] = K.t_px[4 * f + k];
        b.o_seg_cell[2 * o] = K.t_cell[2 * f]; b.o_seg_cell[2 * o + 1] = K.t_cell[2 * f + 1];
        b.o_seg_obs[o] = obs_local; b.o_seg_view[o] = has_view ? 1 : 0; b.o_seg_active[o] = active;
#pragma unroll
        for (int e = 0; e < 2; ++e) {               // start point, end point: [points | start points | end points]
          const long long m = M.m_off + n_pt + e * n_seg + rank;
          const double* pos = (e ? K.pos1 : K.pos0) + 3 * lm;
          double rf[3] = { 0.0, 0.0, 0.0 }, rpx[2] = { 0.0, 0.0 };
          int rlevel = 0;
          if (obs >= 0) {                           // an empty observation list: no address in the observation tables is formed
            const long long g = M.segobs_off + obs;
#pragma unroll
            for (int k = 0; k < 3; ++k) rf[k] = (e ? b.seg_obs_ef : b.seg_obs_sf)[3 * g + k];
#pragma unroll
            for (int k = 0; k < 2; ++k) rpx[k] = (e ? b.seg_obs_epx : b.seg_obs_spx)[2 * g + k];
            rlevel = b.seg_obs_level[g];
          }
          b.m_cur_frame[m] = cur_frame; b.m_ref_frame[m] = ref_frame; b.m_active[m] = active;
          b.m_px_cur[2 * m] = K.t_px[4 * f + 2 * e]; b.m_px_cur[2 * m + 1] = K.t_px[4 * f + 2 * e + 1];
#pragma unroll
          for (int k = 0; k < 3; ++k) { b.m_pos[3 * m + k] = pos[k]; b.m_ref_f[3 * m + k] = rf[k]; }
#pragma unroll
          for (int k = 0; k < 2; ++k) { b.m_ref_px[2 * m + k] = rpx[k]; b.m_ref_grad[2 * m + k] = 0.0; }
          b.m_ref_level[m] = rlevel; b.m_ref_type[m] = PLSVO_FTR_CORNER;
        }
      }
    }
  }

  // -- the rest of the stream's matcher entries: nothing to match
  for (int i = n_pt + 2 * n_seg + lane; i < M.cap_pt + 2 * M.cap_seg; i += 64) {
    const long long m = M.m_off + i;
    b.m_cur_frame[m] = cur_frame; b.m_ref_frame[m] = (int)M.f_off; b.m_active[m] = 0;
    b.m_px_cur[2 * m] = 0.0; b.m_px_cur[2 * m + 1] = 0.0; b.m_ref_px[2 * m] = 0.0; b.m_ref_px[2 * m + 1] = 0.0;
    b.m_ref_level[m] = 0; b.m_ref_type[m] = PLSVO_FTR_CORNER;
  }
  if (lane == 0) { b.counts[2 * job] = n_pt; b.counts[2 * job + 1] = n_seg; }
}

}  // namespace plsvo_hip
