// alignjob_device.hpp -- the NEXT frame's sparse-image-alignment job built on gfx950 from what the resident map pipeline left on the
// device: one WAVE per stream, four waves per workgroup, no LDS, nothing synchronised across waves; an inactive stream returns at once.
// Included by seeds_kernels.hip (compiled with -ffp-contract=off: every output is bit-identical to tests/np_alignjob.py; the stage's only
// transcendental call is sqrt).
//
//   map_align_job_kernel    what FrameHandlerMono::processFrame hands SparseImgAlign::run(last_frame_, new_frame_)
//                           (src/frame_handler_mono.cpp:266-274) once the tracked frame has become last_frame_: the reference frame's
//                           features that still hold a landmark, f * ||pos_ - ref_frame->pos()|| (src/sparse_img_align.cpp:229-230,
//                           :327-330), LineFeat::length (src/feature.cpp:90), the initial model cur.T_f_w * ref.T_f_w^-1 with
//                           cur.T_f_w = ref.T_f_w (:266, src/sparse_img_align.cpp:80), and the static patch-slot layout of
//                           plsvo_capi.hip::slot_layout per level -- written as one job of an alignment batch laid out by capacity
//   map_align_kf_job_kernel the same job with a keyframe row of the resident tables as the reference frame: SparseImgAlign::run(ref_keyframe,
//                           new_frame_) of relocalizeFrame (src/frame_handler_mono.cpp:408-436) and the first frame, Map::getClosestKeyframe
//                           (src/map.cpp:181-199) picking the row on request; the keyframe's feature lists and their observations in it
//   map_align_pose_kernel   cur_frame->T_f_w_ = T_cur_from_ref * ref_frame->T_f_w_ (src/sparse_img_align.cpp:92)
//   map_track_gate_kernel   the gates of processFrame behind the pose optimisation (:315-321, :335, FrameHandlerBase::setTrackingQuality,
//                           src/frame_handler_base.cpp:173-190) and the pose the frame carries forward; a lane per stream
//
// The reference frame's features are the last selection's (SelectBatchDev::f_*), its feat3D pointers the keep bytes of the pose
// optimiser's cull.  PINNED: a feature whose landmark row is TYPE_DELETED at build time counts as feat3D == NULL -- that is what
// Map::safeDeleteFrame (src/map.cpp:82-127) leaves of the landmarks it cuts loose from the new keyframe's features.  Positions are read
// from the TABLES, behind whatever optimizeStructure moved.
// LEFT OUT: writing the alignment's cull back into a keyframe's own segment features (src/sparse_img_align.cpp:687-688).
//
// The layout's sequential parts become:
//   * points: stable close-up of the kept features, ballot prefix carried across rounds of 64;
//   * shorts (N <= 64) first-fit in decreasing N, ties in feature order: a segment's place in that order is counted,
//     #{t : N_t > N_s or (N_t == N_s and t < s)}, and the walk in that order is serial -- one bin (wave-round) per lane, the first bin
//     that fits found by a ballot, kAlignJobBins bins in groups of 64;
//   * longs behind the packed rounds in feature order: a wave prefix sum of their N carried across rounds of 64.
// A stream that does not fit its reserved rows (kept points > cap_pts, segments > cap_seg, a level's slots > slot_cap or beyond the
// bins, N > 2047 -- which pixels inside an image cannot reach) is DROPPED whole and reported: its job says skip = 1 with no features,
// its feature rows are not written, its two poses are (the composed pose of a dropped stream is its reference pose).
#pragma once
#include <hip/hip_runtime.h>

#include "keystage_device.hpp"
#include "select_device.hpp"

namespace plsvo_hip {

#pragma clang fp contract(off)

constexpr int kAjWaves = kSelWaves;               // streams per workgroup
constexpr int kAjGroups = kAlignJobBinGroups;     // bin groups of 64 wave-rounds each (plsvo_dev.hpp: kAlignJobBins in all)

// ||p - ref||: the three squares added in that order
__device__ __forceinline__ double aj_dist(const double* p, const double* ref) {
  const double dx = p[0] - ref[0], dy = p[1] - ref[1], dz = p[2] - ref[2];
  return sqrt(dx * dx + dy * dy + dz * dz);
}
// LineFeat::length (src/feature.cpp:90)
__device__ __forceinline__ double aj_seg_len(const double* px4) {
  const double dx = px4[2] - px4[0], dy = px4[3] - px4[1];
  return sqrt(dx * dx + dy * dy);
}
// a segment's samples at a level, -1 when an end point fails the 3-pixel border test (slot_layout's first loop)
__device__ __forceinline__ int aj_seg_samples(const double* px4, double len, int level, int cam_w, int cam_h) {
  const double scale = 1.0 / (double)(1 << level);
  const int cw = cam_w / (1 << level), ch = cam_h / (1 << level);
  const int isx = (int)(px4[0] * scale), isy = (int)(px4[1] * scale), iex = (int)(px4[2] * scale), iey = (int)(px4[3] * scale);
  const bool vis = isx >= 3 && isx < cw - 3 && isy >= 3 && isy < ch - 3 && iex >= 3 && iex < cw - 3 && iey >= 3 && iey < ch - 3;
  return vis ? seg_num_samples(px4[0], px4[1], px4[2], px4[3], len, level) : -1;
}
__device__ __forceinline__ int aj_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The segment features a layout works on: is segment s alive, and its four pixel doubles (spx, epx; px4 may fill and return the caller's four).
//   the selection's: f_seg_px rows, alive by the keep byte and the landmark's row
struct AjSelSegs {
  const double* px; const uint8_t* keep; const int* lm; const int* type;
  __device__ __forceinline__ bool alive(int s) const { return keep[s] != 0 && type[lm[s]] != PLSVO_LM_DELETED; }
  __device__ __forceinline__ const double* px4(int s, double*) const { return px + 4 * s; }   // (the rows lie as they are read)
};
//   a resident keyframe's: the observation of the feature's landmark in that keyframe, its index kept per feature (-1: dead)
struct AjKfSegs {
  const int* obs; const double* spx; const double* epx;
  __device__ __forceinline__ bool alive(int s) const { return obs[s] >= 0; }
  __device__ __forceinline__ const double* px4(int s, double* o) const { const int k = obs[s]; o[0] = spx[2 * k]; o[1] = spx[2 * k + 1]; o[2] = epx[2 * k]; o[3] = epx[2 * k + 1]; return o; }
};

// One level's layout of one stream into row[0 .. n_seg) (codes: first slot | N << 20, or -1).  Returns false when the level cannot be
// laid out at all (N > 2047, more wave-rounds than bins).  Control flow is wave-uniform.
template <typename Segs>
__device__ __forceinline__ bool aj_layout_level(const Segs& S, int n_seg, int n_pts, int level,
                                                int cam_w, int cam_h, int seg_align, int* row, int* rank, int* n_slots, int* any_long, int* n_patches) {
  const int lane = threadIdx.x & 63;
  // -- 1. the border test and N per segment
  int n_short = 0, sum_n = 0;
  bool too_long = false, longs = false;
  for (int base = 0; base < n_seg; base += 64) {
    const int s = base + lane;
    int N = -1;
    if (s < n_seg) {
      if (S.alive(s)) { double tmp[4]; const double* p = S.px4(s, tmp); N = aj_seg_samples(p, aj_seg_len(p), level, cam_w, cam_h); }
      row[s] = N >= 0 ? (N << 20) : -1;
    }
    too_long = too_long || __ballot(N > 2047) != 0;
    longs = longs || __ballot(N > 64) != 0;
    n_short += __popcll(__ballot(N >= 0 && N <= 64));
    sum_n += N > 0 ? N : 0;
  }
  *n_patches = n_pts + aj_wave_sum(sum_n);
  *any_long = longs ? 1 : 0;
  if (too_long) return false;
  const int seg0 = (seg_align == 64 && n_seg > 0) ? ((n_pts + 63) & ~63) : n_pts;   // first slot a segment may take
  const int r0 = seg0 / 64;                         // the round the first segment may share with the last points
  int used = n_pts;
  int n_bins = 1;
  cand_wave_sync();                                 // the codes, read back by other lanes
  if (n_short > 0) {
    // -- 2. the shorts' places in decreasing N, ties in feature order
    for (int base = 0; base < n_seg; base += 64) {
      const int s = base + lane;
      const int code = s < n_seg ? row[s] : -1;
      if (code >= 0 && (code >> 20) <= 64) {
        const int N = code >> 20;
        int place = 0;
        for (int t = 0; t < n_seg; ++t) {
          const int ct = row[t];
          const int Nt = ct >> 20;
          if (ct >= 0 && Nt <= 64 && (Nt > N || (Nt == N && t < s))) ++place;
        }
        rank[place] = (N << 20) | s;
      }
    }
    cand_wave_sync();                               // the order, read back by other lanes
    // -- 3. first-fit in that order: lane k of group g holds the slots taken in round r0 + 64 g + k
    int fill[kAjGroups];
#pragma unroll
    for (int g = 0; g < kAjGroups; ++g) fill[g] = 0;
    if (lane == 0) fill[0] = seg0 - r0 * 64;
    bool overflow = false;
    for (int base = 0; base < n_short && !overflow; base += 64) {
      const int mine = base + lane < n_short ? rank[base + lane] : 0;
      const int m = n_short - base < 64 ? n_short - base : 64;
      for (int i = 0; i < m && !overflow; ++i) {
        const int e = __shfl(mine, i, 64);
        const int N = e >> 20, s = e & 0xfffff;
        int k = -1, old = 0;
#pragma unroll
        for (int g = 0; g < kAjGroups; ++g) {
          const kf_u64 fits = __ballot(k < 0 && g * 64 + lane < n_bins && fill[g] + N <= 64);
          const int w = fits ? (int)__builtin_ctzll(fits) : 0;
          const int f = __shfl(fill[g], w, 64);
          if (fits) { k = g * 64 + w; old = f; if (lane == w) fill[g] += N; }
        }
        if (k < 0) {                                // a new round
          if (n_bins >= kAlignJobBins) { overflow = true; continue; }
          k = n_bins++;
#pragma unroll
          for (int g = 0; g < kAjGroups; ++g) if (g * 64 + lane == k) fill[g] = N;
        }
        const int first = (r0 + k) * 64 + old;
        if (lane == 0) row[s] = (N << 20) | first;
        used = used > first + N ? used : first + N;
      }
    }
    if (overflow) return false;
  }
  // -- 4. longs behind the packed rounds (a two-pass level: any contiguous run of slots will do)
  if (longs) {
    cand_wave_sync();                               // lane 0's codes of the shorts, before the rows are read again
    int cur = n_short == 0 ? ((seg0 + 63) / 64) * 64 : (r0 + n_bins) * 64;
    for (int base = 0; base < n_seg; base += 64) {
      const int s = base + lane;
      const int code = s < n_seg ? row[s] : -1;
      const int N = (code >= 0 && (code >> 20) > 64) ? (code >> 20) : 0;
      int v = N;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(v, d, 64); if (lane >= d) v += t; }
      if (N > 0) row[s] = (N << 20) | ((cur + v - N) & 0xfffff);   // (a first slot beyond 20 bits belongs to a level that does not fit: the stream is dropped)
      cur += __shfl(v, 63, 64);
    }
    used = cur;
  }
  *n_slots = used;
  return true;
}

// Every level's layout of one stream, coarse to fine, into the stream's rows of the code table (nothing else is written before the stream
// is known to fit), and the record below: the keyframe build's form of map_align_job_kernel's level loop and lane-0 tail, which that kernel
// keeps inline: through these it compiles to 129 VGPRs, one granule above four waves per SIMD, and its launch at 4096 streams takes 0.148 ms
// instead of 0.110.  fits: in -- the stream's features fit their rows; out -- and every level its slots.
struct AjLayout { int n_slots[PLSVO_MAX_LEVELS]; int long_mask, patches, finest; bool fits; };
template <typename Segs>
__device__ __forceinline__ AjLayout aj_layout_levels(const AlignBuildBatchDev& b, const Segs& S, int job, int n_seg, int n_pts, bool fits) {
  const CandBatchDev& c = b.s.c;
  AjLayout L;
  L.fits = fits;
  bool laid_out = fits;
#pragma unroll
  for (int l = 0; l < PLSVO_MAX_LEVELS; ++l) L.n_slots[l] = 0;
  L.long_mask = 0; L.patches = 0; L.finest = 0;
  const size_t stride = (size_t)c.n_jobs * (size_t)b.cap_seg;
  for (int level = b.max_level; level >= b.min_level && laid_out; --level) {
    int* row = b.seg_slot + (size_t)(level - b.min_level) * stride + (size_t)job * (size_t)b.cap_seg;
    int ns = 0, any_long = 0, np = 0;
    laid_out = aj_layout_level(S, n_seg, n_pts, level, c.cam_width, c.cam_height, b.seg_align, row, b.seg_rank + (size_t)job * (size_t)b.cap_seg, &ns, &any_long, &np);
    if (!laid_out) break;
    if (ns > b.slot_cap) L.fits = false;
#pragma unroll
    for (int l = 0; l < PLSVO_MAX_LEVELS; ++l) if (l == level) L.n_slots[l] = ns;
    if (any_long) L.long_mask |= 1 << level;
    L.patches += np;
    L.finest = ns;
  }
  if (!laid_out) { L.fits = false; L.long_mask = 0; L.finest = 0; }
  return L;
}
// The stream's two poses, its job of the alignment batch, its launch-order key and its report (one lane)
__device__ __forceinline__ void aj_write_record(const AlignBuildBatchDev& b, int job, const SE3d& T0, const SE3d& T_ref, int ref_slot, int cur_slot, const AjLayout& L,
                                                int n_pts, int n_seg, int n_seg_alive, int status, int ref_code) {
  const CandBatchDev& c = b.s.c;
  const bool fits = status == kAlignJobOk;
  se3_store(T0, b.T0 + 7 * job);
  se3_store(T_ref, b.T_ref + 7 * job);
  const bool skip = !fits || (n_pts == 0 && n_seg == 0);   // src/sparse_img_align.cpp:58-62, as plsvo_align_stage sets it
  AlignJobDev& A = b.a_jobs[job];
  A.ref_slot = ref_slot; A.cur_slot = cur_slot;
  A.fx = c.fx; A.fy = c.fy; A.cx = c.cx; A.cy = c.cy; A.width = c.cam_width; A.height = c.cam_height;
  A.max_level = b.max_level; A.min_level = b.min_level; A.n_iter = b.n_iter; A.skip = skip ? 1 : 0;
  A.eps = b.eps;
  A.pt_off = job * b.cap_pts; A.n_pts = fits ? n_pts : 0; A.seg_off = job * b.cap_seg; A.n_seg = fits ? n_seg : 0;
  A.patch_off = job * b.patch_cap; A.patch_cap = b.patch_cap;
#pragma unroll
  for (int l = 0; l < PLSVO_MAX_LEVELS; ++l) A.n_slots[l] = fits ? L.n_slots[l] : 0;
  A.long_mask = fits ? L.long_mask : 0; A.ldlt_flavour = b.ldlt_flavour;
  b.work_key[job] = skip ? 0 : L.patches;
  AlignBuildReportDev& R = b.report[job];
  R.n_pts = n_pts; R.n_seg = n_seg; R.n_seg_alive = n_seg_alive; R.n_slots = L.finest; R.long_mask = L.long_mask;
  R.status = status; R.reserved0 = ref_code; R.reserved1 = 0;
}

__global__ __launch_bounds__(64 * kAjWaves) void map_align_job_kernel(const AlignBuildBatchDev b) {
  const CandBatchDev& c = b.s.c;
  const int lane = threadIdx.x & 63;
  const int job = blockIdx.x * kAjWaves + (int)(threadIdx.x >> 6);
  if (job >= c.n_jobs) return;                      // whole waves leave: nothing below synchronises across waves
  const AlignBuildJobDev& J = b.jobs[job];
  if (!J.active) return;
  const CandMapDev& M = c.maps[job];
  const kf_u64 below = ((kf_u64)1 << lane) - 1;
  // -- poses: Frame::pos() of the reference frame, the initial model (not the literal identity)
  const SE3d T_ref = se3_load(J.d_T ? J.d_T : J.T);
  const SE3d T_inv = se3_inv(T_ref);
  const SE3d T0 = se3_mul(T_ref, T_inv);
  const double ref_pos[3] = { T_inv.t[0], T_inv.t[1], T_inv.t[2] };
  // -- the reference frame's features: the selection's, the keep bytes, the landmarks' rows
  const int n_sel_pt = b.s.scalars[3 * job], n_seg = b.s.scalars[3 * job + 1];
  const int* pt_lm = b.s.f_pt_lm + M.opt_off; const double* pt_px = b.s.f_pt_px + 2 * M.opt_off; const uint8_t* pt_keep = J.pt_keep + M.opt_off;
  const int* seg_lm = b.s.f_seg_lm + 2 * M.oseg_off; const double* seg_px = b.s.f_seg_px + 8 * M.oseg_off; const uint8_t* seg_keep = J.seg_keep + 2 * M.oseg_off;
  const int* pt_type = c.pt_type + M.pt_off; const int* seg_type = c.seg_type + M.seg_off;
  const double* pt_pos = c.pt_pos + 3 * M.pt_off; const double* seg_spos = c.seg_spos + 3 * M.seg_off; const double* seg_epos = c.seg_epos + 3 * M.seg_off;
  int n_pts = 0, n_seg_alive = 0;
  for (int base = 0; base < n_sel_pt; base += 64) {
    const int i = base + lane;
    n_pts += __popcll(__ballot(i < n_sel_pt && pt_keep[i] != 0 && pt_type[pt_lm[i]] != PLSVO_LM_DELETED));
  }
  for (int base = 0; base < n_seg; base += 64) {
    const int s = base + lane;
    n_seg_alive += __popcll(__ballot(s < n_seg && seg_keep[s] != 0 && seg_type[seg_lm[s]] != PLSVO_LM_DELETED));
  }
  const AjSelSegs segs = { seg_px, seg_keep, seg_lm, seg_type };
  // -- the slot layout of every level, into the stream's rows of the code table (nothing else is written before the stream is known to fit)
  //    (INLINE COPY of aj_layout_levels, kept for the register count stated there: change the two together)
  bool fits = n_pts <= b.cap_pts && n_seg <= b.cap_seg;
  bool laid_out = fits;
  int n_slots[PLSVO_MAX_LEVELS];
#pragma unroll
  for (int l = 0; l < PLSVO_MAX_LEVELS; ++l) n_slots[l] = 0;
  int long_mask = 0, patches = 0, finest = 0;
  const size_t stride = (size_t)c.n_jobs * (size_t)b.cap_seg;
  for (int level = b.max_level; level >= b.min_level && laid_out; --level) {
    int* row = b.seg_slot + (size_t)(level - b.min_level) * stride + (size_t)job * (size_t)b.cap_seg;
    int ns = 0, any_long = 0, np = 0;
    laid_out = aj_layout_level(segs, n_seg, n_pts, level, c.cam_width, c.cam_height, b.seg_align, row, b.seg_rank + (size_t)job * (size_t)b.cap_seg, &ns, &any_long, &np);
    if (!laid_out) break;
    if (ns > b.slot_cap) fits = false;
#pragma unroll
    for (int l = 0; l < PLSVO_MAX_LEVELS; ++l) if (l == level) n_slots[l] = ns;
    if (any_long) long_mask |= 1 << level;
    patches += np;
    finest = ns;
  }
  if (!laid_out) { fits = false; long_mask = 0; finest = 0; }
  const size_t P0 = (size_t)job * (size_t)b.cap_pts, S0 = (size_t)job * (size_t)b.cap_seg;
  if (fits) {
    // -- points: the kept ones closed up stably
    int at0 = 0;
    for (int base = 0; base < n_sel_pt; base += 64) {
      const int i = base + lane;
      const bool kept = i < n_sel_pt && pt_keep[i] != 0 && pt_type[pt_lm[i]] != PLSVO_LM_DELETED;
      const kf_u64 mask = __ballot(kept);
      if (kept) {
        const size_t at = P0 + (size_t)(at0 + __popcll(mask & below));
        double f[3];
        sel_bearing(c, pt_px + 2 * i, f);
        const double d = aj_dist(pt_pos + 3 * pt_lm[i], ref_pos);
        b.pt_px[2 * at] = pt_px[2 * i]; b.pt_px[2 * at + 1] = pt_px[2 * i + 1];
        b.pt_xyz[3 * at] = f[0] * d; b.pt_xyz[3 * at + 1] = f[1] * d; b.pt_xyz[3 * at + 2] = f[2] * d;
      }
      at0 += __popcll(mask);
    }
    // -- segments: ALL of them, so that indices stay stable; a dead one keeps its pixels and gets zeros for the two 3-D vectors
    for (int s = lane; s < n_seg; s += 64) {
      const double* px4 = seg_px + 4 * s;
      const bool alive = seg_keep[s] != 0 && seg_type[seg_lm[s]] != PLSVO_LM_DELETED;
      double p[3] = { 0.0, 0.0, 0.0 }, q[3] = { 0.0, 0.0, 0.0 };
      if (alive) {
        double sf[3], ef[3];
        sel_bearing(c, px4, sf); sel_bearing(c, px4 + 2, ef);
        const double ds = aj_dist(seg_spos + 3 * seg_lm[s], ref_pos), de = aj_dist(seg_epos + 3 * seg_lm[s], ref_pos);
#pragma unroll
        for (int k = 0; k < 3; ++k) { p[k] = sf[k] * ds; q[k] = ef[k] * de; }
      }
      const size_t at = S0 + (size_t)s;
      b.seg_spx[2 * at] = px4[0]; b.seg_spx[2 * at + 1] = px4[1]; b.seg_epx[2 * at] = px4[2]; b.seg_epx[2 * at + 1] = px4[3];
      b.seg_len[at] = aj_seg_len(px4);
#pragma unroll
      for (int k = 0; k < 3; ++k) { b.seg_p[3 * at + k] = p[k]; b.seg_q[3 * at + k] = q[k]; }
      b.seg_alive_in[at] = alive ? 1 : 0;
    }
  }
  // (INLINE COPY of aj_write_record with status OK / NO_ROOM and ref_code 0, for the same reason: change the two together)
  if (lane == 0) {
    se3_store(T0, b.T0 + 7 * job);
    se3_store(T_ref, b.T_ref + 7 * job);
    const bool skip = !fits || (n_pts == 0 && n_seg == 0);   // src/sparse_img_align.cpp:58-62, as plsvo_align_stage sets it
    AlignJobDev& A = b.a_jobs[job];
    A.ref_slot = J.ref_slot; A.cur_slot = J.cur_slot;
    A.fx = c.fx; A.fy = c.fy; A.cx = c.cx; A.cy = c.cy; A.width = c.cam_width; A.height = c.cam_height;
    A.max_level = b.max_level; A.min_level = b.min_level; A.n_iter = b.n_iter; A.skip = skip ? 1 : 0;
    A.eps = b.eps;
    A.pt_off = (int)P0; A.n_pts = fits ? n_pts : 0; A.seg_off = (int)S0; A.n_seg = fits ? n_seg : 0;
    A.patch_off = job * b.patch_cap; A.patch_cap = b.patch_cap;
#pragma unroll
    for (int l = 0; l < PLSVO_MAX_LEVELS; ++l) A.n_slots[l] = fits ? n_slots[l] : 0;
    A.long_mask = fits ? long_mask : 0; A.ldlt_flavour = b.ldlt_flavour;
    b.work_key[job] = skip ? 0 : patches;
    AlignBuildReportDev& R = b.report[job];
    R.n_pts = n_pts; R.n_seg = n_seg; R.n_seg_alive = n_seg_alive; R.n_slots = finest; R.long_mask = long_mask;
    R.status = fits ? kAlignJobOk : kAlignJobNoRoom; R.reserved0 = 0; R.reserved1 = 0;
  }
}

// ---- the same job with a RESIDENT KEYFRAME as the reference frame: relocalizeFrame (src/frame_handler_mono.cpp:408-436), the first frame ----
// the first observation of landmark lm in keyframe kf (keystage_device.hpp::ks_feature_px's pairing), or -1
__device__ __forceinline__ int aj_obs_in_kf(const int* obs_off, const int* obs_kf, int lm, int kf) {
  for (int o = obs_off[lm]; o < obs_off[lm + 1]; ++o) if (obs_kf[o] == kf) return o;
  return -1;
}
// Map::getClosestKeyframe (src/map.cpp:181-199): the close keyframes' minimum by (distance, row) -- the front of the stable sort -- and,
// when that is the frame itself (self_kf), the minimum of the others.  PINNED: with self_kf the only close keyframe the reference calls
// front() on an empty list; here that is "none" (-1).  Either way it is the minimum over the close rows other than self_kf.
__device__ __forceinline__ int aj_closest_keyframe(const KsView& V, const int* kp, const double* kf_T, int n_kf, const SE3d& T, const CamDev& cam, int self_kf) {
  const int lane = threadIdx.x & 63;
  constexpr int kNone = 0x7fffffff;
  double best = 0.0; int best_i = kNone;
  for (int i = lane; i < n_kf; i += 64) {           // (rows ascend: the lower row keeps a tie)
    double d;
    if (i == self_kf || !ks_close(V, kp, kf_T, T, cam, i, &d)) continue;
    if (best_i == kNone || d < best) { best = d; best_i = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double od = __shfl_xor(best, o, 64); const int oi = __shfl_xor(best_i, o, 64);
    if (oi != kNone && (best_i == kNone || od < best || (od == best && oi < best_i))) { best = od; best_i = oi; }
  }
  return best_i == kNone ? -1 : best_i;
}

// SparseImgAlign::run(ref_keyframe, new_frame_) on keyframe row ref_kf of the stream's tables: T_ref = kf_T[ref_kf], the keyframe's point
// features in list order that hold a landmark which is not TYPE_DELETED and has an observation in this keyframe (the first one: its px and
// its STORED bearing, (*it)->f at src/sparse_img_align.cpp:229-230), all its segment features (a dead one: zeros), the initial model
// T_init * T_ref^-1 (:80).  ref_kf == kAlignRefClosest: the wave picks the row first; none close: kAlignJobNoKeyframe, an empty job whose
// reference pose is T_init (:413-417).
__global__ __launch_bounds__(64 * kAjWaves) void map_align_kf_job_kernel(const AlignKfBatchDev k) {
  const AlignBuildBatchDev& b = k.a;
  const CandBatchDev& c = b.s.c;
  const int lane = threadIdx.x & 63;
  const int job = blockIdx.x * kAjWaves + (int)(threadIdx.x >> 6);
  if (job >= c.n_jobs) return;                      // whole waves leave: nothing below synchronises across waves
  const AlignKfJobDev& J = k.jobs[job];
  if (!J.active) return;
  const CandMapDev& M = c.maps[job];
  const kf_u64 below = ((kf_u64)1 << lane) - 1;
  const KsView V = ks_view(c, M);
  const double* kf_T = c.kf_T + 7 * M.kf_off;
  // -- the reference keyframe
  int ref_kf = J.ref_kf;
  if (ref_kf == kAlignRefClosest) {
    CamDev cam; cam.fx = c.fx; cam.fy = c.fy; cam.cx = c.cx; cam.cy = c.cy; cam.width = c.cam_width; cam.height = c.cam_height;
    ref_kf = aj_closest_keyframe(V, k.keypts + 5 * M.kf_off, kf_T, M.n_kf, se3_load(J.d_T_last ? J.d_T_last : J.T_last), cam, J.self_kf);
  }
  if (ref_kf >= M.n_kf) ref_kf = -1;                // (the host's mirror has refused such a row)
  const bool have_kf = ref_kf >= 0;
  // -- poses: the initial model T_init * T_ref^-1; without a keyframe the reference pose is T_init
  const SE3d T_init = se3_load((J.init_source == kAlignInitKeyframe && have_kf) ? kf_T + 7 * ref_kf : J.init_source == kAlignInitDev ? J.d_T_init : J.T_init);
  const SE3d T_ref = have_kf ? se3_load(kf_T + 7 * ref_kf) : T_init;
  const SE3d T_inv = se3_inv(T_ref);
  const SE3d T0 = se3_mul(T_init, T_inv);
  const double ref_pos[3] = { T_inv.t[0], T_inv.t[1], T_inv.t[2] };
  AjLayout L;
#pragma unroll
  for (int l = 0; l < PLSVO_MAX_LEVELS; ++l) L.n_slots[l] = 0;
  L.long_mask = 0; L.patches = 0; L.finest = 0; L.fits = true;
  if (!have_kf) {
    if (lane == 0) aj_write_record(b, job, T0, T_ref, J.cur_slot, J.cur_slot, L, 0, 0, 0, kAlignJobNoKeyframe, 0);
    return;
  }
  // -- the keyframe's features and their observations in it
  const int p0 = V.kf_off[ref_kf], n_ftr_pt = V.kf_off[ref_kf + 1] - p0;
  const int* kf_seg_off = c.kf_seg_off + M.kf_off + M.stream; const int* kf_seg_lm = c.kf_seg_lm + M.kfseg_off;
  const int s0 = kf_seg_off[ref_kf], n_seg = kf_seg_off[ref_kf + 1] - s0;
  const int* pt_type = c.pt_type + M.pt_off; const int* seg_type = c.seg_type + M.seg_off;
  const double* pt_obs_f = c.pt_obs_f + 3 * M.ptobs_off;
  const int* seg_obs_off = c.seg_obs_off + M.seg_off + M.stream; const int* seg_obs_kf = c.seg_obs_kf + M.segobs_off;
  const double* seg_obs_spx = c.seg_obs_spx + 2 * M.segobs_off; const double* seg_obs_epx = c.seg_obs_epx + 2 * M.segobs_off;
  const double* seg_obs_sf = c.seg_obs_sf + 3 * M.segobs_off; const double* seg_obs_ef = c.seg_obs_ef + 3 * M.segobs_off;
  const double* seg_spos = c.seg_spos + 3 * M.seg_off; const double* seg_epos = c.seg_epos + 3 * M.seg_off;
  int n_pts = 0, n_seg_alive = 0;
  for (int base = 0; base < n_ftr_pt; base += 64) {
    const int i = base + lane;
    const int lm = i < n_ftr_pt ? V.kf_lm[p0 + i] : -1;
    n_pts += __popcll(__ballot(lm >= 0 && pt_type[lm] != PLSVO_LM_DELETED && aj_obs_in_kf(V.obs_off, V.obs_kf, lm, ref_kf) >= 0));
  }
  // (a keyframe of more segment features than the stream's rows is dropped before the scratch row is touched)
  int* const seg_obs = k.seg_obs + (size_t)job * (size_t)b.cap_seg;
  const bool seg_room = n_seg <= b.cap_seg;
  for (int base = 0; base < n_seg; base += 64) {
    const int s = base + lane;
    const int lm = s < n_seg ? kf_seg_lm[s0 + s] : -1;
    const int o = (lm >= 0 && seg_type[lm] != PLSVO_LM_DELETED) ? aj_obs_in_kf(seg_obs_off, seg_obs_kf, lm, ref_kf) : -1;
    if (seg_room && s < n_seg) seg_obs[s] = o;
    n_seg_alive += __popcll(__ballot(o >= 0));
  }
  cand_wave_sync();                                 // the observation indices, read back by other lanes
  // -- the slot layout of every level
  const AjKfSegs segs = { seg_obs, seg_obs_spx, seg_obs_epx };
  L = aj_layout_levels(b, segs, job, n_seg, n_pts, n_pts <= b.cap_pts && seg_room);
  const bool fits = L.fits;
  const size_t P0 = (size_t)job * (size_t)b.cap_pts, S0 = (size_t)job * (size_t)b.cap_seg;
  if (fits) {
    // -- points: the kept ones closed up stably
    int at0 = 0;
    for (int base = 0; base < n_ftr_pt; base += 64) {
      const int i = base + lane;
      const int lm = i < n_ftr_pt ? V.kf_lm[p0 + i] : -1;
      const int o = (lm >= 0 && pt_type[lm] != PLSVO_LM_DELETED) ? aj_obs_in_kf(V.obs_off, V.obs_kf, lm, ref_kf) : -1;
      const kf_u64 mask = __ballot(o >= 0);
      if (o >= 0) {
        const size_t at = P0 + (size_t)(at0 + __popcll(mask & below));
        const double d = aj_dist(V.pt_pos + 3 * lm, ref_pos);
        b.pt_px[2 * at] = V.obs_px[2 * o]; b.pt_px[2 * at + 1] = V.obs_px[2 * o + 1];
        b.pt_xyz[3 * at] = pt_obs_f[3 * o] * d; b.pt_xyz[3 * at + 1] = pt_obs_f[3 * o + 1] * d; b.pt_xyz[3 * at + 2] = pt_obs_f[3 * o + 2] * d;
      }
      at0 += __popcll(mask);
    }
    // -- segments: ALL of them, so that indices stay stable.  PINNED: a dead one has no pixels in the tables: zeros for pixels, length and vectors
    for (int s = lane; s < n_seg; s += 64) {
      const int o = seg_obs[s];
      double px4[4] = { 0.0, 0.0, 0.0, 0.0 }, p[3] = { 0.0, 0.0, 0.0 }, q[3] = { 0.0, 0.0, 0.0 }, len = 0.0;
      if (o >= 0) {
        const int lm = kf_seg_lm[s0 + s];
        (void)segs.px4(s, px4);
        len = aj_seg_len(px4);
        const double ds = aj_dist(seg_spos + 3 * lm, ref_pos), de = aj_dist(seg_epos + 3 * lm, ref_pos);
#pragma unroll
        for (int e = 0; e < 3; ++e) { p[e] = seg_obs_sf[3 * o + e] * ds; q[e] = seg_obs_ef[3 * o + e] * de; }
      }
      const size_t at = S0 + (size_t)s;
      b.seg_spx[2 * at] = px4[0]; b.seg_spx[2 * at + 1] = px4[1]; b.seg_epx[2 * at] = px4[2]; b.seg_epx[2 * at + 1] = px4[3];
      b.seg_len[at] = len;
#pragma unroll
      for (int e = 0; e < 3; ++e) { b.seg_p[3 * at + e] = p[e]; b.seg_q[3 * at + e] = q[e]; }
      b.seg_alive_in[at] = o >= 0 ? 1 : 0;
    }
  }
  if (lane == 0) aj_write_record(b, job, T0, T_ref, c.frame_slot[M.f_off + ref_kf], J.cur_slot, L, n_pts, n_seg, n_seg_alive, fits ? kAlignJobOk : kAlignJobNoRoom, ref_kf + 1);
}

// a lane per stream
__global__ __launch_bounds__(64) void map_align_pose_kernel(const AlignPoseBatchDev b) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= b.n_jobs) return;
  se3_store(se3_mul(se3_load(b.align_poses + 7 * j), se3_load(b.T_ref + 7 * j)), b.out + 7 * j);   // cur_frame->T_f_w_ = T_cur_from_ref * ref_frame->T_f_w_
}

// The tracking gates of FrameHandlerMono::processFrame behind the pose optimisation, a lane per stream:
//   "not enough matched features" (src/frame_handler_mono.cpp:315-321), fewer than 10 edges (:335), and
//   FrameHandlerBase::setTrackingQuality (src/frame_handler_base.cpp:173-190) literally -- the segments' drop is computed and reported
//   and decides nothing.  :346-350 cannot be reached (TRACKING_INSUFFICIENT is never set by setTrackingQuality) and is not built.
// The pose carried forward: under kGateTrack the first failure resets it to last_frame_'s (:318) and the second leaves the optimised one
// (:336); under kGateReloc every failure gives the last well localised pose (:432).  finishFrameProcessingCommon's num_obs_last_pt / _ls
// (src/frame_handler_base.cpp:131-133) are Frame::nObs() at every call site, the frame's feature counts, whatever the result.
__global__ __launch_bounds__(64) void map_track_gate_kernel(const TrackGateBatchDev b) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= b.n_jobs) return;
  const TrackGateJobDev& J = b.jobs[j];
  if (!J.active) return;
  const int n_pt = b.scalars[3 * j], n_ls = b.scalars[3 * j + 1];
  const int obs_pt = (int)b.state[j].num_obs_pt, obs_ls = (int)b.state[j].num_obs_ls;
  const int last_pt = J.last_resident ? b.obs_last[2 * j] : J.num_obs_last_pt, last_ls = J.last_resident ? b.obs_last[2 * j + 1] : J.num_obs_last_ls;
  const int n_matched = n_pt + n_ls, n_edges = obs_pt + obs_ls;
  const int result = n_matched < J.quality_min_fts ? kGateFailMatches : n_edges < 10 ? kGateFailEdges : kGateOk;
  const int drop_pt = (last_pt < J.max_fts ? last_pt : J.max_fts) - obs_pt, drop_ls = (last_ls < J.max_fts_segs ? last_ls : J.max_fts_segs) - obs_ls;
  int quality = kTrackGood;
  if (n_edges < J.quality_min_fts) quality = kTrackBad;
  if (drop_pt > J.quality_max_drop_fts) quality = kTrackBad;
  if (result != kGateOk) quality = kTrackInsufficient;
  const bool reset = result == kGateFailMatches || (result == kGateFailEdges && J.mode == kGateReloc);
  const double* T = reset ? (J.d_T_reset ? J.d_T_reset : J.T_reset) : b.poses + 7 * j;
#pragma unroll
  for (int k = 0; k < 7; ++k) b.carried[7 * j + k] = T[k];
  TrackGateOutDev& O = b.out[j];
  O.result = result; O.quality = quality; O.n_matched = n_matched; O.n_edges = n_edges; O.drop_pt = drop_pt; O.drop_ls = drop_ls;
  O.num_obs_last_pt = last_pt; O.num_obs_last_ls = last_ls;
  b.obs_last[2 * j] = n_pt; b.obs_last[2 * j + 1] = n_ls;
}

}  // namespace plsvo_hip
