// keystage_device.hpp -- the keyframe stage on the RESIDENT map tables on gfx950: one WAVE per stream, four waves per workgroup,
// nothing synchronised across waves (the decision's median select has LDS rows of its wave's own).  Included by seeds_kernels.hip
// (compiled with -ffp-contract=off: every output is bit-identical to tests/np_keystage.py).  The arithmetic is keyframe_device.hpp's, called from here: kf_visible, kf_translation_dist, kf_rank_scatter,
// kf_point_values, kf_slot_offer, kf_slots_reduce.
//
//   map_keypts_kernel   Frame::key_pts_ of every keyframe as a table of positions in the keyframe's point-feature list:
//                       Frame::setKeyPoints / checkKeyPoints (src/frame.cpp:87-141) from five NULLs (Frame::setKeyframe), and what
//                       Frame::removeKeyPoint (:143-154) leaves behind when Map::safeDeletePoint (src/map.cpp:116-123) took a holder's
//                       landmark; the rows close up over a keyframe Map::safeDeleteFrame removed
//   map_keyframe_decide_kernel   getSceneDepth, needNewKf, setKeyPoints, getFurthestKeyframe (keyframe_device.hpp) on the resident selection
//   map_close_kernel    Map::getCloseKeyframes (src/map.cpp:158-179) on kf_T, the key-point table and the LIVE pt_pos of each key
//                       point's landmark, the sort and the cut of Reprojector::reprojectMap (src/reprojector.cpp:147-163); writes the
//                       run's overlap row and count where map_candidates_kernel reads them
//
// A feature's px is not a table of its own: it is the observation of the feature's landmark whose *_obs_kf is this keyframe (the
// insertion's precondition: it exists; the first one when a landmark is a feature of the keyframe twice).  A feature without such an
// observation is passed over.
//
// removeKeyPoint, batched: the device sees a launch's deletions at once.  A keyframe is rebuilt when one of its holders has lost its
// landmark; then every slot is the best of the surviving features, a surviving holder winning ties (rank -1 before every feature, the
// lowest position among equal features).  The reference rebuilds after every single deletion: the two differ only when two distinct
// features tie exactly in a slot's value after an intermediate promotion (include/plsvo_hip.h pins it).
#pragma once
#include <hip/hip_runtime.h>

#include "candidates_device.hpp"

namespace plsvo_hip {

#pragma clang fp contract(off)

constexpr int kKsWaves = kKfWaves;                // streams per workgroup

// one stream's point tables, advanced to its rows
struct KsView {
  const int* kf_off; const int* kf_lm;
  const int* obs_off; const int* obs_kf; const double* obs_px;
  const double* pt_pos;
};
__device__ __forceinline__ KsView ks_view(const CandBatchDev& c, const CandMapDev& M) {
  KsView V;
  V.kf_off = c.kf_pt_off + M.kf_off + M.stream; V.kf_lm = c.kf_pt_lm + M.kfpt_off;
  V.obs_off = c.pt_obs_off + M.pt_off + M.stream; V.obs_kf = c.pt_obs_kf + M.ptobs_off; V.obs_px = c.pt_obs_px + 2 * M.ptobs_off;
  V.pt_pos = c.pt_pos + 3 * M.pt_off;
  return V;
}
// ftr->px of the feature of keyframe kf that holds landmark lm; false: no observation of lm in kf
__device__ __forceinline__ bool ks_feature_px(const KsView& V, int kf, int lm, double* px) {
  for (int o = V.obs_off[lm]; o < V.obs_off[lm + 1]; ++o)
    if (V.obs_kf[o] == kf) { px[0] = V.obs_px[2 * o]; px[1] = V.obs_px[2 * o + 1]; return true; }
  return false;
}

__global__ __launch_bounds__(64 * kKsWaves) void map_keypts_kernel(const KeyStageBatchDev b) {
  const int lane = threadIdx.x & 63;
  const int job = blockIdx.x * kKsWaves + (int)(threadIdx.x >> 6);
  if (job >= b.c.n_jobs) return;                    // whole waves leave: nothing below synchronises across waves
  const KeyPtsJobDev& J = b.kp_jobs[job];
  if (J.mode == kKeyPtsStandBy) return;
  const CandMapDev& M = b.c.maps[job];
  const KsView V = ks_view(b.c, M);
  const int n_kf = M.n_kf;
  int* const kp = b.keypts + 5 * M.kf_off;
  // -- the rows above a removed keyframe close up; the table holds n_kf - 1 old rows afterwards, the new keyframe's is the last
  if (J.remove_kf >= 0) {
    for (int base = 5 * J.remove_kf; base < 5 * (n_kf - 1); base += 64) {
      const int e = base + lane;
      int v = -1;
      if (e < 5 * (n_kf - 1)) v = kp[e + 5];
      cand_wave_sync();                             // every lane's entry is in a register before the entries below it are overwritten
      if (e < 5 * (n_kf - 1)) kp[e] = v;
      cand_wave_sync();
    }
  }
  const int cu = b.c.cam_width / 2, cv = b.c.cam_height / 2;
  for (int i = 0; i < n_kf; ++i) {                  // (wave-uniform)
    const int f0 = V.kf_off[i], n_ftr = V.kf_off[i + 1] - f0;
    const bool is_new = J.new_row != kKeyPtsRowOld && i == n_kf - 1;   // the new keyframe: from five NULLs, or the run's decision (selection order = its feature list)
    const bool fresh = J.mode == kKeyPtsFresh || (is_new && J.new_row == kKeyPtsRowFresh);
    bool rebuild = fresh;
    int hold[5];
#pragma unroll
    for (int s = 0; s < 5; ++s) {                   // removeKeyPoint: a holder whose feature has lost its landmark
      int h = fresh ? -1 : (is_new ? b.decided[job].key_pts[s] : kp[5 * i + s]);
      if (h >= n_ftr) h = -1;
      if (h >= 0 && V.kf_lm[f0 + h] < 0) { h = -1; rebuild = true; }
      hold[s] = h;
    }
    if (!rebuild) {
      if (is_new && lane == 0) {
#pragma unroll
        for (int s = 0; s < 5; ++s) kp[5 * i + s] = hold[s];
      }
      continue;
    }
    // setKeyPoints: five arg-max reductions over (value, rank); a surviving holder has rank -1
    double val[5]; int rank[5];
#pragma unroll
    for (int s = 0; s < 5; ++s) { val[s] = 0.0; rank[s] = kKfNone; }
    if (lane == 0) {
#pragma unroll
      for (int s = 0; s < 5; ++s) {
        double px[2];
        if (hold[s] >= 0 && ks_feature_px(V, i, V.kf_lm[f0 + hold[s]], px)) {   // (a holder is not tested against its slot's quadrant again)
          double v[5]; bool pass[5];
          kf_point_values(px[0], px[1], cu, cv, v, pass);
          val[s] = v[s]; rank[s] = -1;
        }
      }
    }
    for (int j = lane; j < n_ftr; j += 64) {
      const int lm = V.kf_lm[f0 + j];
      double px[2];
      if (lm < 0 || !ks_feature_px(V, i, lm, px)) continue;
      double v[5]; bool pass[5];
      kf_point_values(px[0], px[1], cu, cv, v, pass);
#pragma unroll
      for (int s = 0; s < 5; ++s) if (pass[s]) kf_slot_offer(val[s], rank[s], v[s], j);
    }
    kf_slots_reduce(val, rank);
    if (lane == 0) {
#pragma unroll
      for (int s = 0; s < 5; ++s) kp[5 * i + s] = rank[s] == kKfNone ? -1 : (rank[s] < 0 ? hold[s] : rank[s]);
    }
  }
}

// Map::getCloseKeyframes (src/map.cpp:158-179), one keyframe row of the stream: is one of its key points' landmarks visible at its
// position NOW from the frame at T, and then the distance between the two (map_close_kernel; the closest keyframe of alignjob_device.hpp)
__device__ __forceinline__ bool ks_close(const KsView& V, const int* kp, const double* kf_T, const SE3d& T, const CamDev& cam, int i, double* dist) {
  const int f0 = V.kf_off[i], n_ftr = V.kf_off[i + 1] - f0;
  bool close = false;
  for (int k = 0; k < 5 && !close; ++k) {
    const int h = kp[5 * i + k];
    if (h < 0 || h >= n_ftr) continue;
    const int lm = V.kf_lm[f0 + h];
    if (lm < 0) continue;                           // (the upkeep leaves no such holder)
    close = kf_visible(T, cam, V.pt_pos + 3 * lm);
  }
  *dist = close ? kf_translation_dist(T, kf_T + 7 * i) : -1.0;
  return close;
}

__global__ __launch_bounds__(64 * kKsWaves) void map_close_kernel(const KeyStageBatchDev b) {
  const int lane = threadIdx.x & 63;
  const int job = blockIdx.x * kKsWaves + (int)(threadIdx.x >> 6);
  if (job >= b.c.n_jobs) return;                    // whole waves leave: nothing below synchronises across waves
  const CandMapDev& M = b.c.maps[job];
  CandJobDev& J = const_cast<CandJobDev&>(b.c.jobs[job]);
  const KsView V = ks_view(b.c, M);
  const SE3d T = se3_load(J.d_T ? J.d_T : J.T);
  CamDev cam; cam.fx = b.c.fx; cam.fy = b.c.fy; cam.cx = b.c.cx; cam.cy = b.c.cy; cam.width = b.c.cam_width; cam.height = b.c.cam_height;
  const int room = b.ov_room[job];
  const int n_kf = M.n_kf < room ? M.n_kf : room;   // (the host laid the overlap row out for its own count of the keyframes: the same)
  const double* kf_T = b.c.kf_T + 7 * M.kf_off;
  const int* kp = b.keypts + 5 * M.kf_off;
  double* tmp = b.tmp_dist + M.kf_off;
  int n_close = 0;
  // pass 1, one lane per keyframe in rounds of 64: a key point whose landmark is visible at its position NOW?
  for (int base = 0; base < n_kf; base += 64) {
    const int i = base + lane;
    bool close = false;
    if (i < n_kf) {
      double d;
      close = ks_close(V, kp, kf_T, T, cam, i, &d);
      tmp[i] = d;
    }
    n_close += __popcll(__ballot(close));
  }
  wave_lds_fence();                                 // the wave's own stores to tmp, read back by all of its lanes
  int* oidx = b.close_idx + M.kf_off;
  kf_rank_scatter(tmp, n_kf, oidx, b.close_dist + M.kf_off);   // pass 2
  cand_wave_sync();                                 // the sorted list, read back by other lanes
  // the cut: the run's overlap row and count; the counts per overlap keyframe behind the cut are zero
  const int n_ov = n_close < b.max_n_kfs ? n_close : b.max_n_kfs;
  int* ov = const_cast<int*>(b.c.overlap_idx) + J.ov_off;
  for (int r = lane; r < room; r += 64) {
    if (r < n_ov) ov[r] = oidx[r];
    else b.c.kf_count[J.ov_off + r] = 0;
  }
  if (lane == 0) { J.n_ov = n_ov; b.close_counts[2 * job] = n_close; b.close_counts[2 * job + 1] = n_ov; }
}

// FrameHandlerMono::processFrame between "pose optimised" and the keyframe decision on the resident selection: the arithmetic of
// keyframe_decide_kernel with key_pts_prev all NULL, every input read where it already lies -- the optimised pose, the selection's
// features with the pose optimiser's keep masks as alive, the landmark positions in the TABLES (optimizeStructure may have moved them
// since the selection gathered its copy), kf_T and the run's overlap row.  key_pts are indices in selection order.
__global__ __launch_bounds__(64 * kKsWaves) void map_keyframe_decide_kernel(const KeyDecideBatchDev b) {
  __shared__ int s_hist[kKsWaves][256];
  __shared__ kf_u64 s_cand[kKsWaves][64];
  __shared__ int s_ctr[kKsWaves];
  const CandBatchDev& c = b.s.c;
  const int lane = threadIdx.x & 63, wave = (int)(threadIdx.x >> 6);
  const int job = blockIdx.x * kKsWaves + wave;
  if (job >= c.n_jobs) return;                      // whole waves leave: nothing below synchronises across waves
  const KeyDecideJobDev& J = b.jobs[job];
  if (!J.active) return;
  const CandMapDev& M = c.maps[job];
  const CandJobDev& R = c.jobs[job];
  const SE3d Tn = se3_load(b.poses + 7 * job);
  const int n_pt = b.s.scalars[3 * job], n_seg = b.s.scalars[3 * job + 1];
  const double* kf_T = c.kf_T + 7 * M.kf_off;
  const uint8_t* pt_alive = b.pt_keep + M.opt_off;
  const KfPosIndexed pp = { c.pt_pos + 3 * M.pt_off, b.s.f_pt_lm + M.opt_off };
  const KfPosIndexed sp = { c.seg_spos + 3 * M.seg_off, b.s.f_seg_lm + 2 * M.oseg_off }, ep = { c.seg_epos + 3 * M.seg_off, b.s.f_seg_lm + 2 * M.oseg_off };
  double depth_mean, depth_min;
  const int m = kf_scene_depth(Tn, n_pt, pt_alive, pp, n_seg, b.seg_keep + 2 * M.oseg_off, sp, ep, b.depth_keys + (M.opt_off + 4 * M.oseg_off), s_hist[wave], s_cand[wave], &s_ctr[wave],
                               &depth_mean, &depth_min);
  const int none[5] = { -1, -1, -1, -1, -1 };
  int key[5];
  kf_set_key_points(b.s.f_pt_px + 2 * M.opt_off, pt_alive, n_pt, c.cam_width / 2, c.cam_height / 2, none, key);
  const int blocking = kf_need_new_kf(se3_load(J.d_T_last ? J.d_T_last : J.T_last), kf_T, c.overlap_idx + R.ov_off, R.n_ov, J.min_t, J.min_r,
                                      b.delta_t + R.ov_off, b.delta_r + R.ov_off);
  const int far_i = kf_furthest_keyframe(Tn, kf_T, M.n_kf);
  if (lane == 0) {
    KfDecideOutDev& o = b.out[job];
    o.depth_mean = depth_mean; o.depth_min = depth_min;
    o.has_depth = m > 0 ? 1 : 0; o.n_depth = m;
    o.need_new_kf = blocking < 0 ? 1 : 0; o.blocking = blocking;
#pragma unroll
    for (int s = 0; s < 5; ++s) o.key_pts[s] = key[s];
    o.furthest_kf = far_i;
  }
}

}  // namespace plsvo_hip
