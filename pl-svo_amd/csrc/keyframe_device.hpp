// keyframe_device.hpp -- the keyframe stage of FrameHandlerMono::processFrame on gfx950: one WAVE per stream, four waves per workgroup,
// no host round trip inside a call.  Included by seeds_kernels.hip (compiled with -ffp-contract=off: everything but the two
// transcendental calls of the logarithm is bit-identical to tests/np_keyframe.py).
//
//   close_keyframes_kernel    Map::getCloseKeyframes (src/map.cpp:158-179) with Frame::isVisible (src/frame.cpp:156-165), then the sort
//                             and the cut to max_n_kfs of Reprojector::reprojectMap (src/reprojector.cpp:147-163)
//   keyframe_decide_kernel    frame_utils::getSceneDepth (src/frame.cpp:182-217), FrameHandlerMono::needNewKf
//                             (src/frame_handler_mono.cpp:475-499), Frame::setKeyPoints / checkKeyPoints (src/frame.cpp:87-141),
//                             Map::getFurthestKeyframe (src/map.cpp:201-214)
//   [ext] Sophus SE3::log / SO3::logAndTheta, restated from upstream; vk::getMedian = the element of rank m/2
//
// The sequential loops of the reference become order statistics and arg-reductions over (value, rank):
//   * the sorted close list: a keyframe's place is the number of close keyframes with a smaller (distance, index);
//   * the median depth: exact select of rank m/2 over order-preserving 64-bit keys of the signed depths -- histogram passes of eight bits
//     from the highest bit in which minimum and maximum differ, finished by rank once the bin of rank k holds at most 64 keys
//     (poseopt_select.hpp's route on 64 lanes; nothing is sorted);
//   * a key point slot: the holder that survived ranks before every point, then the lowest index wins among equal values, which is
//     what a loop of strict comparisons in list order leaves behind.
#pragma once
#include <hip/hip_runtime.h>

#include <float.h>

#include "match_device.hpp"
#include "plsvo_wave.hpp"

namespace plsvo_hip {

#pragma clang fp contract(off)

constexpr int kKfWaves = 4;                       // streams per workgroup
typedef unsigned long long kf_u64;
constexpr kf_u64 kKfOnes = ~(kf_u64)0;

// ---- reductions over the 64 lanes of a wave, result in every lane ------------------------------------------------------------------------
__device__ __forceinline__ int kf_wave_sum(int v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ int kf_wave_scan_incl(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(v, d, 64); if (lane >= d) v += t; }
  return v;
}
__device__ __forceinline__ kf_u64 kf_shfl_xor_u64(kf_u64 v, int m) {
  const int lo = __shfl_xor((int)(uint32_t)v, m, 64), hi = __shfl_xor((int)(uint32_t)(v >> 32), m, 64);
  return ((kf_u64)(uint32_t)hi << 32) | (kf_u64)(uint32_t)lo;
}
__device__ __forceinline__ kf_u64 kf_wave_min(kf_u64 v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) { const kf_u64 o = kf_shfl_xor_u64(v, m); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ kf_u64 kf_wave_max(kf_u64 v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) { const kf_u64 o = kf_shfl_xor_u64(v, m); v = o > v ? o : v; }
  return v;
}
__device__ __forceinline__ kf_u64 kf_wave_or(kf_u64 v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v |= kf_shfl_xor_u64(v, m);
  return v;
}

// order-preserving key of a double: a < b (as numbers, -0.0 before +0.0) <=> key(a) < key(b) (as unsigned)
__device__ __forceinline__ kf_u64 kf_key(double z) {
  const kf_u64 b = (kf_u64)__double_as_longlong(z);
  return (b >> 63) ? ~b : (b | ((kf_u64)1 << 63));
}
__device__ __forceinline__ double kf_unkey(kf_u64 k) {
  const kf_u64 b = (k >> 63) ? (k & ~((kf_u64)1 << 63)) : ~k;
  return __longlong_as_double((long long)b);
}

// The k-th smallest (0-based) of keys[0 .. n) by one wave.  mn / mx: minimum and maximum of the keys that count (keys above mx -- the
// all-ones marks of dead features -- sort behind every rank asked for); 0 <= k < number of counting keys.  hist: 256 words, cand: 64 keys,
// ctr: one word, all of this wave's LDS.  Control flow is wave-uniform.
__device__ __forceinline__ kf_u64 kf_wave_select(const kf_u64* keys, int n, int k, kf_u64 mn, kf_u64 mx, int* hist, kf_u64* cand, int* ctr) {
  const int lane = threadIdx.x & 63;
  if (mn == mx) return mn;
  const kf_u64 diff = mn ^ mx;
  const int hb = 63 - __builtin_clzll(diff);
  kf_u64 mask = hb >= 63 ? (kf_u64)0 : (kKfOnes << (hb + 1));
  kf_u64 prefix = mn & mask;
  int shift = hb >= 7 ? hb - 7 : 0;
  for (;;) {
#pragma unroll
    for (int j = 0; j < 4; ++j) hist[lane * 4 + j] = 0;
    if (lane == 0) *ctr = 0;
    wave_lds_fence();
    for (int i = lane; i < n; i += 64) {
      const kf_u64 v = keys[i];
      if ((v & mask) == prefix) atomicAdd(&hist[(int)(((v & ~mask) >> shift) & (kf_u64)255)], 1);
    }
    wave_lds_fence();
    int loc[4], local = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { loc[j] = hist[lane * 4 + j]; local += loc[j]; }
    int cum = kf_wave_scan_incl(local) - local;
    int bin = 0, cnt = 0, kk = 0;   // non-zero in the lane that owns the bin of rank k only
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (k >= cum && k < cum + loc[j]) { bin = lane * 4 + j; cnt = loc[j]; kk = k - cum; }
      cum += loc[j];
    }
    bin = kf_wave_sum(bin); cnt = kf_wave_sum(cnt); k = kf_wave_sum(kk);
    prefix |= (kf_u64)(unsigned)bin << shift;
    mask |= (kf_u64)255 << shift;
    if (shift == 0) return prefix;                  // every bit is decided
    if (cnt <= 64) {
      // at most 64 keys are left: one per lane through LDS (in any order), every lane counts the keys below / not above its own, and
      // a lane with less <= k < leq holds the answer (equal keys: several lanes, the same pattern)
      for (int i = lane; i < n; i += 64) {
        const kf_u64 v = keys[i];
        if ((v & mask) == prefix) { const int at = atomicAdd(ctr, 1); if (at < 64) cand[at] = v; }
      }
      wave_lds_fence();
      const bool holds = lane < cnt;
      const kf_u64 me = holds ? cand[lane] : kKfOnes;
      int less = 0, leq = 0;
      for (int j = 0; j < cnt; ++j) { const kf_u64 o = cand[j]; less += o < me ? 1 : 0; leq += o <= me ? 1 : 0; }
      const kf_u64 r = kf_wave_or((holds && less <= k && k < leq) ? me : (kf_u64)0);
      wave_lds_fence();
      return r;
    }
    shift = shift >= 8 ? shift - 8 : 0;             // heavy duplicates or a crowded bin: another digit
  }
}

// ---- close keyframes ---------------------------------------------------------------------------------------------------------------------
// The arithmetic of Map::getCloseKeyframes, shared by close_keyframes_kernel (host arrays) and keystage_device.hpp's map_close_kernel
// (the resident tables).  Frame::isVisible for one world position:
__device__ __forceinline__ bool kf_visible(const SE3d& T, const CamDev& cam, const double* xyz_w) {
  double c[3], px[2];
  se3_act(T, xyz_w, c);
  if (c[2] < 0.0) return false;                     // behind the camera
  world2cam(cam, c, px);
  return px[0] >= 0.0 && px[1] >= 0.0 && px[0] < cam.width && px[1] < cam.height;
}
// (frame->T_f_w_.translation() - kf->T_f_w_.translation()).norm(), Eigen's norm()
__device__ __forceinline__ double kf_translation_dist(const SE3d& T, const double* kf_T) {
  const double dx = T.t[0] - kf_T[4], dy = T.t[1] - kf_T[5], dz = T.t[2] - kf_T[6];
  return sqrt((dx * dx + dy * dy) + dz * dz);
}
// the place of a close keyframe = close keyframes with a smaller (distance, index), over ALL rounds; scatter.  tmp: per keyframe its
// distance, -1 = not close, complete and fenced
__device__ __forceinline__ void kf_rank_scatter(const double* tmp, int n_kf, int* oidx, double* odist) {
  const int lane = threadIdx.x & 63;
  for (int i = lane; i < n_kf; i += 64) {
    const double d = tmp[i];
    if (d < 0.0) continue;
    int rank = 0;
    for (int j = 0; j < n_kf; ++j) { const double o = tmp[j]; rank += (o >= 0.0 && (o < d || (o == d && j < i))) ? 1 : 0; }
    oidx[rank] = i; odist[rank] = d;
  }
}

__global__ __launch_bounds__(64 * kKfWaves) void close_keyframes_kernel(const CloseKfBatchDev b) {
  const int lane = threadIdx.x & 63;
  const int job = blockIdx.x * kKfWaves + (int)(threadIdx.x >> 6);
  if (job >= b.n_jobs) return;                      // whole waves leave: nothing below synchronises across waves
  const CloseKfJobDev& J = b.jobs[job];
  const SE3d T = se3_load(J.T);
  CamDev cam; cam.fx = J.fx; cam.fy = J.fy; cam.cx = J.cx; cam.cy = J.cy; cam.width = J.width; cam.height = J.height;
  const int n_kf = J.n_kf;
  const double* kf_T = b.kf_T + 7 * J.kf_off;
  const double* kp = b.keypt_pos + 15 * J.kf_off;
  const uint8_t* kv = b.keypt_valid + 5 * J.kf_off;
  double* tmp = b.tmp_dist + J.kf_off;
  int n_close = 0;
  // pass 1, one lane per keyframe in rounds of 64: visible key point?  the distance of the two translations
  for (int base = 0; base < n_kf; base += 64) {
    const int i = base + lane;
    bool close = false;
    if (i < n_kf) {
      for (int k = 0; k < 5 && !close; ++k) {
        if (!kv[5 * i + k]) continue;
        close = kf_visible(T, cam, kp + 15 * i + 3 * k);
      }
      tmp[i] = close ? kf_translation_dist(T, kf_T + 7 * i) : -1.0;
    }
    n_close += __popcll(__ballot(close));
  }
  wave_lds_fence();                                 // the wave's own stores to tmp, read back by all of its lanes
  kf_rank_scatter(tmp, n_kf, b.close_idx + J.kf_off, b.close_dist + J.kf_off);   // pass 2
  if (lane == 0) { b.counts[2 * job] = n_close; b.counts[2 * job + 1] = n_close < J.max_n_kfs ? n_close : J.max_n_kfs; }
}

// ---- Sophus SE3::log -----------------------------------------------------------------------------------------------------------------------
// SO3::logAndTheta on the unit quaternion, then upsilon = V^-1 * translation with V^-1 = I - Omega/2 + c * Omega^2; SMALL_EPS = 1e-10.
// theta carries the sign of w (atan(n / w)), and the small-angle test is on the signed value, as upstream.
__device__ __forceinline__ void se3_log_dev(const SE3d& T, double* xi) {
  const double n = sqrt((T.q.x * T.q.x + T.q.y * T.q.y) + T.q.z * T.q.z);
  const double w = T.q.w, squared_w = w * w;
  double f;
  if (n < 1e-10) f = 2.0 / w - 2.0 * (n * n) / (w * squared_w);
  else if (fabs(w) < 1e-10) f = (w > 0.0 ? 3.14159265358979323846 : -3.14159265358979323846) / n;
  else f = 2.0 * atan(n / w) / n;
  const double theta = f * n;
  const double ox = f * T.q.x, oy = f * T.q.y, oz = f * T.q.z;
  double c;
  if (theta < 1e-10) c = 1.0 / 12.0;
  else c = (1.0 - theta / (2.0 * tan(theta / 2.0))) / (theta * theta);
  const double O2_00 = -(oy * oy + oz * oz), O2_11 = -(ox * ox + oz * oz), O2_22 = -(ox * ox + oy * oy);
  const double O2_01 = ox * oy, O2_02 = ox * oz, O2_12 = oy * oz;
  double V[9];
  V[0] = 1.0 + c * O2_00;         V[1] = 0.5 * oz + c * O2_01;    V[2] = -0.5 * oy + c * O2_02;
  V[3] = -0.5 * oz + c * O2_01;   V[4] = 1.0 + c * O2_11;         V[5] = 0.5 * ox + c * O2_12;
  V[6] = 0.5 * oy + c * O2_02;    V[7] = -0.5 * ox + c * O2_12;   V[8] = 1.0 + c * O2_22;
  for (int i = 0; i < 3; ++i) xi[i] = (V[3 * i] * T.t[0] + V[3 * i + 1] * T.t[1]) + V[3 * i + 2] * T.t[2];
  xi[3] = ox; xi[4] = oy; xi[5] = oz;
}

// ---- scene depth, new-keyframe test, key points, furthest keyframe ------------------------------------------------------------------------
constexpr int kKfNone = 0x7fffffff;               // rank of "no candidate" in a key point slot
// a slot's candidate: the larger value wins, then the lower rank
__device__ __forceinline__ void kf_slot_offer(double& val, int& rank, double oval, int orank) {
  if (orank != kKfNone && (rank == kKfNone || oval > val || (oval == val && orank < rank))) { val = oval; rank = orank; }
}
// the five values of checkKeyPoints for a point: slot 0 prefers the SMALLER max(|x - cu|, |y - cv|) (offered negated); slots 1..4 the
// larger (x - cu) * (y - cv) among the points that pass the slot's test -- the last two compare x with cv, as the reference does
__device__ __forceinline__ void kf_point_values(double x, double y, int cu, int cv, double* val, bool* pass) {
  const double ax = fabs(x - cu), ay = fabs(y - cv);
  val[0] = -(ax < ay ? ay : ax); pass[0] = true;
  const double prod = (x - cu) * (y - cv);
  val[1] = val[2] = val[3] = val[4] = prod;
  pass[1] = x >= cu && y >= cv;
  pass[2] = x >= cu && y < cv;
  pass[3] = x < cv && y < cv;
  pass[4] = x < cv && y >= cv;
}

// the five slots' candidates of all lanes, reduced: every lane ends with the wave's winner per slot
__device__ __forceinline__ void kf_slots_reduce(double* val, int* rank) {
#pragma unroll
  for (int s = 0; s < 5; ++s) {
#pragma unroll
    for (int mk = 1; mk < 64; mk <<= 1) {
      const double ov = __shfl_xor(val[s], mk, 64); const int orank = __shfl_xor(rank[s], mk, 64);
      kf_slot_offer(val[s], rank[s], ov, orank);
    }
  }
}

// The four parts of the decision, shared by keyframe_decide_kernel (host arrays) and keystage_device.hpp's map_keyframe_decide_kernel (the
// resident selection).  A position source maps a feature index to three doubles: the arrays of a call, or the landmark tables through
// the selection's landmark indices.
struct KfPosDirect {
  const double* p;
  __device__ __forceinline__ const double* operator()(int i) const { return p + 3 * i; }
};
struct KfPosIndexed {
  const double* p; const int* lm;
  __device__ __forceinline__ const double* operator()(int i) const { return p + 3 * lm[i]; }
};

// getSceneDepth: the keys of all depths into the stream's row (n_pt points, then two per segment), minimum and maximum on the way; the
// median is the element of rank m / 2.  Returns m, the depths that count.  hist / cand / ctr: this wave's LDS (kf_wave_select).
template <typename PtPos, typename SegPos>
__device__ __forceinline__ int kf_scene_depth(const SE3d& Tn, int n_pt, const uint8_t* pt_alive, const PtPos pt_pos, int n_seg, const uint8_t* seg_alive,
                                              const SegPos seg_spos, const SegPos seg_epos, kf_u64* keys, int* hist, kf_u64* cand, int* ctr,
                                              double* depth_mean, double* depth_min) {
  const int lane = threadIdx.x & 63;
  kf_u64 mn = kKfOnes, mx = 0;
  int m = 0;
  for (int i = lane; i < n_pt; i += 64) {
    kf_u64 key = kKfOnes;
    if (pt_alive[i]) {
      double c[3];
      se3_act(Tn, pt_pos(i), c);
      key = kf_key(c[2]); mn = key < mn ? key : mn; mx = key > mx ? key : mx; ++m;
    }
    keys[i] = key;
  }
  for (int s = lane; s < n_seg; s += 64) {
    kf_u64 ks = kKfOnes, ke = kKfOnes;
    if (seg_alive[s]) {
      double c[3];
      se3_act(Tn, seg_spos(s), c); ks = kf_key(c[2]);
      se3_act(Tn, seg_epos(s), c); ke = kf_key(c[2]);
      const kf_u64 lo = ks < ke ? ks : ke, hi = ks < ke ? ke : ks;
      mn = lo < mn ? lo : mn; mx = hi > mx ? hi : mx; m += 2;
    }
    keys[n_pt + 2 * s] = ks; keys[n_pt + 2 * s + 1] = ke;
  }
  m = kf_wave_sum(m); mn = kf_wave_min(mn); mx = kf_wave_max(mx);
  wave_lds_fence();                                 // the wave's own stores to keys, read back by all of its lanes
  *depth_mean = 0.0; *depth_min = DBL_MAX;
  if (m > 0) {
    *depth_mean = kf_unkey(kf_wave_select(keys, n_pt + 2 * n_seg, m / 2, mn, mx, hist, cand, ctr));
    *depth_min = kf_unkey(mn);
  }
  return m;
}

// setKeyPoints over the alive points of a frame: five arg-max reductions over (value, rank); a surviving holder has rank -1
__device__ __forceinline__ void kf_set_key_points(const double* pt_px, const uint8_t* pt_alive, int n_pt, int cu, int cv, const int* key_prev, int* key_out) {
  const int lane = threadIdx.x & 63;
  double val[5]; int rank[5];
#pragma unroll
  for (int s = 0; s < 5; ++s) { val[s] = 0.0; rank[s] = kKfNone; }
  if (lane == 0) {
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      const int h = key_prev[s];
      if (h >= 0 && pt_alive[h]) {                  // (a holder is not tested against its slot's quadrant again)
        double v[5]; bool pass[5];
        kf_point_values(pt_px[2 * h], pt_px[2 * h + 1], cu, cv, v, pass);
        val[s] = v[s]; rank[s] = -1;
      }
    }
  }
  for (int i = lane; i < n_pt; i += 64) {
    if (!pt_alive[i]) continue;
    double v[5]; bool pass[5];
    kf_point_values(pt_px[2 * i], pt_px[2 * i + 1], cu, cv, v, pass);
#pragma unroll
    for (int s = 0; s < 5; ++s) if (pass[s]) kf_slot_offer(val[s], rank[s], v[s], i);
  }
  kf_slots_reduce(val, rank);
#pragma unroll
  for (int s = 0; s < 5; ++s) key_out[s] = rank[s] == kKfNone ? -1 : (rank[s] < 0 ? key_prev[s] : rank[s]);
}

// needNewKf: one lane per overlap keyframe, in rounds of 64; the first blocking keyframe decides (its place in the list, -1 = none),
// every delta is written
__device__ __forceinline__ int kf_need_new_kf(const SE3d& T_last, const double* kf_T, const int* ov, int n_ov, double min_t, double min_r, double* out_t, double* out_r) {
  const int lane = threadIdx.x & 63;
  const SE3d T_last_inv = se3_inv(T_last);
  int blocking = -1;
  for (int base = 0; base < n_ov; base += 64) {
    const int j = base + lane;
    bool blocks = false;
    if (j < n_ov) {
      const SE3d delta_T = se3_mul(T_last_inv, se3_load(kf_T + 7 * ov[j]));
      double xi[6];
      se3_log_dev(delta_T, xi);
      const double delta_t = sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]);
      const double delta_r = sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]) * 180.0 / 3.1416;
      out_t[j] = delta_t; out_r[j] = delta_r;
      blocks = delta_t < min_t && delta_r < min_r;
    }
    const kf_u64 mask = __ballot(blocks);
    if (blocking < 0 && mask) blocking = base + __builtin_ctzll(mask);
  }
  return blocking;
}

// getFurthestKeyframe(new_frame->pos()): arg-max of the camera-centre distance, strict > from 0.0, the lowest index among equals
__device__ __forceinline__ int kf_furthest_keyframe(const SE3d& Tn, const double* kf_T, int n_kf) {
  const int lane = threadIdx.x & 63;
  const SE3d Tn_inv = se3_inv(Tn);
  double far_d = 0.0; int far_i = -1;
  for (int i = lane; i < n_kf; i += 64) {
    const SE3d Ki = se3_inv(se3_load(kf_T + 7 * i));
    const double dx = Ki.t[0] - Tn_inv.t[0], dy = Ki.t[1] - Tn_inv.t[1], dz = Ki.t[2] - Tn_inv.t[2];
    const double d = sqrt((dx * dx + dy * dy) + dz * dz);
    if (d > far_d) { far_d = d; far_i = i; }
  }
#pragma unroll
  for (int mk = 1; mk < 64; mk <<= 1) {
    const double od = __shfl_xor(far_d, mk, 64); const int oi = __shfl_xor(far_i, mk, 64);
    if (oi >= 0 && (od > far_d || (od == far_d && (far_i < 0 || oi < far_i)))) { far_d = od; far_i = oi; }
  }
  return far_i;
}

__global__ __launch_bounds__(64 * kKfWaves) void keyframe_decide_kernel(const KfDecideBatchDev b) {
  __shared__ int s_hist[kKfWaves][256];
  __shared__ kf_u64 s_cand[kKfWaves][64];
  __shared__ int s_ctr[kKfWaves];
  const int lane = threadIdx.x & 63, wave = (int)(threadIdx.x >> 6);
  const int job = blockIdx.x * kKfWaves + wave;
  if (job >= b.n_jobs) return;                      // whole waves leave: nothing below synchronises across waves
  const KfDecideJobDev& J = b.jobs[job];
  const SE3d Tn = se3_load(J.d_T_new ? J.d_T_new : J.T_new);
  const double* kf_T = b.kf_T + 7 * J.kf_off;
  const uint8_t* pt_alive = b.pt_alive + J.pt_off;
  double depth_mean, depth_min;
  const KfPosDirect pp = { b.pt_pos + 3 * J.pt_off }, sp = { b.seg_spos + 3 * J.seg_off }, ep = { b.seg_epos + 3 * J.seg_off };
  const int m = kf_scene_depth(Tn, J.n_pt, pt_alive, pp, J.n_seg, b.seg_alive + J.seg_off, sp, ep, b.depth_keys + J.depth_off, s_hist[wave], s_cand[wave], &s_ctr[wave],
                               &depth_mean, &depth_min);
  int key[5];
  kf_set_key_points(b.pt_px + 2 * J.pt_off, pt_alive, J.n_pt, J.width / 2, J.height / 2, J.key_prev, key);
  const int blocking = kf_need_new_kf(se3_load(J.T_last), kf_T, b.overlap_idx + J.ov_off, J.n_ov, J.min_t, J.min_r, b.delta_t + J.ov_off, b.delta_r + J.ov_off);
  const int far_i = kf_furthest_keyframe(Tn, kf_T, J.n_kf);
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
