// klt_device.hpp -- the bootstrap's pyramidal KLT tracker on gfx950: KltHomographyInit::addFirstFrame / addSecondFrame
// up to the disparity gate (src/initialization.cpp:40-69) and trackKlt (:170-215).  Included by seeds_kernels.hip only, beside
// keyframe_device.hpp, whose wave select it uses.  That unit is compiled with -ffp-contract=off: every float and double operation
// below is a single IEEE operation in the order written, and the results are bit-identical to tests/np_klt.py.
//   [ext] cv::calcOpticalFlowPyrLK (30 x 30 window, OPTFLOW_USE_INITIAL_FLOW), cv::buildOpticalFlowPyramid (pyrDown 5 x 5, Scharr
//   derivatives, image border reflect-101, derivative border 0), vk::getMedian, vk::PinholeCamera::cam2world: restated from upstream.
//
//   klt_pyrdown_kernel  one level of the KLT pyramid of every active stream: 4 output pixels per lane
//   klt_first_kernel    one workgroup per active stream: the first frame's lists from the detector's device records or a host list
//   klt_track_kernel    one WAVE per (stream, list entry), every level inside the launch.  Per level the 33 x 33 source window is staged in
//                       LDS, the 30 x 30 template (I, Ix, Iy as int16) is built from it with the Scharr derivatives computed on the fly --
//                       no derivative image exists -- and every iteration stages the 31 x 31 window of the current frame and makes 15 trips
//                       of 64 lanes over it.  All sums are exact integers: int32 per lane, int64 across the wave, converted to float once.
//                       The 2 x 2 solve and every exit are wave-uniform.
//   klt_commit_kernel   one wave per active stream: stable ballot / prefix compaction of the lists over status == 0, bearings,
//                       disparities, the exact median (kf_wave_select), the gates, the report
#pragma once
#include <hip/hip_runtime.h>

#include <float.h>

#include "keyframe_device.hpp"

namespace plsvo_hip {

#pragma clang fp contract(off)

constexpr int kKltArea = kKltWin * kKltWin;      // 900 template pixels
constexpr int kKltSrcN = kKltWin + 3;            // the template's source window: 31 x 31 bilinear taps and a ring of 1 for the derivatives
constexpr int kKltPitch = 36;                    // row pitch of the staged window in LDS
constexpr float kKltHalf = 14.5f;                // (win - 1) * 0.5f
constexpr float kKltScale = 9.5367431640625e-07f;   // FLT_SCALE = 1.f / (1 << 20)

// cv::borderInterpolate(i, n, BORDER_REFLECT_101)
__device__ __forceinline__ int klt_reflect(int i, int n) {
  if (n == 1) return 0;
  while ((unsigned)i >= (unsigned)n) i = i < 0 ? -i : 2 * n - 2 - i;
  return i;
}

__device__ __forceinline__ const uint8_t* klt_level(const KltBatchDev& b, int slot, int pyramid, int l) {
  return l == 0 ? b.pyr + (size_t)slot * b.slot_bytes + b.lv.off[0] : b.store + (size_t)pyramid * b.lv.pyr_bytes + b.lv.off[l];
}

// ---- pyrDown ------------------------------------------------------------------------------------------------------------------------------
// grid: (ceil(qw * oh / 256), rows), qw = ceil(ow / 4).  Level l of pyramid 2 * stream + which from level l - 1 (level 0: the slot's).
__global__ __launch_bounds__(256) void klt_pyrdown_kernel(KltBatchDev b, int l, int which) {
  const KltRowDev row = b.rows[blockIdx.y];
  const int sw = b.lv.w[l - 1], sh = b.lv.h[l - 1], ow = b.lv.w[l], oh = b.lv.h[l];
  const int qw = (ow + 3) >> 2;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= qw * oh) return;
  const int y = idx / qw, x0 = 4 * (idx - y * qw);
  const int pyramid = 2 * row.stream + which;
  const uint8_t* src = klt_level(b, which ? row.cur_slot : row.ref_slot, pyramid, l - 1);
  uint8_t* dst = b.store + (size_t)pyramid * b.lv.pyr_bytes + b.lv.off[l];
  const bool inner = 2 * x0 - 2 >= 0 && 2 * x0 + 8 < sw;
  int acc[4] = { 0, 0, 0, 0 };
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    const uint8_t* r = src + (size_t)klt_reflect(2 * y + dy, sh) * sw;
    int v[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) v[k] = r[inner ? 2 * x0 - 2 + k : klt_reflect(2 * x0 - 2 + k, sw)];
    const int ky = dy == 0 ? 6 : ((dy == -1 || dy == 1) ? 4 : 1);
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] += ky * (v[2 * k] + 4 * v[2 * k + 1] + 6 * v[2 * k + 2] + 4 * v[2 * k + 3] + v[2 * k + 4]);
  }
  uint8_t* o = dst + (size_t)y * ow + x0;
  uint32_t px[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) px[k] = (uint32_t)((acc[k] + 128) >> 8);
  if (x0 + 4 <= ow && (reinterpret_cast<uintptr_t>(o) & 3) == 0) *reinterpret_cast<uint32_t*>(o) = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
  else for (int k = 0; k < 4 && x0 + k < ow; ++k) o[k] = (uint8_t)px[k];
}

// ---- first frame ----------------------------------------------------------------------------------------------------------------------------
// unit bearing of a float pixel: sel_bearing's expressions (select_device.hpp) in double
__device__ __forceinline__ void klt_bearing(double fx, double fy, double cx, double cy, float pu, float pv, double* f) {
  const double x = ((double)pu - cx) / fx, y = ((double)pv - cy) / fy;
  const double n = sqrt((x * x + y * y) + 1.0);
  f[0] = x / n; f[1] = y / n; f[2] = 1.0 / n;
}

// grid: active streams.  detectFeatures' lists (:147-167) and addFirstFrame's gate and copy (:44-52)
__global__ __launch_bounds__(256) void klt_first_kernel(KltBatchDev b) {
  const KltFirstDev j = b.first[blockIdx.x];
  const int s = j.stream;
  long long nc = j.d_corners ? (long long)*j.d_count : (long long)j.n_host;
  if (nc < 0) nc = 0;
  const long long n = nc + j.n_extra;
  const int result = n > b.cap_pts ? PLSVO_KLT_DROPPED : (n < PLSVO_KLT_MIN_FIRST ? PLSVO_KLT_FAILURE : PLSVO_KLT_FIRST);
  const int kept = result == PLSVO_KLT_FIRST ? (int)n : 0;
  const size_t base = (size_t)s * b.cap_pts;
  for (int i = threadIdx.x; i < kept; i += blockDim.x) {
    float px[2];
    double f[3];
    if (i < nc) {
      if (j.d_corners) { px[0] = (float)j.d_corners[i].x; px[1] = (float)j.d_corners[i].y; }
      else { px[0] = b.host_px[2 * (j.host_at + i)]; px[1] = b.host_px[2 * (j.host_at + i) + 1]; }
      klt_bearing(j.fx, j.fy, j.cx, j.cy, px[0], px[1], f);
    } else {
      const long long e = j.extra_at + (i - nc);
      px[0] = b.extra_px[2 * e]; px[1] = b.extra_px[2 * e + 1];
      f[0] = b.extra_f[3 * e]; f[1] = b.extra_f[3 * e + 1]; f[2] = b.extra_f[3 * e + 2];
    }
    const size_t at = base + i;
    b.px_ref[2 * at] = px[0]; b.px_ref[2 * at + 1] = px[1];
    b.px_cur[2 * at] = px[0]; b.px_cur[2 * at + 1] = px[1];
    b.f_ref[3 * at] = f[0]; b.f_ref[3 * at + 1] = f[1]; b.f_ref[3 * at + 2] = f[2];
  }
  if (threadIdx.x == 0) {
    b.count[s] = kept;
    KltStreamDev st;
    st.fx = j.fx; st.fy = j.fy; st.cx = j.cx; st.cy = j.cy; st.started = result == PLSVO_KLT_FIRST ? 1 : 0; st.n_calls = 0;
    b.st[s] = st;
    plsvo_klt_report r;
    r.result = result; r.n_before = (int)(n > 0x7fffffffLL ? 0x7fffffffLL : n); r.n_after = kept; r.levels = b.lv.n_lv; r.median_disparity = 0.0;
    r.n_calls = 0; r.reserved0 = 0;
    b.report[s] = r;
  }
}

// ---- track --------------------------------------------------------------------------------------------------------------------------------
struct KltWeights { int w00, w01, w10, w11; };
// cvRound of the float products (round to nearest even), the last weight by difference: the four always sum to 1 << 14
__device__ __forceinline__ KltWeights klt_weights(float a, float bq) {
  KltWeights k;
  k.w00 = (int)rintf((1.f - a) * (1.f - bq) * 16384.f);
  k.w01 = (int)rintf(a * (1.f - bq) * 16384.f);
  k.w10 = (int)rintf((1.f - a) * bq * 16384.f);
  k.w11 = 16384 - k.w00 - k.w01 - k.w10;
  return k;
}
// the window test of calcOpticalFlowPyrLK on the floored position, in float: a position cvFloor cannot hold (huge, NaN) is outside
__device__ __forceinline__ bool klt_in_range(float fx, float fy, int W, int H) {
  return fx >= -(float)kKltWin && fx < (float)W && fy >= -(float)kKltWin && fy < (float)H;
}
__device__ __forceinline__ long long klt_wave_sum(long long v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const int lo = __shfl_xor((int)(uint32_t)v, m, 64), hi = __shfl_xor((int)(uint32_t)((unsigned long long)v >> 32), m, 64);
    v += (long long)(((unsigned long long)(uint32_t)hi << 32) | (unsigned long long)(uint32_t)lo);
  }
  return v;
}
// N x N pixels from (x0, y0) of a level into this wave's LDS window, reflect-101 outside the image
template <int N>
__device__ __forceinline__ void klt_stage(const uint8_t* img, int W, int H, int x0, int y0, uint8_t* win) {
  const int lane = threadIdx.x & 63;
  const bool inside = x0 >= 0 && y0 >= 0 && x0 + N <= W && y0 + N <= H;
  wave_lds_fence();
  for (int e = lane; e < N * N; e += 64) {
    const int r = e / N, c = e - r * N;
    int x = x0 + c, y = y0 + r;
    if (!inside) { x = klt_reflect(x, W); y = klt_reflect(y, H); }
    win[r * kKltPitch + c] = img[(size_t)y * W + x];
  }
  wave_lds_fence();
}

// grid: (ceil(max list length / kKltWaves), rows)
__global__ __launch_bounds__(kKltWaves * 64) void klt_track_kernel(KltBatchDev b) {
  __shared__ int16_t s_tpl[kKltWaves][3 * kKltArea];
  __shared__ __align__(4) uint8_t s_win[kKltWaves][kKltSrcN * kKltPitch];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const KltRowDev row = b.rows[blockIdx.y];
  const int s = row.stream;
  const int pt = blockIdx.x * kKltWaves + wave;
  if (pt >= b.count[s] || pt >= b.cap_pts) return;
  int16_t* tpl = s_tpl[wave];
  uint8_t* win = s_win[wave];
  const size_t at = (size_t)s * b.cap_pts + pt;
  const float prev_x = b.px_ref[2 * at], prev_y = b.px_ref[2 * at + 1];
  float nx = b.px_cur[2 * at], ny = b.px_cur[2 * at + 1];
  int status = 1;
  const int L = b.lv.n_lv - 1;
  for (int l = L; l >= 0; --l) {
    const int W = b.lv.w[l], H = b.lv.h[l];
    const float inv = 1.f / (float)(1 << l);
    const float plx = prev_x * inv - kKltHalf, ply = prev_y * inv - kKltHalf;
    if (l == L) { nx = nx * inv; ny = ny * inv; } else { nx = nx * 2.f; ny = ny * 2.f; }
    int code = PLSVO_KLT_EXIT_PREV_OOR, iters = 0;
    const float fpx = floorf(plx), fpy = floorf(ply);
    if (!klt_in_range(fpx, fpy, W, H)) {
      if (l == 0) status = 0;
    } else {
      const int ix = (int)fpx, iy = (int)fpy;
      const KltWeights wp = klt_weights(plx - fpx, ply - fpy);
      klt_stage<kKltSrcN>(klt_level(b, row.ref_slot, 2 * s, l), W, H, ix - 1, iy - 1, win);
      int a11 = 0, a12 = 0, a22 = 0;
      for (int p = lane; p < kKltArea; p += 64) {
        const int y = p / kKltWin, x = p - y * kKltWin;
        const uint8_t* q = win + y * kKltPitch + x;   // the 4 x 4 block whose inner 2 x 2 are the bilinear taps
        const int ival = q[kKltPitch + 1] * wp.w00 + q[kKltPitch + 2] * wp.w01 + q[2 * kKltPitch + 1] * wp.w10 + q[2 * kKltPitch + 2] * wp.w11;
        int dxv[4], dyv[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int dr = t >> 1, dc = t & 1;
          const uint8_t* c = q + dr * kKltPitch + dc;   // top-left of the tap's 3 x 3
          const bool in = (unsigned)(ix + x + dc) < (unsigned)W && (unsigned)(iy + y + dr) < (unsigned)H;
          const int c00 = c[0], c01 = c[1], c02 = c[2], c10 = c[kKltPitch], c12 = c[kKltPitch + 2];
          const int c20 = c[2 * kKltPitch], c21 = c[2 * kKltPitch + 1], c22 = c[2 * kKltPitch + 2];
          dxv[t] = in ? 3 * (c02 - c00) + 10 * (c12 - c10) + 3 * (c22 - c20) : 0;
          dyv[t] = in ? 3 * (c20 - c00) + 10 * (c21 - c01) + 3 * (c22 - c02) : 0;
        }
        const int I = (ival + 256) >> 9;
        const int Ix = (dxv[0] * wp.w00 + dxv[1] * wp.w01 + dxv[2] * wp.w10 + dxv[3] * wp.w11 + 8192) >> 14;
        const int Iy = (dyv[0] * wp.w00 + dyv[1] * wp.w01 + dyv[2] * wp.w10 + dyv[3] * wp.w11 + 8192) >> 14;
        tpl[p] = (int16_t)I; tpl[kKltArea + p] = (int16_t)Ix; tpl[2 * kKltArea + p] = (int16_t)Iy;
        a11 += Ix * Ix; a12 += Ix * Iy; a22 += Iy * Iy;
      }
      const float A11 = (float)klt_wave_sum((long long)a11) * kKltScale, A12 = (float)klt_wave_sum((long long)a12) * kKltScale;
      const float A22 = (float)klt_wave_sum((long long)a22) * kKltScale;
      float D = A11 * A22 - A12 * A12;
      const float dd = A11 - A22;
      const float min_eig = (A22 + A11 - __fsqrt_rn(dd * dd + 4.f * A12 * A12)) / 1800.f;
      if ((double)min_eig < b.min_eig || D < FLT_EPSILON) {
        code = PLSVO_KLT_EXIT_FLAT;
        if (l == 0) status = 0;
      } else {
        D = 1.f / D;
        const uint8_t* cur = klt_level(b, row.cur_slot, 2 * s + 1, l);
        float qx = nx - kKltHalf, qy = ny - kKltHalf;
        float pdx = 0.f, pdy = 0.f;
        code = PLSVO_KLT_EXIT_MAX_ITER; iters = b.max_iter;
        for (int j = 0; j < b.max_iter; ++j) {
          const float fqx = floorf(qx), fqy = floorf(qy);
          if (!klt_in_range(fqx, fqy, W, H)) {
            if (l == 0) status = 0;
            code = PLSVO_KLT_EXIT_ITER_OOR; iters = j;
            break;
          }
          const KltWeights wq = klt_weights(qx - fqx, qy - fqy);
          klt_stage<kKltWin + 1>(cur, W, H, (int)fqx, (int)fqy, win);
          int b1 = 0, b2 = 0;
          for (int p = lane; p < kKltArea; p += 64) {
            const int y = p / kKltWin, x = p - y * kKltWin;
            const uint8_t* q = win + y * kKltPitch + x;
            const int jval = (q[0] * wq.w00 + q[1] * wq.w01 + q[kKltPitch] * wq.w10 + q[kKltPitch + 1] * wq.w11 + 256) >> 9;
            const int diff = jval - (int)tpl[p];
            b1 += diff * (int)tpl[kKltArea + p]; b2 += diff * (int)tpl[2 * kKltArea + p];
          }
          const float fb1 = (float)klt_wave_sum((long long)b1) * kKltScale, fb2 = (float)klt_wave_sum((long long)b2) * kKltScale;
          const float dx = (A12 * fb2 - A22 * fb1) * D, dy = (A12 * fb1 - A11 * fb2) * D;
          qx += dx; qy += dy;
          nx = qx + kKltHalf; ny = qy + kKltHalf;
          if ((double)dx * (double)dx + (double)dy * (double)dy <= b.eps2) { code = PLSVO_KLT_EXIT_EPS; iters = j + 1; break; }
          if (j > 0 && fabs((double)(dx + pdx)) < 0.01 && fabs((double)(dy + pdy)) < 0.01) {
            nx -= dx * 0.5f; ny -= dy * 0.5f;
            code = PLSVO_KLT_EXIT_OSC; iters = j + 1;
            break;
          }
          pdx = dx; pdy = dy;
        }
      }
    }
    if (b.diag_exit && lane == 0) { b.diag_exit[(size_t)pt * kKltLevels + l] = (uint8_t)code; b.diag_iters[(size_t)pt * kKltLevels + l] = (uint8_t)iters; }
  }
  // the error output's range test behind level 0 (the error itself is not computed)
  if (status && !klt_in_range(floorf(nx - kKltHalf), floorf(ny - kKltHalf), b.lv.w[0], b.lv.h[0])) status = 0;
  if (lane == 0) { b.next[2 * at] = nx; b.next[2 * at + 1] = ny; b.status[at] = (uint8_t)status; }
}

// ---- lists, median, gates -----------------------------------------------------------------------------------------------------------------
// grid: ceil(rows / kKltWaves).  trackKlt's loop (:192-215) and addSecondFrame's gates (:62-69)
__global__ __launch_bounds__(kKltWaves * 64) void klt_commit_kernel(KltBatchDev b) {
  __shared__ int s_hist[kKltWaves][256];
  __shared__ kf_u64 s_cand[kKltWaves][64];
  __shared__ int s_ctr[kKltWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = blockIdx.x * kKltWaves + wave;
  if (r >= b.n_rows) return;
  const int s = b.rows[r].stream;
  const KltStreamDev st = b.st[s];
  plsvo_klt_report rep;
  rep.result = PLSVO_KLT_INACTIVE; rep.n_before = 0; rep.n_after = 0; rep.levels = b.lv.n_lv; rep.median_disparity = 0.0; rep.n_calls = 0; rep.reserved0 = 0;
  if (!st.started) { if (lane == 0) b.report[s] = rep; return; }
  const int n = b.count[s];
  const size_t base = (size_t)s * b.cap_pts;
  kf_u64* keys = b.keys + base;
  int out = 0;
  kf_u64 mn = kKfOnes, mx = 0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const bool keep = i < n && b.status[base + i] != 0;
    float pr[2] = { 0.f, 0.f }, pc[2] = { 0.f, 0.f };
    double fr[3] = { 0.0, 0.0, 0.0 };
    if (keep) {
      pr[0] = b.px_ref[2 * (base + i)]; pr[1] = b.px_ref[2 * (base + i) + 1];
      pc[0] = b.next[2 * (base + i)]; pc[1] = b.next[2 * (base + i) + 1];
      fr[0] = b.f_ref[3 * (base + i)]; fr[1] = b.f_ref[3 * (base + i) + 1]; fr[2] = b.f_ref[3 * (base + i) + 2];
    }
    const kf_u64 mask = __ballot(keep);   // (every lane has read its entry before any lane writes: the lists close up in place)
    if (keep) {
      const size_t o = base + out + __popcll(mask & (((kf_u64)1 << lane) - 1));
      b.px_ref[2 * o] = pr[0]; b.px_ref[2 * o + 1] = pr[1];
      b.px_cur[2 * o] = pc[0]; b.px_cur[2 * o + 1] = pc[1];
      b.f_ref[3 * o] = fr[0]; b.f_ref[3 * o + 1] = fr[1]; b.f_ref[3 * o + 2] = fr[2];
      double f[3];
      klt_bearing(st.fx, st.fy, st.cx, st.cy, pc[0], pc[1], f);
      b.f_cur[3 * o] = f[0]; b.f_cur[3 * o + 1] = f[1]; b.f_cur[3 * o + 2] = f[2];
      // Vector2d(px_ref.x - px_cur.x, px_ref.y - px_cur.y).norm(): float differences, double norm
      const double ddx = (double)(pr[0] - pc[0]), ddy = (double)(pr[1] - pc[1]);
      const double disp = sqrt(ddx * ddx + ddy * ddy);
      b.disparity[o] = disp;
      const kf_u64 k = kf_key(disp);
      b.keys[o] = k;
      mn = k < mn ? k : mn; mx = k > mx ? k : mx;
    }
    out += __popcll(mask);
  }
  wave_lds_fence();   // the keys of every lane are visible to the wave
  mn = kf_wave_min(mn); mx = kf_wave_max(mx);
  double median = 0.0;
  if (out > 0) median = kf_unkey(kf_wave_select(keys, out, out / 2, mn, mx, s_hist[wave], s_cand[wave], &s_ctr[wave]));
  rep.result = out < b.min_tracked ? PLSVO_KLT_FAILURE : (median < b.min_disparity ? PLSVO_KLT_NO_KEYFRAME : PLSVO_KLT_TRACKED);
  rep.n_before = n; rep.n_after = out; rep.median_disparity = median; rep.n_calls = st.n_calls + 1;
  if (lane == 0) { b.count[s] = out; b.st[s].n_calls = st.n_calls + 1; b.report[s] = rep; }
}

}  // namespace plsvo_hip
