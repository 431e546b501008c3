// pyramid_kernels.hip -- 2x2 half-sampling of u8 images on the device (SURVEY 8f "next" #1).
// Replaces vk::halfSample ([ext] vikit/vision.h), called by frame_utils::createImgPyramid
// (src/frame.cpp:171-180).  HBM-bound byte kernel: each lane reads 2 x 8 contiguous bytes and writes
// 4 bytes, fully coalesced; one launch handles one level of a whole batch of slots.
//   rounding 0: vikit's SSE2 path  avg(avg(a,c), avg(b,d)) with rounding averages (x+y+1)>>1
//   rounding 1: vikit's scalar path (a+b+c+d)/4 truncating
// Also the rectification of raw distorted frames into level 0 (vk::PinholeCamera::undistortImage, app/run_pipeline.cpp:397-411):
// a byte gather through a packed map shared by every slot (DESIGN.md "Rectification").
// And the corner detector that reads the slots (feature_detection::FastDetector::detect, src/feature_detection.cpp:53-104): detect_device.hpp.
#include <hip/hip_runtime.h>

#include "plsvo_dev.hpp"
#include "detect_device.hpp"

namespace plsvo_hip {

__device__ __forceinline__ uint32_t half4(uint32_t t0, uint32_t t1, uint32_t b0, uint32_t b1, int rounding) {
  // t0,t1: 8 bytes of the top row; b0,b1: 8 bytes of the bottom row -> 4 output bytes
  uint32_t out = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t tw = (k < 2) ? t0 : t1, bw = (k < 2) ? b0 : b1;
    const int sh = (k & 1) * 16;
    const uint32_t a = (tw >> sh) & 0xff, b = (tw >> (sh + 8)) & 0xff, c = (bw >> sh) & 0xff, d = (bw >> (sh + 8)) & 0xff;
    uint32_t v;
    if (rounding == 0) { const uint32_t ac = (a + c + 1) >> 1, bd = (b + d + 1) >> 1; v = (ac + bd + 1) >> 1; }
    else v = (a + b + c + d) >> 2;
    out |= v << (8 * k);
  }
  return out;
}

// grid: (ceil(ow/4 * oh / 256), n_slots); src/dst: slot s at base + s*pitch
__global__ __launch_bounds__(256) void halfsample_kernel(const uint8_t* src, size_t src_pitch, int in_w, int in_h, int in_stride,
                                                         uint8_t* dst, size_t dst_pitch, int rounding) {
  const int ow = in_w >> 1, oh = in_h >> 1;
  const int qw = (ow + 3) >> 2;  // quads per output row
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= qw * oh) return;
  const int y = idx / qw, q = idx - y * qw;
  const uint8_t* s = src + (size_t)blockIdx.y * src_pitch;
  uint8_t* d = dst + (size_t)blockIdx.y * dst_pitch;
  const uint8_t* r0 = s + (size_t)(2 * y) * in_stride + 8 * q;
  const uint8_t* r1 = r0 + in_stride;
  uint8_t* o = d + (size_t)y * ow + 4 * q;
  const bool fast = (4 * q + 4 <= ow) && ((in_stride & 7) == 0) && ((reinterpret_cast<uintptr_t>(s) & 7) == 0) &&
                    ((ow & 3) == 0) && ((reinterpret_cast<uintptr_t>(d) & 3) == 0);
  if (fast) {
    const uint2 t = *reinterpret_cast<const uint2*>(r0);
    const uint2 bt = *reinterpret_cast<const uint2*>(r1);
    *reinterpret_cast<uint32_t*>(o) = half4(t.x, t.y, bt.x, bt.y, rounding);
  } else {
    for (int k = 0; k < 4 && 4 * q + k < ow; ++k) {
      const uint32_t a = r0[2 * k], b = r0[2 * k + 1], c = r1[2 * k], dd = r1[2 * k + 1];
      uint32_t v;
      if (rounding == 0) { const uint32_t ac = (a + c + 1) >> 1, bd = (b + dd + 1) >> 1; v = (ac + bd + 1) >> 1; }
      else v = (a + b + c + dd) >> 2;
      o[k] = (uint8_t)v;
    }
  }
}

// strided copy of level 0 into the slab (rows tightened)
__global__ __launch_bounds__(256) void copy_level0_kernel(const uint8_t* src, size_t src_pitch, int w, int h, int stride,
                                                          uint8_t* dst, size_t dst_pitch) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const int qw = (w + 15) >> 4;
  if (idx >= qw * h) return;
  const int y = idx / qw, q = idx - y * qw;
  const uint8_t* s = src + (size_t)blockIdx.y * src_pitch + (size_t)y * stride + 16 * q;
  uint8_t* d = dst + (size_t)blockIdx.y * dst_pitch + (size_t)y * w + 16 * q;
  const bool fast = (16 * q + 16 <= w) && ((reinterpret_cast<uintptr_t>(s) & 15) == 0) && ((reinterpret_cast<uintptr_t>(d) & 15) == 0);
  if (fast) *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(s);
  else for (int k = 0; k < 16 && 16 * q + k < w; ++k) d[k] = s[k];
}

// row-major level -> 16 x 8 tiles (plsvo_dev.hpp): one thread per 16-byte tile row; pixels beyond the image edge are written as 0
__global__ __launch_bounds__(256) void tile_level_kernel(const uint8_t* src, size_t src_pitch, int w, int h, uint8_t* dst, size_t dst_pitch) {
  const int tiles_x = (w + 15) >> 4, tiles_y = (h + 7) >> 3;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;      // tile-row index: (tile, row inside the tile)
  if (idx >= tiles_x * tiles_y * 8) return;
  const int tile = idx >> 3, r = idx & 7;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int y = ty * 8 + r, x0 = tx * 16;
  const uint8_t* s = src + (size_t)blockIdx.y * src_pitch + (size_t)y * w + x0;
  uint8_t* d = dst + (size_t)blockIdx.y * dst_pitch + ((size_t)tile << 7) + (r << 4);
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (y < h) {
    if (x0 + 16 <= w && (reinterpret_cast<uintptr_t>(s) & 15) == 0) v = *reinterpret_cast<const uint4*>(s);
    else {
      uint32_t q[4] = { 0u, 0u, 0u, 0u };
      for (int k = 0; k < 16 && x0 + k < w; ++k) q[k >> 2] |= (uint32_t)s[k] << (8 * (k & 3));
      v = make_uint4(q[0], q[1], q[2], q[3]);
    }
  }
  *reinterpret_cast<uint4*>(d) = v;
}

// ---- rectification of raw distorted frames (vk::PinholeCamera::undistortImage = OpenCV remap INTER_LINEAR, BORDER_CONSTANT 0) ----
// One map word per output pixel, shared by every slot (built and packed on the host, plsvo_capi.hip):
//   bits 0..9 = (fy & 31) * 32 + (fx & 31), the fixed-point fraction; bits 10..20 = x0 + 1; bits 21..31 = y0 + 1
// (x0, y0) = the top-left source tap.  A tap outside the raw frame reads 0; a pixel with every tap outside is stored as x0 = w.
// Map rows are padded to a multiple of 4 words, so every lane loads its 4 words as one 16-byte load.
__device__ __forceinline__ uint32_t rectify_px(const uint8_t* src, int row_step, int w, int h, int y_first, int y_sign, uint32_t m) {
  const int tx = (int)(m & 31u), ty = (int)((m >> 5) & 31u);
  const int x0 = (int)((m >> 10) & 2047u) - 1, y0 = (int)(m >> 21) - 1;
  // initInterTab2D's fixed-point weights (INTER_REMAP_COEF_SCALE = 32768); entry (0, 0) saturates to 32767 and OpenCV's fix-up adds the
  // missing 1 to the last tap
  int w00 = (32 - ty) * (32 - tx) * 32, w01 = (32 - ty) * tx * 32, w10 = ty * (32 - tx) * 32, w11 = ty * tx * 32;
  if ((m & 1023u) == 0u) { w00 = 32767; w11 = 1; }
  const uint8_t* r0 = src + (ptrdiff_t)(y_first + y_sign * y0) * row_step;   // raw row of tap row y0 (flipped: h - 1 - y0)
  const uint8_t* r1 = r0 + (ptrdiff_t)y_sign * row_step;
  int v00 = 0, v01 = 0, v10 = 0, v11 = 0;
  if ((unsigned)x0 < (unsigned)(w - 1) && (unsigned)y0 < (unsigned)(h - 1)) {
    v00 = r0[x0]; v01 = r0[x0 + 1]; v10 = r1[x0]; v11 = r1[x0 + 1];
  } else {
    const bool xa = (unsigned)x0 < (unsigned)w, xb = (unsigned)(x0 + 1) < (unsigned)w;
    const bool ya = (unsigned)y0 < (unsigned)h, yb = (unsigned)(y0 + 1) < (unsigned)h;
    if (ya && xa) v00 = r0[x0];
    if (ya && xb) v01 = r0[x0 + 1];
    if (yb && xa) v10 = r1[x0];
    if (yb && xb) v11 = r1[x0 + 1];
  }
  const int s = (v00 * w00 + v01 * w01 + v10 * w10 + v11 * w11 + (1 << 14)) >> 15;
  return (uint32_t)(s > 255 ? 255 : s);
}

// grid: (ceil(qw * h / 256), n_slots), qw = ceil(w / 4), like the other pyramid kernels: the workgroups in flight walk one frame after the
// other (the shared map is re-read per slot from L2 / MALL).  Each lane writes 4 output pixels of one row (one 32-bit store when the row
// allows it).
// raw frame of slot s at raw + s * raw_pitch, rows stride apart; flip: raw row h - 1 - y is read as row y.
__global__ __launch_bounds__(256) void rectify_kernel(const uint8_t* raw, size_t raw_pitch, int stride, int flip, const uint32_t* map,
                                                      int w, int h, uint8_t* dst, size_t dst_pitch) {
  const int qw = (w + 3) >> 2;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= qw * h) return;
  const int y = idx / qw, q = idx - y * qw;
  const uint4 m = *reinterpret_cast<const uint4*>(map + (size_t)idx * 4);
  const uint8_t* src = raw + (size_t)blockIdx.y * raw_pitch;
  const int y_first = flip ? h - 1 : 0, y_sign = flip ? -1 : 1;
  const uint32_t p0 = rectify_px(src, stride, w, h, y_first, y_sign, m.x);
  const uint32_t p1 = rectify_px(src, stride, w, h, y_first, y_sign, m.y);
  const uint32_t p2 = rectify_px(src, stride, w, h, y_first, y_sign, m.z);
  const uint32_t p3 = rectify_px(src, stride, w, h, y_first, y_sign, m.w);
  uint8_t* o = dst + (size_t)blockIdx.y * dst_pitch + (size_t)y * w + 4 * q;
  if (4 * q + 4 <= w && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
    *reinterpret_cast<uint32_t*>(o) = p0 | (p1 << 8) | (p2 << 16) | (p3 << 24);
  } else {
    const uint32_t p[4] = { p0, p1, p2, p3 };
    for (int k = 0; k < 4 && 4 * q + k < w; ++k) o[k] = (uint8_t)p[k];
  }
}

hipError_t launch_rectify(const uint8_t* raw, size_t raw_pitch, int stride, int flip, const uint32_t* map, int w, int h, uint8_t* dst,
                          size_t dst_pitch, int n_slots, hipStream_t stream) {
  const int work = ((w + 3) >> 2) * h;
  if (work <= 0 || n_slots <= 0) return hipSuccess;
  hipLaunchKernelGGL(rectify_kernel, dim3((work + 255) / 256, n_slots), dim3(256), 0, stream, raw, raw_pitch, stride, flip, map, w, h,
                     dst, dst_pitch);
  return hipGetLastError();
}

// FAST corners per grid cell (detect_device.hpp): keys of n_slots slots, then (launch_detect_compact) records + counts
hipError_t launch_detect_fast(const DetectLaunch& a, int n_slots, hipStream_t stream) {
  const int tiles = a.tile_begin[a.n_lv];
  if (tiles <= 0 || n_slots <= 0) return hipSuccess;
  if (a.slot_table) hipLaunchKernelGGL((detect_fast_kernel<false, true>), dim3(tiles, n_slots), dim3(kDetThreads), 0, stream, a);
  else hipLaunchKernelGGL(detect_fast_kernel<false>, dim3(tiles, n_slots), dim3(kDetThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_detect_stages(const DetectLaunch& a, hipStream_t stream) {
  const int tiles = a.tile_begin[a.n_lv];
  if (tiles <= 0) return hipSuccess;
  hipLaunchKernelGGL(detect_fast_kernel<true>, dim3(tiles, 1), dim3(kDetThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_detect_compact(unsigned long long* keys, int n_cells, plsvo_corner* corners, int32_t* counts, int n_slots, hipStream_t stream) {
  if (n_cells <= 0 || n_slots <= 0) return hipSuccess;
  hipLaunchKernelGGL(detect_compact_kernel, dim3(n_slots), dim3(kDetThreads), 0, stream, keys, n_cells, corners, counts);
  return hipGetLastError();
}

hipError_t launch_tile_level(const uint8_t* src, size_t src_pitch, int w, int h, uint8_t* dst, size_t dst_pitch, int n_slots, hipStream_t stream) {
  const int work = ((w + 15) >> 4) * ((h + 7) >> 3) * 8;
  if (work <= 0 || n_slots <= 0) return hipSuccess;
  hipLaunchKernelGGL(tile_level_kernel, dim3((work + 255) / 256, n_slots), dim3(256), 0, stream, src, src_pitch, w, h, dst, dst_pitch);
  return hipGetLastError();
}

hipError_t launch_halfsample(const uint8_t* src, size_t src_pitch, int in_w, int in_h, int in_stride, uint8_t* dst,
                             size_t dst_pitch, int n_slots, int rounding, hipStream_t stream) {
  const int ow = in_w >> 1, oh = in_h >> 1;
  const int work = ((ow + 3) >> 2) * oh;
  if (work <= 0 || n_slots <= 0) return hipSuccess;
  hipLaunchKernelGGL(halfsample_kernel, dim3((work + 255) / 256, n_slots), dim3(256), 0, stream, src, src_pitch, in_w, in_h,
                     in_stride, dst, dst_pitch, rounding);
  return hipGetLastError();
}

hipError_t launch_copy_level0(const uint8_t* src, size_t src_pitch, int w, int h, int stride, uint8_t* dst, size_t dst_pitch,
                              int n_slots, hipStream_t stream) {
  const int work = ((w + 15) >> 4) * h;
  if (work <= 0 || n_slots <= 0) return hipSuccess;
  hipLaunchKernelGGL(copy_level0_kernel, dim3((work + 255) / 256, n_slots), dim3(256), 0, stream, src, src_pitch, w, h, stride,
                     dst, dst_pitch);
  return hipGetLastError();
}

}  // namespace plsvo_hip
