// detect_device.hpp -- FAST corner detection per grid cell on the pyramid slots (DESIGN.md 3.9 "Corner detection").
// Replaces plsvo::feature_detection::FastDetector::detect (src/feature_detection.cpp:53-104): per level fast_corner_detect_10,
// fast_corner_score_10 and fast_nonmax_3x3 ([ext] fast), vk::shiTomasiScore ([ext] vikit) for the survivors, and the best corner of
// every grid cell.  Included by pyramid_kernels.hip only.
//
//   detect_fast_kernel     one workgroup = one 64 x 32 tile of one (slot, level); every level of every slot in one launch.  The tile and
//                          its halo are staged in LDS; every pixel takes the early reject, the pixels that pass are listed and scored one
//                          lane each, the survivors of the 3 x 3 suppression are listed and get their Shi-Tomasi score one lane each;
//                          candidates are reduced per cell in LDS, then one global atomic per touched cell
//   detect_compact_kernel  one workgroup = one slot: cell keys -> plsvo_corner records in cell order + count, keys re-armed
//                          (seeds_start_kernel, seedlist_device.hpp, reads the keys in its place: seed rows instead of records)
//
// A candidate is a 64-bit key: high word = the bits of its (positive) Shi-Tomasi score, low word = ~((L << 26) | (y << 13) | x) in
// level-L pixels.  max over the keys of a cell = "strictly greater score wins, the earlier one in (level, y, x) order wins a tie":
// what the reference's sequential loop computes, whatever order the workgroups arrive in.  0 = no candidate (an armed cell).
#pragma once
#include <stdint.h>

#include "plsvo_dev.hpp"

namespace plsvo_hip {

// the 16 Bresenham offsets of radius 3 in circular order from (0, 3), as byte offsets into the LDS image
__device__ __forceinline__ int det_ring(int i) {
  constexpr int dx[16] = { 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1 };
  constexpr int dy[16] = { 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3 };
  return dy[i] * kDetImgW + dx[i];
}

// fast_corner_detect_10 + fast_corner_score_10 of the pixel at LDS offset c: 0 = no corner, else the score in [b, 254].
// t = max over the 32 arcs (16 starts, 2 signs) of the minimum over the arc's 10 pixels of +-(ring - p); the pixel is a corner iff
// t > b and upstream's binary search returns t - 1.
// The early reject: an arc of 10 leaves out 6 contiguous pixels, so it holds at least one pixel of every opposite pair -- two pairs
// reject most pixels of a real image.
__device__ __forceinline__ bool det_fast_maybe(const uint8_t* img, int c, int b) {
  const int p = img[c];
  const int hi = p + b, lo = p - b;
  const int r0 = img[c + det_ring(0)], r8 = img[c + det_ring(8)], r4 = img[c + det_ring(4)], r12 = img[c + det_ring(12)];
  const bool brighter = (r0 > hi || r8 > hi) && (r4 > hi || r12 > hi);
  const bool darker = (r0 < lo || r8 < lo) && (r4 < lo || r12 < lo);
  return brighter || darker;
}

__device__ __forceinline__ int det_fast_score(const uint8_t* img, int c, int b) {
  const int p = img[c];
  int d[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) d[i] = (int)img[c + det_ring(i)] - p;
  // sliding minimum and maximum over windows of 10 (2 -> 4 -> 8 -> 8 + 2), indices modulo 16
  int mn2[16], mx2[16], mn4[16], mx4[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) { mn2[i] = min(d[i], d[(i + 1) & 15]); mx2[i] = max(d[i], d[(i + 1) & 15]); }
#pragma unroll
  for (int i = 0; i < 16; ++i) { mn4[i] = min(mn2[i], mn2[(i + 2) & 15]); mx4[i] = max(mx2[i], mx2[(i + 2) & 15]); }
  int t = -256;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int mn10 = min(min(mn4[i], mn4[(i + 4) & 15]), mn2[(i + 8) & 15]);
    const int mx10 = max(max(mx4[i], mx4[(i + 4) & 15]), mx2[(i + 8) & 15]);
    t = max(t, max(mn10, -mx10));
  }
  return t > b ? t - 1 : 0;
}

// fast_nonmax_3x3 on the LDS score map (0 = no corner): s points at a corner's own score
__device__ __forceinline__ bool det_survives(const uint8_t* s) {
  const int sc = s[0];
  return sc > 0 && s[-kDetScoreW - 1] < sc && s[-kDetScoreW] < sc && s[-kDetScoreW + 1] < sc && s[-1] < sc && s[1] < sc &&
         s[kDetScoreW - 1] < sc && s[kDetScoreW] < sc && s[kDetScoreW + 1] < sc;
}

// vk::shiTomasiScore(img, x, y) on the LDS image; the caller has checked the border rule.  Integer sums are exact (each below 2^24, as
// upstream's float sums are), the division by 2.0 * 64 is exact, the rest is double arithmetic without contraction.
__device__ __forceinline__ float det_shi_tomasi(const uint8_t* img, int c) {
#pragma clang fp contract(off)
  int sxx = 0, syy = 0, sxy = 0;
#pragma unroll 1
  for (int j = -4; j < 4; ++j) {
    const uint8_t* r = img + c + j * kDetImgW;
#pragma unroll
    for (int i = -4; i < 4; ++i) {
      const int dx = (int)r[i + 1] - (int)r[i - 1];
      const int dy = (int)r[i + kDetImgW] - (int)r[i - kDetImgW];
      sxx += dx * dx; syy += dy * dy; sxy += dx * dy;
    }
  }
  const double a = (double)((float)sxx / 128.0f), bb = (double)((float)syy / 128.0f), cc = (double)((float)sxy / 128.0f);
  const double s = a + bb;
  const double det = a * bb - cc * cc;
  const double disc = s * s - 4.0 * det;
  return (float)(0.5 * (s - sqrt(disc)));
}

// grid: (tiles of all levels of one slot, n_slots).  kStages: write the score and survivor maps of the (single) level instead of keys.
// kTable: the slot of launch position blockIdx.y comes from a.slot_table (plsvo_seeds_keyframe_detect: the streams' keyframes sit in any
// slots).  An instantiation of its own: with the table as a run-time branch in the one kernel, plsvo_hip_detect_fast_dev measured 0.8 - 1.2 %
// slower than the parent on 4096 slots, outside the parent's run-to-run range; without the table the code is the parent's.
template <bool kStages, bool kTable = false>
__global__ __launch_bounds__(kDetThreads) void detect_fast_kernel(DetectLaunch a) {
  __shared__ __align__(16) uint8_t s_img[kDetImgW * kDetImgH + 16];
  __shared__ __align__(16) uint8_t s_score[kDetScoreW * kDetScoreH];
  __shared__ unsigned long long s_keys[kDetCellCap];
  __shared__ uint16_t s_cand[(kDetTileW + 2) * kDetScoreH];   // pixels of the 66 x 34 region that passed the early reject
  __shared__ uint16_t s_surv[kDetTileW * kDetTileH];          // pixels of the tile that survived the suppression
  __shared__ int s_n[2];                                      // their counts
  const int tid = threadIdx.x;
  int e = 0;
  while (e + 1 < a.n_lv && (int)blockIdx.x >= a.tile_begin[e + 1]) ++e;
  const int L = a.level[e], W = a.w[e], H = a.h[e];
  const int tile = (int)blockIdx.x - a.tile_begin[e];
  const int ty = tile / a.tiles_x[e], tx = tile - ty * a.tiles_x[e];
  const int x0 = tx * kDetTileW, y0 = ty * kDetTileH;
  const size_t slot = kTable ? (size_t)a.slot_table[blockIdx.y] : (size_t)blockIdx.y;
  const uint8_t* lvl = a.pyr + slot * a.slot_bytes + a.off[e];   // 256-byte aligned, W * H bytes + >= 64 of slack

  // ---- stage the tile + halo: dword loads of the row-major level.  Row r of the LDS image starts at level byte (y0 - 5 + r) * W + x0 - 8,
  // which is dword-aligned only when W is a multiple of 4: otherwise two dwords are merged.  Bytes left or right of the image row belong
  // to its neighbour rows and bytes past the level to its slack: no pixel the stencils accept reads them.  Dwords outside
  // [0, W * H + 64) are not read at all (0).
  const int limit = (W * H + 64) & ~3;
  for (int i = tid; i < (kDetImgW / 4) * kDetImgH; i += kDetThreads) {
    const int r = i / (kDetImgW / 4), q = i - r * (kDetImgW / 4);
    const int g = (y0 - kDetImgY0 + r) * W + x0 - kDetImgX0 + 4 * q;
    const int al = g & ~3, sh = g & 3;
    uint32_t v = 0;
    if (al >= 0 && al + 4 <= limit) {
      v = *reinterpret_cast<const uint32_t*>(lvl + al);
      if (sh) {
        const uint32_t v1 = (al + 8 <= limit) ? *reinterpret_cast<const uint32_t*>(lvl + al + 4) : 0u;
        v = __builtin_amdgcn_alignbyte(v1, v, (uint32_t)sh);
      }
    }
    reinterpret_cast<uint32_t*>(s_img)[i] = v;
  }
  if (!kStages) for (int i = tid; i < kDetCellCap; i += kDetThreads) s_keys[i] = 0ull;
  if (tid < 2) s_n[tid] = 0;
  __syncthreads();

  // ---- corner + score over the tile and a ring of 1 (66 x 34): one byte per pixel, 0 = no corner.  Two passes, so that the lanes of a
  // wave do the expensive part together: every pixel takes the early reject and the ones that pass are listed in LDS (in any order:
  // a pixel's score depends on the image alone); then one lane per listed pixel computes its score.
  for (int i = tid; i < (kDetTileW + 2) * kDetScoreH; i += kDetThreads) {
    const int py = i / (kDetTileW + 2), px = i - py * (kDetTileW + 2);
    const int x = x0 - 1 + px, y = y0 - 1 + py;
    s_score[py * kDetScoreW + px] = 0;
    if (x >= 3 && x < W - 3 && y >= 3 && y < H - 3 && det_fast_maybe(s_img, (py - 1 + kDetImgY0) * kDetImgW + px - 1 + kDetImgX0, a.fast_b))
      s_cand[atomicAdd(&s_n[0], 1)] = (uint16_t)i;
  }
  __syncthreads();
  const int n_cand = s_n[0];
  for (int j = tid; j < n_cand; j += kDetThreads) {
    const int i = s_cand[j];
    const int py = i / (kDetTileW + 2), px = i - py * (kDetTileW + 2);
    s_score[py * kDetScoreW + px] = (uint8_t)det_fast_score(s_img, (py - 1 + kDetImgY0) * kDetImgW + px - 1 + kDetImgX0, a.fast_b);
  }
  __syncthreads();

  // the cells this tile can touch
  const int xl = min(x0 + kDetTileW, W) - 1, yl = min(y0 + kDetTileH, H) - 1;
  const int cx0 = (x0 << L) / a.cell, cy0 = (y0 << L) / a.cell;
  const int ncx = (xl << L) / a.cell - cx0 + 1, ncy = (yl << L) / a.cell - cy0 + 1;
  const bool in_lds = ncx * ncy <= kDetCellCap;
  const size_t slot_cells = (size_t)blockIdx.y * (size_t)a.n_cells;

  // ---- non-maximum suppression: a corner survives iff no 8-neighbour that is a corner scores >= it (non-corners are 0 < sc)
  if (kStages) {   // the diagnostic writes both maps for every pixel of the tile
    for (int i = tid; i < kDetTileW * kDetTileH; i += kDetThreads) {
      const int iy = i / kDetTileW, ix = i - iy * kDetTileW;
      const int x = x0 + ix, y = y0 + iy;
      const int sc = s_score[(iy + 1) * kDetScoreW + ix + 1];
      if (x < W && y < H) {
        a.stage_score[(size_t)y * W + x] = (uint8_t)sc;
        a.stage_survives[(size_t)y * W + x] = det_survives(s_score + (iy + 1) * kDetScoreW + ix + 1) ? 1 : 0;
      }
    }
    return;
  }
  // the survivors among the listed pixels of the tile proper (not its ring) are listed in turn; shiTomasiScore returns 0.0f within 4 px
  // of the border, which is never above the threshold
  for (int j = tid; j < n_cand; j += kDetThreads) {
    const int i = s_cand[j];
    const int py = i / (kDetTileW + 2), px = i - py * (kDetTileW + 2);
    const int x = x0 - 1 + px, y = y0 - 1 + py;
    if (px < 1 || px > kDetTileW || py < 1 || py > kDetTileH || !det_survives(s_score + py * kDetScoreW + px)) continue;
    if (x - 4 < 1 || x + 4 >= W - 1 || y - 4 < 1 || y + 4 >= H - 1) continue;
    s_surv[atomicAdd(&s_n[1], 1)] = (uint16_t)((py - 1) * kDetTileW + px - 1);
  }
  __syncthreads();
  // ---- Shi-Tomasi of the survivors, one lane each, and the best candidate per cell
  const int n_surv = s_n[1];
  for (int j = tid; j < n_surv; j += kDetThreads) {
    const int i = s_surv[j];
    const int iy = i / kDetTileW, ix = i - iy * kDetTileW;
    const int x = x0 + ix, y = y0 + iy;
    const float st = det_shi_tomasi(s_img, (iy + kDetImgY0) * kDetImgW + ix + kDetImgX0);
    if (!(st > a.thr)) continue;
    const unsigned long long key = ((unsigned long long)__float_as_uint(st) << 32) | (uint32_t)~(((uint32_t)L << 26) | ((uint32_t)y << 13) | (uint32_t)x);
    const int cx = (x << L) / a.cell, cy = (y << L) / a.cell;
    if (in_lds) atomicMax(&s_keys[(cy - cy0) * ncx + (cx - cx0)], key);
    else {
      const size_t k = slot_cells + (size_t)cy * a.cols + cx;
      if (!a.occupancy || !a.occupancy[k]) atomicMax(&a.keys[k], key);
    }
  }
  __syncthreads();

  // ---- one global atomic per touched, unoccupied cell
  if (in_lds)
    for (int i = tid; i < ncx * ncy; i += kDetThreads) {
      const unsigned long long key = s_keys[i];
      if (!key) continue;
      const int cy = i / ncx, cx = i - cy * ncx;
      const size_t k = slot_cells + (size_t)(cy0 + cy) * a.cols + cx0 + cx;
      if (!a.occupancy || !a.occupancy[k]) atomicMax(&a.keys[k], key);
    }
}

// grid: n_slots.  Cell keys of a slot -> records in cell-index order (the first counts[slot] of the slot's n_cells are valid), keys back to 0.
__global__ __launch_bounds__(kDetThreads) void detect_compact_kernel(unsigned long long* keys, int n_cells, plsvo_corner* corners, int32_t* counts) {
  __shared__ int s_wave[kDetThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long* k = keys + (size_t)blockIdx.x * (size_t)n_cells;
  plsvo_corner* out = corners + (size_t)blockIdx.x * (size_t)n_cells;
  int base = 0;
  for (int c0 = 0; c0 < n_cells; c0 += kDetThreads) {
    const int i = c0 + tid;
    unsigned long long key = 0ull;
    if (i < n_cells) { key = k[i]; if (key) k[i] = 0ull; }
    const unsigned long long m = __ballot(key != 0ull);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int off = base, total = 0;
#pragma unroll
    for (int w = 0; w < kDetThreads / 64; ++w) { if (w < wave) off += s_wave[w]; total += s_wave[w]; }
    if (key) {
      const uint32_t pos = ~(uint32_t)key;
      const int L = (int)(pos >> 26), y = (int)((pos >> 13) & 8191u), x = (int)(pos & 8191u);
      plsvo_corner r;
      r.x = x << L; r.y = y << L; r.score = __uint_as_float((uint32_t)(key >> 32)); r.level = L;
      out[off + __popcll(m & ((1ull << lane) - 1ull))] = r;
    }
    base += total;
    __syncthreads();
  }
  if (tid == 0) counts[blockIdx.x] = base;
}

}  // namespace plsvo_hip
