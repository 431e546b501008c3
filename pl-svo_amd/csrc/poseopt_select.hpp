// poseopt_select.hpp -- the exact medians of the pose optimiser's row kernels (poseopt_kernels.hip: pose_opt_rows_kernel, prologue and
// epilogue of the row refill): the k-th smallest of a row's non-negative IEEE values, taken over their bit patterns by the 16 lanes of
// a row.  row_radix_select walks all digits of the pattern, eight bits per pass from the top, and re-reads every value from memory in
// every pass, one load and one full wait per element.  row_select_regs reads nothing: every lane holds its values (i = rl, rl + 16, ...)
// in registers -- fetched once, all loads in flight together -- and
//   * takes the row's minimum and maximum pattern (DPP): equal = the answer; otherwise the first digit starts at their highest
//     differing bit (the top byte of an IEEE pattern is sign and high exponent bits and separates almost nothing);
//   * takes histogram passes from the registers until the bin of rank k holds at most 16 values, or no bit is left;
//   * compacts those values one per lane and finishes by rank: the lane with less <= k < leq holds the k-th smallest.
// An order statistic has one value: both routes return the same bits (tests/test_gpu_poseopt_select.py against np.sort, bit for bit).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace plsvo_hip {

constexpr int kRowSelectChunks = 20;                       // values per lane held in registers
constexpr int kRowSelectCap = 16 * kRowSelectChunks;       // 320 per row: 200 points + 80 segments are inside it; a wave with a longer active row takes row_radix_select
// which route a row took (RowSelectDev::path; the production kernels drop it)
constexpr int kRowSelectEqual = 1;       // minimum == maximum: no pass
constexpr int kRowSelectRank = 2;        // finished by rank among at most 16 values
constexpr int kRowSelectExtraPass = 4;   // more than one histogram pass (the bin of rank k held more than 16 values)
constexpr int kRowSelectFallback = 8;    // row_radix_select (option off, or a row of the wave above the cap)
constexpr int kRowSelectDigits = 16;     // every bit decided by histogram passes (more than 16 copies of the answer)

struct RowSelectDev {          // plsvo_poseopt_row_select: rows of patterns, four rows per workgroup
  const void* patterns;        // uint32 (bits == 32) or uint64 (bits == 64), the rows concatenated
  const long long* row_off;    // per row: first pattern
  const int* row_n;
  const int* row_k;
  const uint8_t* row_active;
  void* selected;              // per row: the k-th smallest pattern (0 for an inactive row)
  int* path;                   // per row: kRowSelect* bits (0 for an inactive row)
  int n_rows, bits, select;
};
hipError_t launch_pose_row_select(const RowSelectDev& t, hipStream_t stream);

}  // namespace plsvo_hip
