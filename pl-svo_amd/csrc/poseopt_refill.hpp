// poseopt_refill.hpp -- the row shape of the pose optimiser as three launches (poseopt_kernels.hip: prologue = rows_begin, persistent
// Gauss-Newton kernel whose rows take their next frame from a queue and run rows_gn_step, epilogue = rows_finish -- the phase functions
// pose_opt_rows_kernel is made of): what a frame carries through HBM between them, and the queue.
#pragma once
#include <hip/hip_runtime.h>

#include "plsvo_dev.hpp"

namespace plsvo_hip {

struct PoseRefillCarry {   // per frame, 544 bytes
  double pose[32];         // PoseRowLds::pose: 0..8 R, 9..11 t, 12..18 model, 19..25 T_old, 26 chi2, 27 point-iterations, 28 line-iterations
  double tot[32];          // PoseRowLds::tot of the last ASSEMBLED iteration (zero while none ran): the covariance's input
  double scale_pt, scale_ls;
  int iters;               // Gauss-Newton iterations run
  int reserved[3];
};

struct PoseRefillDev {
  PoseRefillCarry* carry;  // 1 per job
  int* next;               // the queue: next launch slot to hand out; zeroed ahead of every launch
};

// false in a -DPLSVO_TIMING build (the three kernels carry no phase ticks)
bool pose_opt_refill_built();
// prologue (4 frames per workgroup), Gauss-Newton kernel (gn_grid persistent workgroups), epilogue, back to back on `stream`;
// select: 1 = the medians of prologue and epilogue finish from registers (poseopt_select.hpp), 0 = row_radix_select everywhere
hipError_t launch_pose_opt_refill(const PoseBatchDev& b, const PoseRefillDev& q, double* d_poses, int gn_grid, int select, hipStream_t stream);

}  // namespace plsvo_hip
