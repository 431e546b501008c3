// structopt_kernels.hip -- structure optimisation on gfx950: one LANE per 3-D landmark.
//
// Replaces (reference file:line):
//   plsvo::Point::optimize      src/feature3D_impl.cpp:36-95
//   plsvo::LineSeg::optimize    src/feature3D_impl.cpp:97-174
//   Point::jacobian_xyz2uv      include/plsvo/feature3D.h:126-140
//   [ext] Eigen::LDLT<Matrix3d>::solve
// called per frame from FrameHandlerBase::optimizeStructure (src/frame_handler_base.cpp:202-237) on <= 20 points
// and <= 20 segments, 5 iterations each.  Every landmark is an independent 3x3 Gauss-Newton over a handful of
// observations, so there is nothing to reduce across lanes: a batch of landmarks (many frames' worth) is one
// launch, one lane each, observations read through flat offset tables.
//
// This file is compiled with -ffp-contract=off and evaluates every expression in the reference's order, so the
// results are BIT-IDENTICAL to the CPU oracle (the reference's own arithmetic here is unambiguous double math).
#include <hip/hip_runtime.h>

#include "plsvo_dev.hpp"
#include "structopt_device.hpp"   // the solve and the two optimise bodies, shared with the resident stage (structsel_device.hpp)

namespace plsvo_hip {

__global__ __launch_bounds__(64) void structopt_kernel(StructBatchDev s) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < s.n_pts) {                                     // Point::optimize :36-95
    const int i = idx;
    double pos[3] = { s.pt_pos[3 * i], s.pt_pos[3 * i + 1], s.pt_pos[3 * i + 2] };
    const int iters = point_optimize(s.frame_T, s.pt_obs_frame, s.pt_obs_f, s.pt_obs_off[i], s.pt_obs_off[i + 1], s.n_iter_pts, pos);
    s.pt_pos_out[3 * i] = pos[0]; s.pt_pos_out[3 * i + 1] = pos[1]; s.pt_pos_out[3 * i + 2] = pos[2];
    s.pt_iters[i] = iters;
  } else if (idx < s.n_pts + s.n_seg) {                    // LineSeg::optimize :97-174
    const int i = idx - s.n_pts;
    double sp[3], ep[3];
    for (int k = 0; k < 3; ++k) { sp[k] = s.seg_spos[3 * i + k]; ep[k] = s.seg_epos[3 * i + k]; }
    const int iters = segment_optimize(s.frame_T, s.seg_obs_frame, s.seg_obs_sf, s.seg_obs_ef, s.seg_obs_off[i], s.seg_obs_off[i + 1], s.n_iter_segs, sp, ep);
    for (int k = 0; k < 3; ++k) { s.seg_spos_out[3 * i + k] = sp[k]; s.seg_epos_out[3 * i + k] = ep[k]; }
    s.seg_iters[i] = iters;
  }
}

hipError_t launch_structopt(const StructBatchDev& s, hipStream_t stream) {
  const int n = s.n_pts + s.n_seg;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(structopt_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, s);
  return hipGetLastError();
}

// Diagnostic view of the solve (plsvo_structure_solve3; tests): one lane per system through the very ldlt_solve3 of structopt_device.hpp, in this
// translation unit and therefore under its flags.  A is row-major 3x3 (the lower triangle is read), n systems back to back.
__global__ __launch_bounds__(64) void structopt_solve3_kernel(const double* A, const double* b, double* x, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double a[9], r[3], o[3];
  for (int k = 0; k < 9; ++k) a[k] = A[9 * (size_t)i + k];
  for (int k = 0; k < 3; ++k) r[k] = b[3 * (size_t)i + k];
  ldlt_solve3(a, r, o);
  for (int k = 0; k < 3; ++k) x[3 * (size_t)i + k] = o[k];
}

hipError_t launch_structopt_solve3(const double* A, const double* b, double* x, int n, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(structopt_solve3_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, A, b, x, n);
  return hipGetLastError();
}

}  // namespace plsvo_hip
