/*
 * plsvo_hip.h -- C ABI of the MI355X (gfx950) hot path of PL-SVO:
 *   sparse image alignment (points + sampled line segments) and motion-only pose optimisation,
 *   plus the steps either side of it: device pyramids, map reprojection, direct feature
 *   matching, structure optimisation, depth-filter seed updates, trajectory records.
 *
 * This header IS the drop-in boundary.  The reference has no FFI layer; its boundary is two C++
 * call signatures (reference file:line given per entry point below).  The C++ adapter in
 * pl-svo_amd/host/plsvo/ re-creates those signatures on top of this ABI.
 *
 * Conventions
 *   - every function returns 0 on success and a negative PLSVO_E_* code on failure; nothing throws,
 *     nothing aborts; plsvo_hip_last_error() gives a human-readable string for the last failure.
 *   - plain pointers and sizes only; no C++/torch types.  Pointers are HOST pointers unless the
 *     parameter name starts with d_ (device pointer, HBM of the ctx's device).
 *   - a ctx is bound to one device and one HIP stream; use one ctx per calling thread.
 *   - poses travel as double[7] = { qx, qy, qz, qw, tx, ty, tz } (unit quaternion + translation),
 *     the storage of the reference's Sophus::SE3 (SO3 as unit quaternion, Vector3d translation).
 *   - there is NO CPU fallback behind this ABI: without a gfx950 device plsvo_hip_create() fails.
 */
#ifndef PLSVO_HIP_H_
#define PLSVO_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLSVO_MAX_LEVELS 8
#define PLSVO_PATCH_SIZE 4   /* reference: include/plsvo/sparse_img_align.h:48-50 (halfsize 2, size 4, area 16) */
#define PLSVO_PATCH_AREA 16

/* error codes */
#define PLSVO_OK              0
#define PLSVO_E_INVALID      -1  /* bad argument */
#define PLSVO_E_NODEVICE     -2  /* no usable HIP device (there is no CPU fallback) */
#define PLSVO_E_HIP          -3  /* a HIP runtime call failed; see plsvo_hip_last_error */
#define PLSVO_E_CAPACITY     -4  /* a ctx capacity (slots, features, patches) would be exceeded */
#define PLSVO_E_STATE        -5  /* call order violated (e.g. run before stage) */
#define PLSVO_E_RCCL         -6  /* an RCCL call failed */

typedef struct plsvo_ctx plsvo_ctx;

/* undistorted pinhole camera: the only model the reference demo hands the VO
 * (app/run_pipeline.cpp:786-795; vk::PinholeCamera with zero distortion, [ext] vikit) */
typedef struct plsvo_pinhole {
  double fx, fy, cx, cy;
  int32_t width, height;      /* level-0 image size */
} plsvo_pinhole;

/* ------------------------------------------------------------------------------------------ */
/* context                                                                                    */
/* ------------------------------------------------------------------------------------------ */

/* device_id: HIP ordinal.  stream: a hipStream_t (as void*) to enqueue on, or NULL to let the
 * ctx create its own non-blocking stream. */
int plsvo_hip_create(int device_id, void* stream, plsvo_ctx** out);
/* The same, but `stream` is ALWAYS the stream to enqueue on -- including the NULL handle, which is HIP's default (legacy)
 * stream and what e.g. torch.cuda.current_stream().cuda_stream returns when no other stream is current.  A caller that
 * orders other work (an RCCL collective, its own kernels) against the library's launches must use this form, or pass a
 * non-NULL stream: plsvo_hip_create(.., NULL, ..) enqueues on a private stream the caller's work is not ordered with. */
int plsvo_hip_create_on_stream(int device_id, void* stream, plsvo_ctx** out);
void plsvo_hip_destroy(plsvo_ctx* ctx);
/* Options of a context.  PLSVO_OPT_LDLT_FLAVOUR selects the zero-pivot rule of the 6x6 `H.ldlt().solve()` the two optimisers call
 * (src/sparse_img_align.cpp:699, src/pose_optimizer.cpp:170), which changed between the Eigen releases PL-SVO's named platforms
 * ship: 320 (default) = Eigen 3.1 ... 3.2.1 (Ubuntu 12.04 / 14.04: stop at eps * max|A_ii|, drop |d| <= eps * max|D|),
 * 330 = Eigen 3.2.2 and later (Ubuntu 16.04's 3.3-beta: exact zeros only).  Identical arithmetic on every full-rank system; they
 * differ with fewer than three point observations.  Takes effect at the next *_stage call. */
#define PLSVO_OPT_LDLT_FLAVOUR 1
/* Launch shapes (threads per frame) of the two hot kernels: 0 = chosen from the batch size (default), or a fixed 64 / 128 / 256 / 512
 * (alignment), 16 / 64 / 256 / 512 (pose optimiser; 16 = a 16-lane row per frame, four frames per wave: the large-batch shape).  For tests and measurements: every shape computes the same thing. */
#define PLSVO_OPT_ALIGN_THREADS 2
#define PLSVO_OPT_POSEOPT_THREADS 3
/* Launch order of a RE-RUN staged batch (plsvo_align_run / plsvo_poseopt_run called again without a new stage call): 1 (default) =
 * the frames start longest-first by the work the PREVIOUS launch of the batch measured (a counting sort on the device behind every
 * launch), 0 = every launch keeps the stage call's order (the alignment's: most patches first).  Scheduling only -- no result depends
 * on it.  The environment switches PLSVO_ALIGN_NO_REORDER / PLSVO_POSEOPT_NO_REORDER set the initial value to 0. */
#define PLSVO_OPT_ALIGN_REORDER 4
#define PLSVO_OPT_POSEOPT_REORDER 5
/* Tail split of the large-batch alignment launch (one wave per frame, at least four rounds of resident workgroups, at least two pyramid
 * levels): 1 (default) = the frames at the end of the launch order run as two workgroups of the same launch, their coarse levels first
 * of all and their finest level last of all, so that the launch does not end on whole long frames; 0 = one workgroup per frame
 * throughout.  Scheduling only -- every result is bit-identical.  The environment switch PLSVO_ALIGN_TAIL_SPLIT=0 sets the initial value to 0. */
#define PLSVO_OPT_ALIGN_TAIL_SPLIT 6
/* Row refill of the large-batch pose-optimiser launch (a 16-lane row per frame, more than two frames per resident row, no refinement
 * loop -- every n_iter_ref <= 0 --, no iteration trace): 1 (default) = the launch runs as three kernels, and the rows of the middle one
 * -- the Gauss-Newton loop, persistent -- take their next frame from a queue as soon as their frame stops; 0 = one kernel, the four
 * frames of a wave iterate until the last of them stops.  Scheduling only -- every result is bit-identical.  The environment switch
 * PLSVO_POSEOPT_REFILL=0 sets the initial value to 0; for tests and measurements PLSVO_POSEOPT_REFILL_MIN is the smallest batch (in
 * frames) that takes the three kernels and PLSVO_POSEOPT_REFILL_WAVES the number of workgroups of the persistent one (read once, at
 * plsvo_hip_create). */
#define PLSVO_OPT_POSEOPT_REFILL 7
/* Medians of the pose optimiser's row kernels (the two MAD scales, error_init, error_final; a 16-lane row per frame): 1 (default) =
 * every lane fetches its values once into registers, the first digit starts at the highest bit in which the row's minimum and maximum
 * differ, and the last (at most 16) candidates are finished by rank; 0 = the radix select that walks every digit over memory.  A wave
 * with a row of more than 320 values takes the latter either way.  An order statistic has one value: every result is bit-identical.
 * The environment switch PLSVO_POSEOPT_SELECT=0 sets the initial value to 0. */
#define PLSVO_OPT_POSEOPT_SELECT 8
/* 6x6 solve of the alignment's Gauss-Newton iteration, every launch shape: 1 (default) = six distinct, non-NaN |diagonals| fix Eigen's
 * pivot order before the first elimination step, so the order is sorted once and the six steps run without a pivot search; exact ties
 * and NaN diagonals take the search; 0 = the search in every step.  Same arithmetic in the same order: every result is bit-identical.
 * The environment switch PLSVO_ALIGN_STATIC_SOLVE=0 sets the initial value to 0. */
#define PLSVO_OPT_ALIGN_STATIC_SOLVE 9
int plsvo_hip_set_option(plsvo_ctx* ctx, int option, int value);
const char* plsvo_hip_last_error(const plsvo_ctx* ctx);   /* ctx may be NULL: last create error */
void* plsvo_hip_stream(plsvo_ctx* ctx);                   /* the hipStream_t all work is enqueued on */
int plsvo_hip_synchronize(plsvo_ctx* ctx);

/* ------------------------------------------------------------------------------------------ */
/* image pyramids (input of both frames; replaces Frame::img_pyr_, include/plsvo/frame.h:64,   */
/* filled by frame_utils::createImgPyramid, src/frame.cpp:171-180)                             */
/* ------------------------------------------------------------------------------------------ */

/* Allocate n_slots pyramid slots of n_levels u8 images, level l = (width>>l) x (height>>l),
 * rows stored tightly (stride == width of the level).  Re-configuring frees the old slab. */
int plsvo_hip_config_pyramids(plsvo_ctx* ctx, int n_slots, int width, int height, int n_levels);

/* Upload an existing host pyramid (what the reference keeps in Frame::img_pyr_) into a slot.
 * The call returns WITHOUT a stream synchronisation: the levels are packed into a pinned image of the slot and cross PCIe as one
 * copy enqueued on the context's stream -- the caller's buffers are free on return, and whatever is launched on the stream afterwards
 * reads the new pyramid (a caller that reads the slot from ANOTHER stream orders it with plsvo_hip_synchronize).  The slot's tiled
 * mirror (read by the one-wave-per-frame shape of the alignment only) is refreshed LAZILY: the slot is marked stale here and re-tiled
 * by the first launch that reads the mirror; plsvo_hip_build_pyramid / _build_pyramids_dev / _copy_slots refresh it eagerly. */
int plsvo_hip_upload_pyramid(plsvo_ctx* ctx, int slot, int n_levels,
                             const uint8_t* const* level_ptr, const int* width, const int* height,
                             const int* stride_bytes);

/* Upload level 0 only and build levels 1.. on the device with the 2x2 half-sampler
 * (replaces vk::halfSample, [ext] vikit/vision.h, called from src/frame.cpp:178).
 * rounding: 0 = vikit SSE2 path  avg(avg(a,c),avg(b,d)) with (x+y+1)>>1
 *           1 = vikit scalar path (a+b+c+d)/4 truncating. */
int plsvo_hip_build_pyramid(plsvo_ctx* ctx, int slot, const uint8_t* level0, int stride_bytes,
                            int rounding);
/* Same, level 0 already in HBM (tight rows or stride_bytes), for n consecutive slots starting at
 * first_slot; image i is at d_level0 + i*image_pitch_bytes. */
int plsvo_hip_build_pyramids_dev(plsvo_ctx* ctx, int first_slot, int n, const void* d_level0,
                                 int stride_bytes, size_t image_pitch_bytes, int rounding);
/* Device-to-device copy of n whole pyramid slots (src_first.. -> dst_first.., ranges must not overlap), enqueued on the ctx stream:
 * "the current frame becomes the reference frame" (src/frame_handler_mono.cpp:272-274) for a resident batch without crossing PCIe. */
int plsvo_hip_copy_slots(plsvo_ctx* ctx, int dst_first, int src_first, int n);
/* Read one level of a slot back to the host (tight rows); for tests. */
int plsvo_hip_download_level(plsvo_ctx* ctx, int slot, int level, uint8_t* out);

/* ------------------------------------------------------------------------------------------ */
/* rectification of raw distorted frames into pyramid slots                                   */
/* replaces vk::PinholeCamera::undistortImage ([ext] vikit, an OpenCV initUndistortRectifyMap  */
/* + remap) and the vertical flip before it (app/run_pipeline.cpp:397-411), followed by        */
/* frame_utils::createImgPyramid (DESIGN.md "Rectification")                                  */
/* ------------------------------------------------------------------------------------------ */

/* radial-tangential pinhole camera: vk::PinholeCamera(w, h, fx, fy, cx, cy, d0, d1, d2, d3, d4),
 * d = { k1, k2, p1, p2, k3 }.  fx..cy and d are rounded to float first, as vikit stores them.
 * |d[0]| <= 1e-7 is vikit's identity branch: the frame is copied, whatever d[1..4] hold. */
typedef struct plsvo_pinhole_radtan {
  plsvo_pinhole cam;
  double d[5];
} plsvo_pinhole_radtan;

#define PLSVO_MAX_RECTIFY_MAPS 8   /* rectification maps one ctx holds (one per camera of a rig) */

/* Host-only helper (no device needed): the map OpenCV's initUndistortRectifyMap(K, D, I, K, size, CV_16SC2) builds for the camera,
 * in OpenCV's form: xy = width*height pairs (x, y) of the top-left source tap, frac = width*height entries (fy & 31) * 32 + (fx & 31).
 * This is the map of the parameters as given: the identity branch (|d[0]| <= 1e-7) is applied by the device calls, not here.
 * PLSVO_E_INVALID (nothing written) for non-finite parameters or a size outside 1 .. 2046 in either direction. */
int plsvo_rectify_map(const plsvo_pinhole_radtan* cam, int16_t* xy, uint16_t* frac);
/* Build the camera's map once, pack it for the device and upload it: *map_id receives its handle (0 .. PLSVO_MAX_RECTIFY_MAPS-1).
 * flip_vertical != 0: the raw frame is flipped vertically before the remap (run_pipeline does this for a negative fy).  The camera size
 * must equal the level-0 size of plsvo_hip_config_pyramids (which must have been called); a re-configuration keeps the maps. */
int plsvo_hip_config_rectify(plsvo_ctx* ctx, const plsvo_pinhole_radtan* cam, int flip_vertical, int* map_id);
/* Rectify one raw host frame (stride_bytes per row) into level 0 of `slot` and build levels 1.. with the half-sampler (rounding as
 * plsvo_hip_build_pyramid).  One PCIe copy of the raw frame; the tiled mirror is refreshed eagerly. */
int plsvo_hip_rectify_build_pyramid(plsvo_ctx* ctx, int map_id, int slot, const uint8_t* raw, int stride_bytes, int rounding);
/* Same, raw frames already in HBM: frame i at d_raw + i*image_pitch_bytes -> slot first_slot + i, i < n.
 * Every error (unknown map, camera size != configured pyramid, slot range out of bounds, stride < width) is PLSVO_E_INVALID and
 * writes nothing. */
int plsvo_hip_rectify_build_pyramids_dev(plsvo_ctx* ctx, int map_id, int first_slot, int n, const void* d_raw,
                                         int stride_bytes, size_t image_pitch_bytes, int rounding);

/* ------------------------------------------------------------------------------------------ */
/* FAST corners per grid cell from pyramid slots                                              */
/* replaces plsvo::feature_detection::FastDetector::detect (src/feature_detection.cpp:53-104), */
/* called by DepthFilter::initializeSeeds (src/depth_filter.cpp:161-165) and the bootstrap     */
/* (src/initialization.cpp:135-137): fast_corner_detect_10, fast_corner_score_10 and           */
/* fast_nonmax_3x3 ([ext] fast) per level, vk::shiTomasiScore ([ext] vikit) of the survivors,  */
/* the best corner of every grid cell (DESIGN.md "Corner detection")                          */
/* ------------------------------------------------------------------------------------------ */

/* one feature: px in level-0 pixels = (x_L << level, y_L << level), score = its Shi-Tomasi score (feature_detection.cpp:93) */
typedef struct plsvo_corner { int32_t x, y; float score; int32_t level; } plsvo_corner;

typedef struct plsvo_detect_params {
  int32_t cell_size;            /* Config::gridSize() (25) */
  int32_t n_levels;             /* Config::nPyrLevels() (3); <= the configured levels */
  int32_t fast_threshold;       /* 20 (feature_detection.cpp:67), 1..254 */
  int32_t reserved0;
  double  detection_threshold;  /* Config::triangMinCornerScore() (20.0): >= 0, finite, exactly representable as float */
} plsvo_detect_params;

/* Host only, no ctx: the grid of AbstractDetector (include/plsvo/feature_detection.h:97,110-112), cols = ceil(width / cell_size),
 * rows = ceil(height / cell_size).  PLSVO_E_INVALID (nothing written) for a size or cell below 1 or a NULL output. */
int plsvo_detect_grid(int width, int height, int cell_size, int* cols, int* rows);
/* Host only, no ctx: the cell index FastDetector::setGridOccpuancy / setExistingFeatures mark for a feature at level-0 pixel
 * (px_x, px_y) (src/feature_detection.cpp:106-121): (int)(px_y / cell_size) * cols + (int)(px_x / cell_size).
 * PLSVO_E_INVALID for cols or cell_size below 1 and for a pixel that is negative or not finite. */
int plsvo_detect_cell(int cols, int cell_size, double px_x, double px_y);
/* FastDetector::detect for slots [first_slot, first_slot + n): with cells = cols * rows of plsvo_detect_grid for the configured
 * level-0 size, slot i reads occupancy[i * cells .. ) (non-zero = the cell already holds a feature; NULL = no cell does) and writes
 * its features to corners[i * cells .. ) in cell-index order, the first counts[i] of them valid.  Host buffers; synchronous.
 * PLSVO_E_STATE when the pyramids are not configured; PLSVO_E_INVALID for a slot range out of bounds, n_levels outside 1 .. the
 * configured levels, cell_size < 1, a level smaller than 7 x 7, a level-0 width or height above 8191, fast_threshold outside 1..254,
 * a detection_threshold that is negative, not finite or not a float, or a NULL params / corners / counts.  An error writes nothing. */
int plsvo_hip_detect_fast(plsvo_ctx* ctx, int first_slot, int n, const plsvo_detect_params* params, const uint8_t* occupancy,
                          plsvo_corner* corners, int32_t* counts);
/* Same with device buffers (d_occupancy may be NULL); enqueued on the ctx stream, nothing is waited for: a detection can follow
 * plsvo_hip_rectify_build_pyramids_dev / plsvo_hip_build_pyramids_dev without a host round trip. */
int plsvo_hip_detect_fast_dev(plsvo_ctx* ctx, int first_slot, int n, const plsvo_detect_params* params, const uint8_t* d_occupancy,
                              plsvo_corner* d_corners, int32_t* d_counts);
/* Diagnostic: the stages of one level of one slot before the grid, as the three fast:: calls leave them
 * (src/feature_detection.cpp:63-82): score[y * W_L + x] = fast_corner_score_10 of a corner, 0 = not a corner;
 * survives[..] = 1 where fast_nonmax_3x3 keeps it.  Host buffers of W_L * H_L bytes each; synchronous. */
int plsvo_hip_detect_stages(plsvo_ctx* ctx, int slot, int level, int fast_threshold, uint8_t* score, uint8_t* survives);

/* ------------------------------------------------------------------------------------------ */
/* sparse image alignment                                                                      */
/* replaces plsvo::SparseImgAlign::run   (include/plsvo/sparse_img_align.h:64-66,              */
/*                                        src/sparse_img_align.cpp:54-95; call sites           */
/*                                        src/frame_handler_mono.cpp:272-274, 418-420)         */
/* ------------------------------------------------------------------------------------------ */

/* One alignment job = one SparseImgAlign::run(ref_frame, cur_frame).
 * Features are those of the REFERENCE frame, flattened (the adapter walks the std::lists once):
 *   points  (ref_frame->pt_fts_ with feat3D != NULL):
 *     pt_px      2*n_pts  Feature::px, level-0 pixels                (include/plsvo/feature.h:42)
 *     pt_xyz_ref 3*n_pts  f * ||feat3D->pos_ - ref_frame->pos()||    (src/sparse_img_align.cpp:229-230)
 *   segments (ref_frame->seg_fts_, ALL of them, so indices stay stable):
 *     seg_spx/seg_epx 2*n_seg  LineFeat::spx / epx                   (include/plsvo/feature.h:85-86)
 *     seg_len    n_seg    LineFeat::length                           (include/plsvo/feature.h:92)
 *     seg_p_ref  3*n_seg  sf * ||feat3D->spos_ - ref_pos||           (src/sparse_img_align.cpp:327-328)
 *     seg_q_ref  3*n_seg  ef * ||feat3D->epos_ - ref_pos||           (src/sparse_img_align.cpp:329-330)
 *     seg_alive_in n_seg  1 if feat3D != NULL, 0 otherwise; NULL = all alive
 */
typedef struct plsvo_align_in {
  int32_t ref_slot, cur_slot;       /* pyramid slots of ref_frame / cur_frame */
  plsvo_pinhole cam;                /* cur_frame->cam_ == ref_frame->cam_ */
  int32_t max_level, min_level;     /* SparseImgAlign ctor (src/sparse_img_align.cpp:40-52) */
  int32_t n_iter;                   /* n_iter_ (30 at the call sites) */
  int32_t reserved0;
  double eps;                       /* eps_ = 1e-6 (src/sparse_img_align.cpp:51) */
  double T_cur_from_ref[7];         /* cur.T_f_w * ref.T_f_w^-1 (src/sparse_img_align.cpp:80) */
  int32_t n_pts, n_seg;
  const double* pt_px;
  const double* pt_xyz_ref;
  const double* seg_spx;
  const double* seg_epx;
  const double* seg_len;
  const double* seg_p_ref;
  const double* seg_q_ref;
  const uint8_t* seg_alive_in;
} plsvo_align_in;

typedef struct plsvo_align_out {
  double T_cur_from_ref[7];         /* after all levels (src/sparse_img_align.cpp:92 multiplies by ref.T_f_w) */
  uint64_t n_meas;                  /* n_meas_ of the last computeResiduals call */
  uint64_t n_tracked;               /* run()'s return value n_meas_/16 (src/sparse_img_align.cpp:94) */
  double H[36];                     /* H_ of the last computeResiduals (row-major; getFisherInformation, :97-102) */
  double chi2;                      /* chi2_ of the solver ([ext] vk::NLLSSolver) */
  uint8_t* seg_alive_out;           /* caller buffer of n_seg bytes or NULL; 0 = LineFeat::feat3D set to NULL
                                       (src/sparse_img_align.cpp:687-688) */
  int32_t iters_per_level[PLSVO_MAX_LEVELS];  /* #computeResiduals calls in the GN loop, index = level */
  int32_t status;                   /* bit 0: solver stop_ flag was raised (NaN in solve, :700) */
  int32_t reserved0;
} plsvo_align_out;

/* per-iteration trace (debug/parity): one record per GN iteration, in execution order */
typedef struct plsvo_align_iterlog {
  int32_t level, iter;
  int32_t accepted;                 /* 1: update applied; 0: rolled back / stopped at this iteration */
  int32_t stop;                     /* solver stop_ flag after this iteration */
  uint64_t n_meas;
  double new_chi2;                  /* value returned by computeResiduals (float chi2 / n_meas) */
  double H[36], Jres[6], x[6];
  double T_after[7];                /* model after this iteration's accept/rollback decision */
} plsvo_align_iterlog;

/* one job, synchronous: stage + run + fetch (the drop-in call) */
int plsvo_sparse_align(plsvo_ctx* ctx, const plsvo_align_in* in, plsvo_align_out* out);
/* n independent jobs in one batch, synchronous (BASELINE config 4: many streams) */
int plsvo_sparse_align_batch(plsvo_ctx* ctx, int n, const plsvo_align_in* in, plsvo_align_out* out);

/* the same, split so that a batch can stay resident in HBM and be re-run (bench, pipelining):
 *   stage: copy job descriptors + features to the device (replaces any previously staged batch)
 *   run  : enqueue the kernels on the ctx stream (asynchronous); re-initialises poses and alive
 *          masks from the staged inputs each time it is called
 *   fetch: wait for the stream and copy the results back */
int plsvo_align_stage(plsvo_ctx* ctx, int n, const plsvo_align_in* in);
int plsvo_align_run(plsvo_ctx* ctx);
int plsvo_align_fetch(plsvo_ctx* ctx, int n, plsvo_align_out* out);

/* per-iteration trace: enable before plsvo_align_run; max_records_per_job bounds the trace */
/* Host-only helper (no device needed): the static patch-slot layout plsvo_align_stage gives one job at one pyramid level.
 * Points own slots [0, n_pts); the segments are packed behind them into the kernel's wave-rounds of 64 slots, first-fit in
 * decreasing N (N = 1 + (N0-1)/2^level, LineFeat::setupSampling src/feature.cpp:160-173, src/sparse_img_align.cpp:320; ties in
 * feature order), starting in the round the points leave partly empty; a segment with N <= 64 samples never straddles a multiple
 * of 64, longer ones follow behind the packed rounds.  seg_code[s] = first slot | N << 20, or -1 for a segment without landmark on
 * entry or with an end point inside the 3-pixel border of the level (src/sparse_img_align.cpp:299-301).  n_slots: slots in use;
 * long_lines: some N > 64 (the level then runs in two passes); n_patches: points + samples (holes not counted).  No result depends
 * on where a segment sits.  Returns PLSVO_E_CAPACITY for N > 2047 or more than 2^20 slots. */
int plsvo_align_slot_layout(const plsvo_align_in* in, int level, int32_t* seg_code, int32_t* n_slots, int32_t* long_lines,
                            long long* n_patches);

/* Diagnostic (measurements): the threads per frame and the LDS bytes per workgroup plsvo_align_run would launch the staged batch with. */
int plsvo_align_launch_shape(plsvo_ctx* ctx, int32_t* threads, uint64_t* lds_bytes);

int plsvo_align_set_trace(plsvo_ctx* ctx, int max_records_per_job);
int plsvo_align_fetch_trace(plsvo_ctx* ctx, int job, plsvo_align_iterlog* out, int max_records,
                            int* n_records);

/* Diagnostic view of the per-level set-up (tests; like plsvo_structure_solve3 for the structure optimiser): after plsvo_align_run,
 * the first n_slots patch slots of one job as the LAST level the run executed left them -- records: 64 bytes per slot (seven rows
 * of the 8 reference-image bytes [vi-3+k][ui-3 .. ui+4], then the two sub-pixel fractions as floats), uvref: the slot's reference
 * pixel position (u, v) at that level.  Slots no live feature owns at the level (holes) hold whatever was there.  Run ONE level
 * (max_level == min_level) to look at that level.  PLSVO_E_STATE before a run or after a run in a latency shape (256 threads per
 * frame and more keep float rows, not records); PLSVO_E_INVALID for n_slots beyond the job's allocation (the largest level's
 * slot count, rounded up to 4).  Costs the hot path nothing: two copies out of the buffers the kernel works in. */
int plsvo_align_fetch_records(plsvo_ctx* ctx, int job, int n_slots, unsigned char* records, float* uvref);

/* device pointer to the staged batch's result poses, n*7 doubles (for a device-side gather) */
const double* plsvo_align_poses_dev(plsvo_ctx* ctx);
/* enqueue a device-to-device copy of those n*7 doubles into caller-owned HBM (e.g. a torch tensor) */
int plsvo_align_copy_poses(plsvo_ctx* ctx, double* d_dst);

/* work counters of the last plsvo_align_run (for the roofline accounting):
 *   patch_levels = sum over jobs and levels of patches precomputed (497 B each)
 *   patch_iters  = sum over jobs, levels and GN iterations of patches evaluated (485 B each) */
int plsvo_align_work(plsvo_ctx* ctx, uint64_t* patch_levels, uint64_t* patch_iters);
/* The order in which the NEXT plsvo_align_run of the resident batch starts its jobs (block w works on job order[w]): the stage call's
   (most patches first) until the batch has run; after a run of a batch larger than the device's resident slots, the jobs sorted by the
   patch-iterations that run measured, longest first (align_kernels.hip::align_reorder_kernel).  Scheduling only: a job's results do not
   depend on its place in the launch.  Tests and measurements. */
int plsvo_align_launch_order(plsvo_ctx* ctx, int n, int32_t* order);
/* How many frames at the end of that order the LAST plsvo_align_run ran as two workgroups (PLSVO_OPT_ALIGN_TAIL_SPLIT): 0 when the
   launch was not split.  Tests and measurements. */
int plsvo_align_tail_frames(plsvo_ctx* ctx, int* tail_frames);
/* of patch_iters, the evaluations of POINT patches that also wrote their 64 B of per-pixel chi2 terms to HBM (see plsvo_align_chi2_ties) */
int plsvo_align_work_points(plsvo_ctx* ctx, uint64_t* point_patch_iters);

/* parity accounting of the last plsvo_align_run: Gauss-Newton iterations in total, and how many of them had their
 * `new_chi2 > chi2_` decision ([ext] vk::NLLSSolver::optimizeGaussNewton) taken on the reference's own sequential float sums
 * (src/sparse_img_align.cpp:484, 683, 171, 192) because the two chi2 values were closer than the rounding noise of those sums;
 * near_ties_without_terms: such iterations whose per-pixel terms had not been kept (large batches keep them only once the solver's
 * steps are small) -- decided on the exactly-rounded sums instead.  Any output may be NULL. */
int plsvo_align_chi2_ties(plsvo_ctx* ctx, uint64_t* iterations, uint64_t* ties, uint64_t* near_ties_without_terms);

/* ------------------------------------------------------------------------------------------ */
/* pose optimisation                                                                           */
/* replaces plsvo::pose_optimizer::optimizeGaussNewton (include/plsvo/pose_optimizer.h:47-64,  */
/*          src/pose_optimizer.cpp:38-260 and :262-582; call site frame_handler_mono.cpp:327)  */
/* ------------------------------------------------------------------------------------------ */

/* Features are those of the frame being optimised, flattened, only entries with feat3D != NULL:
 *   pt_f   3*n_pts  Feature::f (bearing)         pt_pos  3*n_pts  feat3D->pos_ (world)
 *   pt_level n_pts  Feature::level
 *   seg_line 3*n_seg LineFeat::line (src/feature.cpp:103-104)
 *   seg_spos/seg_epos 3*n_seg feat3D->spos_/epos_ (world)     seg_level n_seg */
typedef struct plsvo_poseopt_in {
  double T_f_w[7];                  /* frame->T_f_w_ on entry */
  double fx;                        /* frame->cam_->errorMultiplier2() = |fx| ([ext] vikit) */
  double reproj_thresh;             /* 2.0 at the call site (src/config.cpp:102) */
  int32_t n_iter;                   /* 10 at the call site (src/config.cpp:103) */
  int32_t n_iter_ref;               /* <0: 9-argument overload (:38); >=0: 10-argument overload (:262) */
  int32_t n_pts, n_seg;
  const double* pt_f;
  const double* pt_pos;
  const int32_t* pt_level;
  const double* seg_line;
  const double* seg_spos;
  const double* seg_epos;
  const int32_t* seg_level;
} plsvo_poseopt_in;

typedef struct plsvo_poseopt_out {
  double T_f_w[7];                  /* frame->T_f_w_ on exit */
  double cov[36];                   /* frame->Cov_ (src/pose_optimizer.cpp:198-199), row-major */
  double estimated_scale, error_init, error_final;
  uint64_t num_obs_pt, num_obs_ls;
  uint8_t* pt_keep;                 /* caller buffers (n_pts / n_seg bytes) or NULL; 0 = feat3D set to NULL */
  uint8_t* seg_keep;                /*   (src/pose_optimizer.cpp:218, 239) */
  int32_t iters;                    /* GN iterations executed in the first loop */
  int32_t iters_ref;                /* ... in the refinement loop of the 10-argument overload */
  int32_t status;                   /* bit 0: early return, nothing written (errors.empty(), :88-89) */
  int32_t reserved0;
} plsvo_poseopt_out;

typedef struct plsvo_poseopt_iterlog {
  int32_t phase;                    /* 0: first loop, 1: refinement loop */
  int32_t iter;
  int32_t accepted;
  int32_t reserved0;
  double new_chi2;
  double A[36], b[6], dT[6];
  double T_after[7];
} plsvo_poseopt_iterlog;

int plsvo_pose_optimize(plsvo_ctx* ctx, const plsvo_poseopt_in* in, plsvo_poseopt_out* out);
int plsvo_pose_optimize_batch(plsvo_ctx* ctx, int n, const plsvo_poseopt_in* in, plsvo_poseopt_out* out);
int plsvo_poseopt_stage(plsvo_ctx* ctx, int n, const plsvo_poseopt_in* in);
int plsvo_poseopt_run(plsvo_ctx* ctx);
int plsvo_poseopt_fetch(plsvo_ctx* ctx, int n, plsvo_poseopt_out* out);
int plsvo_poseopt_set_trace(plsvo_ctx* ctx, int max_records_per_job);
int plsvo_poseopt_fetch_trace(plsvo_ctx* ctx, int job, plsvo_poseopt_iterlog* out, int max_records,
                              int* n_records);
const double* plsvo_poseopt_poses_dev(plsvo_ctx* ctx);
int plsvo_poseopt_copy_poses(plsvo_ctx* ctx, double* d_dst);
/* feature-iterations of the last run: points (24 B each) and lines (40 B each), SURVEY 8d */
int plsvo_poseopt_work(plsvo_ctx* ctx, uint64_t* pt_iters, uint64_t* seg_iters);
/* How many frames the LAST pose-optimiser launch of the context -- plsvo_poseopt_run, or the pose stage of plsvo_chain_run -- ran
   through the row-refill path (PLSVO_OPT_POSEOPT_REFILL): the whole batch, or 0 when it ran as one kernel (the chain's always does:
   its jobs are written on the device).  Tests and measurements. */
int plsvo_poseopt_refill_frames(plsvo_ctx* ctx, int* refill_frames);
/* For tests: the select of the row kernels' medians -- the very device function, four rows per 64-thread workgroup -- on rows of
 * unsigned patterns.  selected: n_rows patterns of `bits` bits (the k-th smallest of each row, 0-based; 0 for an inactive or empty row);
 * path: n_rows words of PLSVO_ROW_SELECT_* bits, the route a row took (0 for an inactive row).  Rows of one workgroup (4 consecutive
 * rows) share the route when one of them is above the cap.  Follows PLSVO_OPT_POSEOPT_SELECT. */
#define PLSVO_ROW_SELECT_CAP 320          /* values per row the register route holds */
#define PLSVO_ROW_SELECT_EQUAL 1          /* minimum == maximum */
#define PLSVO_ROW_SELECT_RANK 2           /* finished by rank among at most 16 candidates */
#define PLSVO_ROW_SELECT_EXTRA_PASS 4     /* more than one histogram pass */
#define PLSVO_ROW_SELECT_FALLBACK 8       /* the radix select over memory */
#define PLSVO_ROW_SELECT_DIGITS 16        /* every bit decided by histogram passes */
typedef struct {
  int32_t bits;                 /* 32 or 64 */
  int32_t n_rows;
  const void* patterns;         /* n_patterns values of uint32_t / uint64_t */
  int64_t n_patterns;
  const int64_t* row_off;       /* per row: index of its first pattern */
  const int32_t* row_n;
  const int32_t* row_k;         /* 0 <= k < n for an active row */
  const uint8_t* row_active;
} plsvo_row_select_in;
int plsvo_poseopt_row_select(plsvo_ctx* ctx, const plsvo_row_select_in* in, void* selected, int32_t* path);

/* ------------------------------------------------------------------------------------------ */
/* structure optimisation (hot-path contract row (f) "next" #3)                                */
/* replaces plsvo::Point::optimize / plsvo::LineSeg::optimize (src/feature3D_impl.cpp:36-95,   */
/* :97-174), called from FrameHandlerBase::optimizeStructure (src/frame_handler_base.cpp:      */
/* 202-237; call site src/frame_handler_mono.cpp:340)                                          */
/* ------------------------------------------------------------------------------------------ */

/* A batch of independent 3-D landmarks, each refined by its own 3x3 Gauss-Newton over its observations
 * (Feature3D::obs_, include/plsvo/feature3D.h): observation = (frame pose T_f_w, unit bearing f).
 *   frame_T        7*n_frames   poses of every frame referenced by an observation
 *   pt_pos         3*n_pts      Point::pos_ on entry
 *   pt_obs_off     n_pts+1      observations of point i are [pt_obs_off[i], pt_obs_off[i+1])
 *   pt_obs_frame   n_pt_obs     index into frame_T            (Feature::frame)
 *   pt_obs_f       3*n_pt_obs   Feature::f
 *   seg_*                       the same for LineSeg::spos_/epos_ with LineFeat::sf / ef
 * The landmark selection (nth_element on last_structure_optim_) stays on the host. */
typedef struct plsvo_structopt_in {
  int32_t n_frames;
  int32_t n_iter_pts;               /* Config::structureOptimNumIter() */
  int32_t n_iter_segs;              /* Config::structureOptimNumIterSegs() */
  int32_t n_pts, n_seg;
  int32_t reserved0;
  const double* frame_T;
  const double* pt_pos;
  const int32_t* pt_obs_off;
  const int32_t* pt_obs_frame;
  const double* pt_obs_f;
  const double* seg_spos;
  const double* seg_epos;
  const int32_t* seg_obs_off;
  const int32_t* seg_obs_frame;
  const double* seg_obs_sf;
  const double* seg_obs_ef;
} plsvo_structopt_in;

typedef struct plsvo_structopt_out {   /* caller buffers; any of them may be NULL */
  double* pt_pos;                   /* 3*n_pts  Point::pos_ on exit */
  double* seg_spos;                 /* 3*n_seg */
  double* seg_epos;                 /* 3*n_seg */
  int32_t* pt_iters;                /* n_pts: residual evaluations executed (1..n_iter) */
  int32_t* seg_iters;               /* n_seg */
} plsvo_structopt_out;

/* pt_obs_off / seg_obs_off must start at 0 and never decrease: anything else is PLSVO_E_INVALID before anything is uploaded. */
int plsvo_structure_optimize(plsvo_ctx* ctx, const plsvo_structopt_in* in, plsvo_structopt_out* out);

/* Diagnostic view of the optimiser's 3x3 solve (tests; like plsvo_match_warp_patches for the matcher): x = A.ldlt().solve(b) for n
 * independent systems, one lane each, through the device function plsvo_structure_optimize's kernel calls (Eigen 3.2's zero-pivot
 * rule, flavour 320 only).  A: 9*n, row-major 3x3 per system, the lower triangle is read; b, x: 3*n.  NaN/Inf propagate into x. */
int plsvo_structure_solve3(plsvo_ctx* ctx, int32_t n, const double* A, const double* b, double* x);

/* ------------------------------------------------------------------------------------------ */
/* direct feature matching (hot-path contract row (f) "next" #2)                               */
/* replaces plsvo::Matcher::findMatchDirect for points (src/matcher.cpp:159-207) and for line  */
/* segments (:232-275), with everything they call: warp::getWarpMatrixAffine (:44-71),         */
/* warp::getBestSearchLevel (:73-86), warp::warpAffine (:88-129),                              */
/* Matcher::createPatchFromPatchWithBorder (:148-157), Matcher::precomputeRefPatch (:209-230), */
/* feature_alignment::align1D (src/feature_alignment.cpp:41-158) and align2D (:160-290).       */
/* Call sites: Reprojector::refineBestCandidate (src/reprojector.cpp:288, :348).               */
/* ------------------------------------------------------------------------------------------ */

#define PLSVO_FTR_CORNER  0         /* PointFeat::CORNER, and both end points of a LineFeat */
#define PLSVO_FTR_EDGELET 1         /* PointFeat::EDGELET: 1-D alignment along the warped gradient */

/* A batch of n independent match candidates.  One candidate = one 2-D position to refine in the image of
 * frame cur_frame[i], starting from px_cur[i] (the landmark's projection, written by Reprojector), against the
 * 8x8 patch around the landmark's closest-view observation (Point::getCloseViewObs, chosen by the host).
 * A line segment contributes two candidates (start and end point, each with its own pos / px / f); the
 * caller ANDs the two `found` flags like matcher.cpp:253-274.  Images are the ctx's pyramid slots.
 *   frame_T      7*n_frames  Frame::T_f_w_ of every frame referenced
 *   frame_slot   n_frames    pyramid slot holding that frame's Frame::img_pyr_
 *   cur_frame    n           index of the frame matched into
 *   ref_frame    n           index of ref_ftr_->frame
 *   ref_px       2*n         ref_ftr_->px (level-0 pixels)       ref_f   3*n   ref_ftr_->f
 *   ref_level    n           ref_ftr_->level                     ref_type n    PLSVO_FTR_*
 *   ref_grad     2*n         PointFeat::grad (read for edgelets only; may be NULL when there are none)
 *   pos          3*n         Point::pos_ (LineSeg::spos_ / epos_)
 *   px_cur       2*n         initial estimate in level-0 pixels of the current image */
typedef struct plsvo_match_in {
  plsvo_pinhole cam;                /* ref_ftr_->frame->cam_ == cur_frame.cam_ (one camera) */
  int32_t n_pyr_levels;             /* Config::nPyrLevels(): search level <= n_pyr_levels-1 (matcher.cpp:177) */
  int32_t align_max_iter;           /* Matcher::Options::align_max_iter (10, include/plsvo/matcher.h:98) */
  int32_t n_frames;
  int32_t n;
  const double* frame_T;
  const int32_t* frame_slot;
  const int32_t* cur_frame;
  const int32_t* ref_frame;
  const double* ref_px;
  const double* ref_f;
  const int32_t* ref_level;
  const uint8_t* ref_type;
  const double* ref_grad;
  const double* pos;
  const double* px_cur;
} plsvo_match_in;

typedef struct plsvo_match_out {    /* caller buffers; any of them may be NULL */
  double* px_cur;                   /* 2*n  refined position (level-0 pixels); the input value when the
                                       reference observation is too close to the border (matcher.cpp:168-170) */
  uint8_t* found;                   /* n    findMatchDirect's return value */
  int32_t* search_level;            /* n    Matcher::search_level_ (-1 when rejected before the warp) */
  int32_t* n_iter;                  /* n    residual passes executed by align1D/align2D */
} plsvo_match_out;

int plsvo_match_direct(plsvo_ctx* ctx, const plsvo_match_in* in, plsvo_match_out* out);

/* Diagnostic view of the matcher's affine warp (tests; like plsvo_hip_detect_stages for the detector): the production kernel of
 * plsvo_match_direct, instantiated to stop after warp::warpAffine and to write what it holds at that point.  Same inputs, same
 * argument checks (px_cur and align_max_iter are checked, not used). */
typedef struct plsvo_match_warp_out { /* caller buffers; any of them may be NULL */
  double* A;                        /* 4*n    warp::getWarpMatrixAffine's A_cur_ref, row-major {a00, a01, a10, a11}; 0 when rejected */
  int32_t* search_level;            /* n      warp::getBestSearchLevel (-1 when rejected by the border check before the warp) */
  uint8_t* warped;                  /* n      1 when warpAffine wrote the patch (0: rejected, or the inverse of A is NaN) */
  uint8_t* patch;                   /* 100*n  patch_with_border_, rows 0..9 x columns 0..9; all 0 when not warped */
  uint8_t* staged;                  /* n      bit g set: patch rows 2g, 2g+1 took their taps from the window staged in LDS
                                              (pl-svo_amd/csrc/match_device.hpp::warp_affine_lds); other groups read the image */
} plsvo_match_warp_out;

int plsvo_match_warp_patches(plsvo_ctx* ctx, const plsvo_match_in* in, plsvo_match_warp_out* out);

/* Reprojector::reproject(frame, Point*) / (frame, LineSeg*) (src/reprojector.cpp:389-423): the projection of map
 * landmarks into a frame that produces the candidates (and their initial px_cur) for plsvo_match_direct.
 *   px[i]   = frame->w2c(pos[i]) = world2cam(T_f_w * pos[i])                      (include/plsvo/frame.h:113)
 *   cell[i] = (int)(px.y / cell_size) * grid_n_cols + (int)(px.x / cell_size)    when isInFrame(px.cast<int>(), 8),
 *             -1 otherwise (the reference then rejects the landmark; a segment needs both end points in frame and
 *             is filed under both cells, :405-421 -- the caller ANDs, like for plsvo_match_direct)
 * The grid itself (cells, random visit order, one match per cell) is host control flow and stays with the caller. */
typedef struct plsvo_reproject_in {
  plsvo_pinhole cam;
  int32_t n_frames;                 /* poses referenced */
  int32_t n;                        /* landmark positions (points, segment start points, segment end points) */
  int32_t cell_size;                /* Config::gridSize() (points) or gridSizeSegs() (segments) */
  int32_t grid_n_cols;              /* ceil(width / cell_size)  (reprojector.cpp:59, :71) */
  int32_t boundary;                 /* 8: "the patch size in the matcher" (:393) */
  int32_t reserved0;
  const double* frame_T;            /* 7*n_frames  Frame::T_f_w_ */
  const int32_t* frame;             /* n: index of the frame each position is projected into */
  const double* pos;                /* 3*n world positions */
} plsvo_reproject_in;

typedef struct plsvo_reproject_out { /* caller buffers; either may be NULL */
  double* px;                       /* 2*n */
  int32_t* cell;                    /* n */
} plsvo_reproject_out;

int plsvo_reproject(plsvo_ctx* ctx, const plsvo_reproject_in* in, plsvo_reproject_out* out);

/* ------------------------------------------------------------------------------------------ */
/* resident frame step (hot-path contract row (f) "next": the callers either side of the path) */
/* FrameHandlerMono::processFrame runs alignment -> Reprojector::reprojectMap -> pose          */
/* optimisation back to back (src/frame_handler_mono.cpp:263-345).  plsvo_chain_* runs the     */
/* same sequence for a batch of streams in ONE call: the alignment result is composed into the */
/* new frame's pose (:92), the map candidates are projected with it, matched                   */
/* (Matcher::findMatchDirect), selected, turned into bearings / line equations                 */
/* (src/feature.cpp:103-104) and handed to the pose optimiser without leaving the device.      */
/* ------------------------------------------------------------------------------------------ */

/* One stream.  Candidates are the landmarks of ONE keyframe (pose T_kf_w, pyramid slot kf_slot) with their observation in it, in
 * the caller's order of preference (the reference sorts a cell's candidates by landmark quality, reprojector.cpp:225):
 * n_cand_pt points, then the start points of n_cand_seg segments, then their end points -- every array below has
 * n_cand_pt + 2 * n_cand_seg entries in that order (ref_type / ref_grad are read for points only). */
typedef struct plsvo_chain_in {
  plsvo_align_in align;             /* previous frame -> new frame; ref_slot / cur_slot are the two frames' pyramid slots */
  double T_prev_w[7];               /* previous frame's T_f_w_ */
  double T_kf_w[7];                 /* keyframe's T_f_w_ */
  int32_t kf_slot;
  int32_t n_cand_pt, n_cand_seg;
  int32_t reserved0;
  const double* pos;                /* 3 per candidate: Point::pos_ / LineSeg::spos_ / LineSeg::epos_ */
  const double* ref_px;             /* 2: the keyframe observation (as plsvo_match_in) */
  const double* ref_f;              /* 3 */
  const int32_t* ref_level;
  const uint8_t* ref_type;          /* PLSVO_FTR_*; may be NULL (all corners) */
  const double* ref_grad;           /* 2; may be NULL without edgelets */
  const uint8_t* active;            /* may be NULL: 0 = leave this candidate out (e.g. a landmark not yet in the map) */
} plsvo_chain_in;

typedef struct plsvo_chain_params {
  plsvo_pinhole cam;                /* one camera for the batch */
  int32_t n_pyr_levels;             /* Config::nPyrLevels() (matcher) */
  int32_t align_max_iter;           /* Matcher::Options::align_max_iter (10) */
  int32_t cell_size;                /* Config::gridSize(): the reprojection grid of the points (reprojector.cpp:57-66) */
  int32_t cell_rule;                /* 0: every matched candidate becomes a feature; 1: the reference's rule -- per cell the first
                                       candidate that matches, cells in cell_order, stop after the match that makes the count exceed
                                       max_fts (reprojector.cpp:188-199, :222-243).  Segments follow their own grid when seg_cell_size > 0
                                       (below); with seg_cell_size == 0 every segment whose two end points match becomes a feature */
  int32_t max_fts;                  /* Config::maxFts() */
  int32_t poseopt_n_iter;           /* 10 (src/config.cpp:103) */
  const int32_t* cell_order;        /* grid_n_cols * grid_n_rows cell indices (Grid::cell_order, shuffled once, :63-66); NULL = 0,1,2,.. */
  double reproj_thresh;             /* 2.0 (src/config.cpp:102) */
  /* the segments' grid, gridls_ (reprojector.cpp:68-79, :200-207, :256-275, :405-421), used when cell_rule != 0 and seg_cell_size > 0:
   * a segment is filed under the cell of its projected start point AND under the cell of its projected end point; cells are visited
   * in seg_cell_order, per cell the first segment (caller's order = quality order) whose findMatchDirect succeeded becomes a feature,
   * and the visit stops after the match that makes the count exceed max_fts_segs.  A segment that wins both of its cells becomes a
   * feature TWICE, as in the reference (refine() adds a LineFeat per success): sel_seg / seg_keep hold up to 2 * n_cand_seg entries. */
  int32_t seg_cell_size;            /* Config::gridSizeSegs(); 0 = no segment grid */
  int32_t max_fts_segs;             /* Config::maxFtsSegs() (100, src/config.cpp:76) */
  const int32_t* seg_cell_order;    /* ceil(width / seg_cell_size) * ceil(height / seg_cell_size) cell indices; NULL = 0,1,2,.. */
} plsvo_chain_params;

typedef struct plsvo_chain_out {
  plsvo_align_out align;            /* as plsvo_align_fetch */
  plsvo_poseopt_out pose;           /* as plsvo_poseopt_fetch; pt_keep / seg_keep index the SELECTED features (sel_pt / sel_seg order) */
  int32_t n_sel_pt, n_sel_seg;      /* features the new frame received */
  /* caller buffers, any may be NULL */
  uint8_t* found;                   /* per candidate: findMatchDirect's result (0 for candidates left out) */
  double* px;                       /* 2 per candidate: refined pixel (the projection for candidates left out / not found) */
  int32_t* search_level;            /* per candidate */
  int32_t* sel_pt;                  /* n_cand_pt: candidate index of selected point feature k, k < n_sel_pt */
  int32_t* sel_seg;                 /* n_cand_seg (2 * n_cand_seg with a segment grid): segment index of selected segment feature k, k < n_sel_seg */
} plsvo_chain_out;

int plsvo_chain_stage(plsvo_ctx* ctx, int n, const plsvo_chain_in* in, const plsvo_chain_params* params);
int plsvo_chain_run(plsvo_ctx* ctx);     /* enqueue only: alignment, pose composition, reprojection, matching, selection, pose optimisation */
int plsvo_chain_fetch(plsvo_ctx* ctx, int n, plsvo_chain_out* out);
int plsvo_frame_step_batch(plsvo_ctx* ctx, int n, const plsvo_chain_in* in, const plsvo_chain_params* params, plsvo_chain_out* out);
const double* plsvo_chain_poses_dev(plsvo_ctx* ctx);   /* n*7 doubles: the optimised T_f_w of the staged streams, on the device */

/* ------------------------------------------------------------------------------------------ */
/* keyframe stage: what FrameHandlerMono::processFrame decides between "pose optimised" and    */
/* "detect corners, start seeds" (src/frame_handler_mono.cpp:351-358, :396) and the head of    */
/* Reprojector::reprojectMap (src/reprojector.cpp:147-163), for a batch of independent streams */
/* (one wave per stream).  Synchronous; host arrays unless named d_.           */
/* ------------------------------------------------------------------------------------------ */

/* Map::getCloseKeyframes (src/map.cpp:158-179) followed by the sort and the cut of reprojectMap (:147-163).
 * The keyframe table of a stream: kf_T = Frame::T_f_w_ of every keyframe, keypt_pos = key_pts_[k]->feat3D->pos_ (world) of its five
 * key points, keypt_valid = 0 where key_pts_[k] is NULL.  A keyframe is close when one valid key point passes Frame::isVisible
 * (src/frame.cpp:156-165) in the frame with pose T_f_w; its distance is |T_f_w.translation() - kf.T_f_w.translation()| -- the
 * translations of the poses, not the camera centres, as in the reference. */
typedef struct plsvo_close_kf_in {
  plsvo_pinhole cam;                /* frame->cam_ */
  double T_f_w[7];                  /* the new frame's pose after alignment */
  int32_t n_kf;                     /* keyframes in the table */
  int32_t max_n_kfs;                /* Reprojector::Options::max_n_kfs (10) */
  const double* kf_T;               /* 7*n_kf */
  const double* keypt_pos;          /* 15*n_kf */
  const uint8_t* keypt_valid;       /* 5*n_kf */
} plsvo_close_kf_in;

typedef struct plsvo_close_kf_out {
  int32_t n_close;                  /* keyframes with an overlapping field of view */
  int32_t n_overlap;                /* min(n_close, max_n_kfs): the first n_overlap entries are the reference's overlap_kfs */
  int32_t* close_idx;               /* caller buffers of n_kf entries or NULL: the first n_close filled, ascending by distance, */
  double* close_dist;               /*   equal distances in table order (std::list::sort is stable) */
} plsvo_close_kf_out;

/* n streams.  PLSVO_E_INVALID (nothing written) for n < 0, a NULL in / out with n > 0, a negative n_kf or max_n_kfs, or a NULL table
 * array with n_kf > 0.  Finite inputs are a precondition. */
int plsvo_close_keyframes(plsvo_ctx* ctx, int n, const plsvo_close_kf_in* in, plsvo_close_kf_out* out);

/* One stream's frame after pose optimisation:
 *   frame_utils::getSceneDepth (src/frame.cpp:182-217) -> has_depth, depth_mean (vk::getMedian: the element of rank m/2), depth_min
 *   FrameHandlerMono::needNewKf (src/frame_handler_mono.cpp:475-499) over the overlap keyframes -> need_new_kf, blocking, delta_t/r
 *   Frame::setKeyPoints / checkKeyPoints (src/frame.cpp:87-141) -> key_pts
 *   Map::getFurthestKeyframe(new_frame->pos()) (src/map.cpp:201-214) -> furthest_kf
 * Features: pt_px = Feature::px, pt_pos = feat3D->pos_, pt_alive = 0 where feat3D is NULL (NULL array = all alive); segments alike. */
typedef struct plsvo_kf_decide_in {
  plsvo_pinhole cam;                /* only width and height are read (cu = width/2, cv = height/2) */
  double T_new_w[7];                /* new_frame_->T_f_w_ after pose optimisation */
  const double* d_T_new;            /* NULL, or a DEVICE pointer to 7 doubles read instead of T_new_w (plsvo_chain_poses_dev(ctx) + 7*i) */
  double T_last_w[7];               /* last_frame_->T_f_w_: the PREVIOUS frame's pose, which needNewKf measures from */
  double kfselect_mindist_t;        /* Config::kfSelectMinDistT() (0.06, src/config.cpp:112) */
  double kfselect_mindist_r;        /* Config::kfSelectMinDistR() (3.0 degrees of 3.1416, src/config.cpp:113) */
  int32_t n_pt, n_seg;
  int32_t n_kf, n_overlap;
  const double* pt_px;              /* 2*n_pt */
  const double* pt_pos;             /* 3*n_pt */
  const uint8_t* pt_alive;          /* n_pt or NULL */
  const double* seg_spos;           /* 3*n_seg */
  const double* seg_epos;           /* 3*n_seg */
  const uint8_t* seg_alive;         /* n_seg or NULL */
  const double* kf_T;               /* 7*n_kf: the keyframe table of plsvo_close_kf_in */
  const int32_t* overlap_idx;       /* n_overlap indices into it, in order (plsvo_close_kf_out.close_idx) */
  int32_t key_pts_prev[5];          /* key_pts_ on entry: indices into the points, -1 = NULL */
  int32_t reserved0;
} plsvo_kf_decide_in;

typedef struct plsvo_kf_decide_out {
  double depth_mean;                /* 0 when has_depth == 0 (the reference leaves its argument untouched) */
  double depth_min;                 /* DBL_MAX when has_depth == 0; of zeros of both signs the negative one */
  int32_t has_depth;                /* getSceneDepth's return value */
  int32_t n_depth;                  /* depth_vec.size(): alive points + 2 * alive segments */
  int32_t need_new_kf;              /* needNewKf's return value */
  int32_t blocking;                 /* position in overlap_idx of the first keyframe closer than both thresholds, -1 = none */
  int32_t key_pts[5];               /* key_pts_ on exit (indices, -1 = NULL) */
  int32_t furthest_kf;              /* index into the table, -1 when no keyframe is further than 0 */
  double* delta_t;                  /* caller buffers of n_overlap entries or NULL: |log(T_last^-1 * T_kf)[0:3]| and */
  double* delta_r;                  /*   |log(..)[3:6]| * 180.0 / 3.1416 of EVERY overlap keyframe (diagnostic) */
} plsvo_kf_decide_out;

/* n streams.  PLSVO_E_INVALID (nothing written) for n < 0, a NULL in / out with n > 0, a negative count, a NULL array with a
 * non-zero count (the alive arrays excepted), an overlap index outside the table or a key_pts_prev entry outside -1 .. n_pt-1. */
int plsvo_keyframe_decide(plsvo_ctx* ctx, int n, const plsvo_kf_decide_in* in, plsvo_kf_decide_out* out);

/* ------------------------------------------------------------------------------------------ */
/* map candidates: what Reprojector::reprojectMap builds between "close keyframes sorted" and   */
/* "match one candidate per cell" (src/reprojector.cpp:157-183) -- the visits of the overlap    */
/* keyframes' features with setKfCandidates (:92-109), setMapCandidates (:111-133), reproject   */
/* (:389-423) -- together with the closest-view observation the matcher picks first             */
/* (Point::getCloseViewObs / LineSeg::getCloseViewObs, src/feature3D.cpp:80-125, called at      */
/* src/matcher.cpp:165, :239) and the order cell.sort(pointQualityComparator) leaves in every   */
/* cell (:219-276), for a batch of independent streams (one wave per stream).   */
/* The map tables are staged once and stay on the device; a frame costs a pose and an overlap   */
/* list; the result is handed to the direct matcher without leaving the device.                 */
/* ------------------------------------------------------------------------------------------ */

#define PLSVO_LM_DELETED   0        /* Point::TYPE_DELETED < TYPE_CANDIDATE < TYPE_UNKNOWN < TYPE_GOOD (include/plsvo/feature3D.h:55-59), */
#define PLSVO_LM_CANDIDATE 1        /* and the same four of LineSeg */
#define PLSVO_LM_UNKNOWN   2
#define PLSVO_LM_GOOD      3

/* One stream's map tables (a keyframe restages them; between keyframes plsvo_candidates_select changes types and lists in place).
 *   kf_T, kf_slot      7*n_kf, n_kf    Frame::T_f_w_ and the pyramid slot of every keyframe
 *   kf_pt_off          n_kf+1          CSR: keyframe k's pt_fts_ are entries [kf_pt_off[k], kf_pt_off[k+1]) of kf_pt_lm, in list order
 *   kf_pt_lm                           the point landmark of every feature (index < n_pt), -1 where feat3D == NULL
 *   kf_seg_off, kf_seg_lm              the same for seg_fts_ and the segment landmarks
 *   pt_pos, pt_type    3*n_pt, n_pt    Point::pos_, Point::type_ (PLSVO_LM_*)
 *   pt_obs_off         n_pt+1          CSR: Point::obs_ in list order (the reference pushes at the front; the list as it stands)
 *   pt_obs_kf ..                       per observation: index of Feature::frame in the keyframe table, px (2), f (3), level,
 *                                      type (PLSVO_FTR_*), PointFeat::grad (2; the array may be NULL without edgelets)
 *   seg_spos, seg_epos, seg_type       LineSeg::spos_, epos_, type_
 *   seg_obs_*                          LineFeat: frame, spx (2), epx (2), sf (3), ef (3), level
 *   pt_cand, seg_cand                  map_.point_candidates_ / map_.segment_candidates_ as landmark indices in list order
 * Preconditions: finite values, and no landmark at a camera centre it is seen from or at the new frame's (Eigen normalises a
 * zero vector to NaN; a finite non-zero direction is required). */
typedef struct plsvo_cand_map {
  int32_t n_kf;
  int32_t n_pt, n_seg;              /* landmarks */
  int32_t n_pt_cand, n_seg_cand;    /* entries of the map's candidate lists */
  int32_t reserved0;
  const double* kf_T;
  const int32_t* kf_slot;
  const int32_t* kf_pt_off;
  const int32_t* kf_pt_lm;
  const int32_t* kf_seg_off;
  const int32_t* kf_seg_lm;
  const double* pt_pos;
  const int32_t* pt_type;
  const int32_t* pt_obs_off;
  const int32_t* pt_obs_kf;
  const double* pt_obs_px;
  const double* pt_obs_f;
  const int32_t* pt_obs_level;
  const uint8_t* pt_obs_type;
  const double* pt_obs_grad;
  const double* seg_spos;
  const double* seg_epos;
  const int32_t* seg_type;
  const int32_t* seg_obs_off;
  const int32_t* seg_obs_kf;
  const double* seg_obs_spx;
  const double* seg_obs_epx;
  const double* seg_obs_sf;
  const double* seg_obs_ef;
  const int32_t* seg_obs_level;
  const int32_t* pt_cand;
  const int32_t* seg_cand;
} plsvo_cand_map;

typedef struct plsvo_cand_params {  /* one set for the batch */
  plsvo_pinhole cam;
  int32_t cell_size;                /* Config::gridSize(): the points' grid (reprojector.cpp:57-66) */
  int32_t seg_cell_size;            /* Config::gridSizeSegs(): the segments' grid (:68-79) */
  int32_t boundary;                 /* 8 (:393) */
  int32_t n_pyr_levels;             /* Config::nPyrLevels() (matcher) */
  int32_t align_max_iter;           /* Matcher::Options::align_max_iter (10) */
  int32_t reserved0;
} plsvo_cand_params;

/* One stream's new frame. */
typedef struct plsvo_cand_frame {
  double T_f_w[7];                  /* the frame's T_f_w_ after alignment */
  const double* d_T_f_w;            /* NULL, or a DEVICE pointer to 7 doubles read instead (as plsvo_kf_decide_in::d_T_new) */
  int32_t cur_slot;                 /* its pyramid slot */
  int32_t n_overlap;
  const int32_t* overlap_idx;       /* n_overlap indices into the keyframe table, in order (plsvo_close_kf_out.close_idx) */
} plsvo_cand_frame;

/* Results of one stream.  A landmark is FILED when its visit won (the first visit of a landmark in the order overlap rank, then
 * point features, then segment features of that keyframe; points and segments are separate landmark spaces) and its projection
 * is what plsvo_reproject accepts (both end points for a segment); the map's candidates follow in list order without the
 * first-visit test.  Filed landmarks come out in stable descending order of type_, within a type in filing order.
 * Caller buffers, any may be NULL; capacity n_pt + n_pt_cand points, n_seg + n_seg_cand segments, of which the first n_filed_*
 * are written (with a landmark reserve -- plsvo_candidates_reserve_landmarks -- the counts of CAPACITY: landmark rows as
 * plsvo_candidates_lm_capacity reports them plus the staged candidate count plus the same room). */
typedef struct plsvo_cand_out {
  int32_t n_filed_pt, n_filed_seg;
  int32_t* pt_lm;                   /* landmark index */
  double* pt_px;                    /* 2: the projection */
  int32_t* pt_cell;                 /* its grid cell */
  int32_t* pt_obs;                  /* position in the landmark's observation list of getCloseViewObs' choice; -1 for an empty list */
  uint8_t* pt_has_view;             /* getCloseViewObs' return value (0 for an empty list) */
  uint8_t* pt_active;               /* has_view and not TYPE_DELETED: refine() would call the matcher */
  int32_t* seg_lm;
  double* seg_px;                   /* 4: projected start point, end point */
  int32_t* seg_cell;                /* 2 */
  int32_t* seg_obs;
  uint8_t* seg_has_view;
  uint8_t* seg_active;
  int32_t* kf_count;                /* n_overlap: overlap_kfs[r].second (a segment counts once) */
  uint8_t* pt_cand_failed;          /* n_pt_cand: 1 where reproject() failed (n_failed_reproj_ += 3 and the deletion stay with the caller) */
  uint8_t* seg_cand_failed;         /* n_seg_cand */
} plsvo_cand_out;

/* The matcher's result for one stream's filed landmarks: n_filed_pt points, then the start points of the n_filed_seg segments,
 * then their end points, each in output order.  An entry with active == 0 reports found 0, its projection and search level -1.
 * Caller buffers of n_pt + n_pt_cand + 2 * (n_seg + n_seg_cand) entries, any may be NULL. */
typedef struct plsvo_cand_match_out {
  uint8_t* found;
  double* px;                       /* 2 */
  int32_t* search_level;
} plsvo_cand_match_out;

/* The candidate arrays on the device, in the layout of plsvo_match_in, for a later stage of a resident chain: stream s owns entries
 * [m_off[s], m_off[s] + cap) with cap = n_pt + n_pt_cand + 2 * (n_seg + n_seg_cand), of which the first n_filed_pt + 2 * n_filed_seg
 * are candidates ([points | start points | end points]) and the rest have active == 0; counts holds n_filed_pt, n_filed_seg per
 * stream.  Frame indices are global: stream s owns frames [f_off[s], f_off[s] + n_kf] -- its keyframes, then the new frame.
 * Valid from plsvo_candidates_run until the next stage or insertion (plsvo_candidates_stage, plsvo_candidates_insert_keyframe). */
typedef struct plsvo_cand_dev {
  int64_t n_entries, n_frames;
  const int64_t* m_off;             /* HOST arrays of n streams, owned by the context */
  const int64_t* f_off;
  const int32_t* d_counts;
  const double* d_frame_T; const int32_t* d_frame_slot;
  const int32_t* d_cur_frame; const int32_t* d_ref_frame;
  const double* d_ref_px; const double* d_ref_f; const int32_t* d_ref_level; const uint8_t* d_ref_type; const double* d_ref_grad;
  const double* d_pos; const double* d_px_cur; const uint8_t* d_active;
  const uint8_t* d_found; const double* d_px_out; const int32_t* d_search_level;   /* written by plsvo_candidates_match */
} plsvo_cand_dev;

/* stage: n streams' tables travel once.  run: enqueue only -- the frames' records travel, the first-visit words are re-armed, one
 * launch.  fetch: synchronises.  match: enqueue only -- Matcher::findMatchDirect (plsvo_match_direct's kernel, unchanged) on the
 * resident candidates; match_fetch synchronises.
 * PLSVO_E_INVALID (nothing written) for n < 0, NULL arguments with n > 0, a negative count, a NULL array with a non-zero count
 * (pt_obs_grad excepted), CSR offsets that do not start at 0 or decrease, a landmark, keyframe, candidate or overlap index out of
 * range, a type outside PLSVO_LM_* / PLSVO_FTR_*, a negative level or slot, non-positive cell sizes; run / fetch with another n
 * than staged.  PLSVO_E_STATE for run without stage, fetch without run, match_fetch without match, match without pyramids;
 * PLSVO_E_CAPACITY for a slot or level outside the configured pyramids at match. */
int plsvo_candidates_stage(plsvo_ctx* ctx, int n, const plsvo_cand_map* maps, const plsvo_cand_params* params);
int plsvo_candidates_run(plsvo_ctx* ctx, int n, const plsvo_cand_frame* frames);
int plsvo_candidates_fetch(plsvo_ctx* ctx, int n, plsvo_cand_out* out);
int plsvo_candidates_match(plsvo_ctx* ctx);
int plsvo_candidates_match_fetch(plsvo_ctx* ctx, int n, plsvo_cand_match_out* out);
int plsvo_candidates_dev(plsvo_ctx* ctx, plsvo_cand_dev* out);

/* ------------------------------------------------------------------------------------------ */
/* cell selection of the map candidates: the second half of Reprojector::reprojectMap           */
/* (src/reprojector.cpp:185-216) with refineBestCandidate (:236-276) and refine (:278-387), the  */
/* failures of setMapCandidates (:116-131) and the deletions they lead to (src/map.cpp:116-139,  */
/* :311-324, :403-416), in place on the resident tables of plsvo_candidates_stage (one wave per  */
/* stream).  Candidates, match, selection and pose optimisation of a frame are   */
/* one enqueue sequence; the tables stay what the reference's map would be from keyframe to      */
/* keyframe.                                                                                    */
/* Preconditions (unchecked): a landmark occurs at most once in a candidate list, and a landmark */
/* in a candidate list is referenced by no keyframe feature -- a point is then filed at most     */
/* once per frame.  The observation lists of a deleted landmark are left as staged (the          */
/* reference clears them; a deleted landmark is never matched).                                  */
/* ------------------------------------------------------------------------------------------ */

#define PLSVO_LM_EVENT_PROMOTED 1   /* TYPE_UNKNOWN -> TYPE_GOOD by the last selection (:306-307, :367-369) */
#define PLSVO_LM_EVENT_DELETED  2   /* -> TYPE_DELETED by the last selection (safeDelete*, deleteCandidate*) */

typedef struct plsvo_cand_select_params {   /* one set for the batch; the grids are those of the staged plsvo_cand_params */
  int32_t max_fts;                  /* Config::maxFts(): the visit stops after the match that makes n_matches_ exceed it (:195) */
  int32_t max_fts_segs;             /* Config::maxFtsSegs() (:205) */
  int32_t poseopt_n_iter;           /* 10 (src/config.cpp:103) */
  int32_t reserved0;
  const int32_t* cell_order;        /* ceil(width / cell_size) * ceil(height / cell_size) cell indices (Grid::cell_order, :63-66); NULL = 0,1,2,.. */
  const int32_t* seg_cell_order;    /* the same for the segments' grid (:76-79) */
  double reproj_thresh;             /* 2.0 (src/config.cpp:102) */
} plsvo_cand_select_params;

/* Point::n_failed_reproj_ / n_succeeded_reproj_ and LineSeg's (include/plsvo/feature3D.h), per landmark of one stream.  A NULL array
 * leaves those counters as they are.  They are zero after plsvo_candidates_stage. */
typedef struct plsvo_cand_quality_in {
  const int32_t* pt_n_failed; const int32_t* pt_n_succeeded;       /* n_pt */
  const int32_t* seg_n_failed; const int32_t* seg_n_succeeded;     /* n_seg */
} plsvo_cand_quality_in;

/* The quality state of one stream as it now stands.  Caller buffers, any may be NULL: n_pt / n_seg entries, the candidate lists
 * n_pt_cand / n_seg_cand of the STAGED counts, of which the first n_pt_cand / n_seg_cand reported here are written (an erased
 * candidate closes the list up).  With a landmark reserve size them from plsvo_candidates_lm_capacity: plsvo_candidates_add
 * lengthens the landmark arrays and the lists.  *_event: PLSVO_LM_EVENT_* of the last plsvo_candidates_select, 0 before the first; a keyframe
 * insertion behind that selection ORs its own bits in (PLSVO_LM_EVENT_JOINED, PLSVO_LM_EVENT_DELETED). */
typedef struct plsvo_cand_quality_out {
  int32_t n_pt_cand, n_seg_cand;
  int32_t* pt_n_failed; int32_t* pt_n_succeeded; int32_t* pt_type; uint8_t* pt_event;
  int32_t* seg_n_failed; int32_t* seg_n_succeeded; int32_t* seg_type; uint8_t* seg_event;
  int32_t* pt_cand; int32_t* seg_cand;
} plsvo_cand_quality_out;

/* The features the new frame received, in the order refine() adds them (:311-312, :373-374).  Caller buffers, any may be NULL:
 * capacity n_filed_pt points and 2 * n_filed_seg segments (a segment that wins both of its cells is a feature twice). */
typedef struct plsvo_cand_select_out {
  int32_t n_matches;                /* Reprojector::n_matches_: point features */
  int32_t n_ls_matches;             /* n_ls_matches_: segment features */
  int32_t n_trials;                 /* n_trials_, points and segments */
  int32_t reserved0;
  int32_t* pt_lm;                   /* landmark index */
  double* pt_px;                    /* 2: the refined pixel */
  int32_t* pt_level;                /* Matcher::search_level_ */
  uint8_t* pt_type;                 /* PLSVO_FTR_EDGELET when the reference observation is one (:319-327) */
  double* pt_grad;                  /* 2: normalize(A_cur_ref * ref grad) for an edgelet, (1, 0) otherwise (src/feature.cpp:56) */
  int32_t* seg_lm;
  double* seg_px;                   /* 4: refined start point, end point */
  int32_t* seg_level;               /* the END point's search level (src/matcher.cpp:264, :373) */
} plsvo_cand_select_out;

/* set_quality / fetch_quality: synchronous; valid from plsvo_candidates_stage on.
 * select: enqueue only -- the re-arm of the launch's scratch and one launch; PLSVO_E_STATE without a preceding plsvo_candidates_match
 * (or plsvo_candidates_set_match) on the last plsvo_candidates_run, or when that run was selected already.  It changes the resident tables: types, counters, the keyframes'
 * feature lists (-1 where safeDelete* cut the landmark loose) and the candidate lists, so the next plsvo_candidates_run sees the map the
 * reference would see.  select_fetch synchronises.
 * pose_optimize: enqueue only -- pose_optimizer::optimizeGaussNewton (plsvo_pose_optimize's kernels, unchanged) on the features the
 * selection wrote on the device, starting from the pose the candidate stage projected with; pose_fetch synchronises, its keep masks are in
 * selection order.  poses_dev: n*7 doubles, the optimised T_f_w, on the device (as plsvo_chain_poses_dev).
 * PLSVO_E_INVALID (nothing written) for another n than staged, NULL arguments with n > 0, negative max_fts / max_fts_segs /
 * poseopt_n_iter, a cell order that is not a permutation of its grid, a negative counter. */
int plsvo_candidates_set_quality(plsvo_ctx* ctx, int n, const plsvo_cand_quality_in* in);
int plsvo_candidates_fetch_quality(plsvo_ctx* ctx, int n, plsvo_cand_quality_out* out);
int plsvo_candidates_select(plsvo_ctx* ctx, const plsvo_cand_select_params* params);
int plsvo_candidates_select_fetch(plsvo_ctx* ctx, int n, plsvo_cand_select_out* out);
int plsvo_candidates_pose_optimize(plsvo_ctx* ctx);
int plsvo_candidates_pose_fetch(plsvo_ctx* ctx, int n, plsvo_poseopt_out* out);
const double* plsvo_candidates_poses_dev(plsvo_ctx* ctx);
/* Diagnostic (tests; like plsvo_hip_detect_stages for the detector): overwrites the resident match output of the last
 * plsvo_candidates_run with the caller's -- per stream n_filed_pt + 2 * n_filed_seg entries in the layout of plsvo_cand_match_out, all
 * three arrays required -- so that the selection can be driven with constructed match results.  Synchronous. */
int plsvo_candidates_set_match(plsvo_ctx* ctx, int n, const plsvo_cand_match_out* in);

/* ------------------------------------------------------------------------------------------ */
/* keyframe insertion: the frame of the last plsvo_candidates_run becomes a keyframe of the     */
/* resident tables, in place (one wave per stream).  It replaces, in this       */
/* order: the landmark a rejected feature loses (src/pose_optimizer.cpp:218, :239); addFrameRef  */
/* of every feature of the new frame, pushed at the FRONT of the landmark's list                */
/* (src/frame_handler_mono.cpp:358-369, include/plsvo/feature3D.h:202-206);                      */
/* MapPointCandidates::addCandidatePointToFrame and its segment twin (src/map.cpp:292-309,       */
/* :384-401): a candidate the new frame observes becomes TYPE_UNKNOWN with n_failed_reproj_ 0,   */
/* its original feature -- the LAST observation -- is appended to the feature list of that       */
/* observation's keyframe, the entry leaves the candidate list; Map::safeDeleteFrame with        */
/* removePtFrameRef / removeLsFrameRef (:53-114), safeDeletePoint / safeDeleteSegment (:116-139) */
/* and removeFrameCandidates (:326-340) when a keyframe is removed; Map::addKeyframe (:153-156). */
/* Keyframe identities are table indices: removing a keyframe closes the table up (every         */
/* *_obs_kf above remove_kf drops by one) and the new keyframe is the LAST row.                  */
/* Map::getFurthestKeyframe and the test map_.size() >= maxNKfs stay with the caller             */
/* (plsvo_keyframe_decide reports furthest_kf).                                                  */
/* Pinned where the reference leaves the result open:                                            */
/*  - a feature of the new frame whose landmark is TYPE_DELETED when the frame becomes a         */
/*    keyframe (a segment that won its first cell and was deleted by its failure in the second)  */
/*    has no landmark; the reference keeps a feature that points at a trashed landmark;          */
/*  - segment candidates of the removed keyframe are deleted and erased like point candidates;   */
/*    the reference (src/map.cpp:73) calls removeFrameCandidates for points only and leaves a    */
/*    segment candidate that observes a freed frame;                                             */
/*  - Frame::key_pts_ (removeKeyPoint) are not in THESE tables: the deleted landmarks are        */
/*    reported as events and the removed keyframe is the caller's own argument.  They are a      */
/*    table of their own beside them once plsvo_candidates_set_keypts has made it live (below,   */
/*    "keyframe stage on the resident tables"): then the insertion keeps it up in a launch of    */
/*    its own behind map_insert_kernel, which itself is what it was;                             */
/*  - the observation list of a landmark deleted HERE is emptied (the reference clears it); a    */
/*    landmark deleted earlier keeps its list, less the observations in the removed keyframe.    */
/* Preconditions (unchecked) as for the selection, and: a landmark in a candidate list has       */
/* exactly one observation; every feature of a keyframe that holds a landmark has an observation */
/* of that landmark in that keyframe.                                                            */
/* ------------------------------------------------------------------------------------------ */

#define PLSVO_LM_EVENT_JOINED   4   /* a candidate whose original feature joined its keyframe (TYPE_CANDIDATE -> TYPE_UNKNOWN) by the last insertion */

/* Room per stream beyond what is staged, added by the NEXT and every later plsvo_candidates_stage to each stream's sizes: the
 * per-stream offsets are then laid out by capacity instead of by count (the matcher's frame table and kf_pos too), so a stream's
 * rows never move.  NULL or all zeros: the tight layout -- every result, offset and byte is what it is without this call. */
typedef struct plsvo_cand_reserve {
  int32_t extra_kf;                 /* keyframes */
  int32_t extra_kf_pt, extra_kf_seg;   /* entries of the keyframes' feature lists */
  int32_t extra_pt_obs, extra_seg_obs; /* observations */
  int32_t reserved0;
} plsvo_cand_reserve;

#define PLSVO_INSERT_POSE_HOST     0   /* T_f_w */
#define PLSVO_INSERT_POSE_DEV      1   /* d_T_f_w: a DEVICE pointer to 7 doubles */
#define PLSVO_INSERT_POSE_RESIDENT 2   /* the optimised pose of plsvo_candidates_pose_optimize, on the device */

/* One stream's insertion: about 100 bytes. */
typedef struct plsvo_cand_insert {
  int32_t is_kf;                    /* 0: this stream is not touched at all */
  int32_t remove_kf;                /* -1, or the table index of the keyframe Map::safeDeleteFrame removes */
  int32_t kf_slot;                  /* the new keyframe's pyramid slot */
  int32_t pose_source;              /* PLSVO_INSERT_POSE_* */
  double T_f_w[7];
  const double* d_T_f_w;
  const uint8_t* pt_keep;           /* HOST keep masks in selection order (n_matches / n_ls_matches entries), or NULL: the resident */
  const uint8_t* seg_keep;          /* masks of plsvo_candidates_pose_optimize */
} plsvo_cand_insert;

/* What an insertion did to one stream (zeros for a stream with is_kf == 0, except n_kf and the sizes, which are reported as they stand). */
typedef struct plsvo_cand_insert_out {
  int32_t n_kf;                     /* keyframes in the table now */
  int32_t new_kf;                   /* the new keyframe's index (n_kf - 1), -1 for a stream that did not insert */
  int32_t n_kf_pt, n_kf_seg;        /* used sizes: entries of the keyframes' feature lists */
  int32_t n_pt_obs, n_seg_obs;      /* observations */
  int32_t n_pt_cand, n_seg_cand;    /* the candidate lists */
  int32_t n_joined_pt, n_joined_seg;     /* candidates that joined */
  int32_t n_deleted_pt, n_deleted_seg;   /* landmarks deleted by the insertion */
} plsvo_cand_insert_out;

/* The resident tables of one stream as they now stand, in plsvo_cand_map's layout.  Caller buffers, any may be NULL, of the stream's
 * CAPACITY as plsvo_candidates_capacity reports it (staged sizes plus the reserve in force at stage time; kf_T / kf_slot one row per
 * keyframe of capacity, offsets one more than their lists; landmark arrays n_pt / n_seg, candidate lists their staged counts -- with a
 * landmark reserve the rows plsvo_candidates_lm_capacity reports, the lists their staged counts plus the same room); the
 * counts are reported.  The library cannot see the buffers' sizes: smaller ones are overrun. */
typedef struct plsvo_cand_map_out {
  int32_t n_kf, n_pt, n_seg, n_pt_cand, n_seg_cand;
  int32_t n_kf_pt, n_kf_seg, n_pt_obs, n_seg_obs;
  int32_t reserved0;
  double* kf_T; int32_t* kf_slot; int32_t* kf_pt_off; int32_t* kf_pt_lm; int32_t* kf_seg_off; int32_t* kf_seg_lm;
  double* pt_pos; int32_t* pt_type; int32_t* pt_obs_off; int32_t* pt_obs_kf; double* pt_obs_px; double* pt_obs_f; int32_t* pt_obs_level; uint8_t* pt_obs_type; double* pt_obs_grad;
  double* seg_spos; double* seg_epos; int32_t* seg_type; int32_t* seg_obs_off; int32_t* seg_obs_kf; double* seg_obs_spx; double* seg_obs_epx; double* seg_obs_sf; double* seg_obs_ef;
  int32_t* seg_obs_level;
  int32_t* pt_cand; int32_t* seg_cand;
} plsvo_cand_map_out;

/* Landmark positions the caller has moved (FrameHandlerBase::optimizeStructure, src/frame_handler_mono.cpp:340): Point::pos_ of
 * n_pt listed points, LineSeg::spos_ / epos_ of n_seg listed segments.  A landmark listed twice in one call ends with either of its
 * positions (one thread writes each entry, unordered): list a landmark once. */
typedef struct plsvo_cand_positions {
  int32_t n_pt, n_seg;
  const int32_t* pt_idx; const double* pt_pos;                           /* n_pt, 3*n_pt */
  const int32_t* seg_idx; const double* seg_spos; const double* seg_epos; /* n_seg, 3*n_seg each */
} plsvo_cand_positions;

/* reserve: host only; PLSVO_E_INVALID for a negative field.
 * insert_keyframe: SYNCHRONISES -- the caller has just waited for the keyframe decision.  A planning launch writes scratch only and a
 * few integers per stream come back; capacity is decided before anything is changed: if any inserting stream's new sizes (keyframes,
 * features per kind, observations per kind) exceed its room the call returns PLSVO_E_CAPACITY and EVERY stream's tables are what they
 * were.  Then one launch changes the tables of the inserting streams; nothing but the per-stream records (and host keep masks) crosses
 * the bus.  Afterwards the next plsvo_candidates_run / _match / _select / _pose_optimize work on the new tables; overlap indices are
 * validated against the new keyframe count.  The insertion ORs PLSVO_LM_EVENT_JOINED / PLSVO_LM_EVENT_DELETED into the event bytes
 * plsvo_candidates_fetch_quality reports; it does not clear the selection's bits.
 * PLSVO_E_STATE: no selection on the last run; NULL masks or PLSVO_INSERT_POSE_RESIDENT without a resident pose optimisation; a second
 * insertion on the same run.  PLSVO_E_INVALID (nothing written): another n than staged, NULL in with n > 0, remove_kf outside the
 * table, a negative slot, an unknown pose source, PLSVO_INSERT_POSE_DEV without a pointer.
 * After an insertion the run it closed is over: plsvo_candidates_match / _set_match / _select / _pose_optimize / _dev return PLSVO_E_STATE
 * until the next plsvo_candidates_run (their inputs index the tables as they were); the run's fetches (plsvo_candidates_fetch,
 * _match_fetch, _select_fetch, _pose_fetch, _poses_dev) still return its results, whose observation and keyframe indices refer to the
 * tables BEFORE the insertion.
 * capacity: per stream the room its rows were laid out with at stage time (staged sizes plus the reserve in force THEN; a later
 * plsvo_candidates_reserve does not change it), in the fields of plsvo_cand_reserve: keyframes, feature entries per kind, observations per
 * kind.  These are the buffer sizes plsvo_candidates_fetch_map needs.
 * insert_fetch: what the last insertion did; PLSVO_E_STATE before the first one since the tables were staged.
 * fetch_map: synchronous, valid from plsvo_candidates_stage on.
 * set_positions: a host-fed scatter into the resident landmark tables, enqueue-only after the copy of the lists; PLSVO_E_INVALID
 * (nothing written) for an index outside the stream's landmarks, a negative count or a NULL array with a non-zero count. */
int plsvo_candidates_reserve(plsvo_ctx* ctx, const plsvo_cand_reserve* reserve);
int plsvo_candidates_insert_keyframe(plsvo_ctx* ctx, int n, const plsvo_cand_insert* in);
int plsvo_candidates_capacity(plsvo_ctx* ctx, int n, plsvo_cand_reserve* out);
int plsvo_candidates_insert_fetch(plsvo_ctx* ctx, int n, plsvo_cand_insert_out* out);
int plsvo_candidates_fetch_map(plsvo_ctx* ctx, int n, plsvo_cand_map_out* out);
int plsvo_candidates_set_positions(plsvo_ctx* ctx, int n, const plsvo_cand_positions* in);

/* ------------------------------------------------------------------------------------------ */
/* structure optimisation on the resident tables: FrameHandlerBase::optimizeStructure           */
/* (src/frame_handler_base.cpp:192-237, called at src/frame_handler_mono.cpp:340 on every        */
/* tracked frame), in place (one wave per stream).  Among the features of the    */
/* last selection whose keep byte is set (feat3D != NULL behind the pose optimiser's cull) the   */
/* min(max_n, count) landmarks with the smallest last_structure_optim_ are refined by            */
/* Point::optimize / LineSeg::optimize (plsvo_structure_optimize's arithmetic, bit for bit) on   */
/* the resident keyframe poses and observation lists; their positions are written in place and   */
/* their last_structure_optim_ becomes frame_id, also when the optimiser rolled back (:221).     */
/* The new frame is no keyframe yet and is in no observation list.  A segment that won both of   */
/* its cells is a feature twice, is in the reference's deque twice and, selected twice, is       */
/* optimised twice in sequence.                                                                  */
/* Pinned where the reference leaves the result open: std::nth_element does not say which of     */
/* several equal keys at the cut are taken -- ties go to the EARLIER feature (signed 32-bit      */
/* keys; with count <= max_n every entry is taken).  The selected entries are reported in        */
/* feature order.                                                                                */
/* last_structure_optim_ is one int32 per landmark row, zero after plsvo_candidates_stage and    */
/* for every row first used later (plsvo_candidates_add, a converged seed), as the reference's   */
/* constructors set it; a keyframe insertion leaves it alone.                                    */
/* Preconditions (unchecked): a feature's landmark is never TYPE_DELETED here (a landmark        */
/* receives a feature only when its refine succeeded in that selection); point features are      */
/* distinct landmarks.                                                                           */
/* ------------------------------------------------------------------------------------------ */

typedef struct plsvo_cand_structopt_params {   /* one set for the batch; the reference's 20 / 5 / 20 / 5 (src/config.cpp:105-108) */
  int32_t max_n_pts;                /* structureoptim_max_pts */
  int32_t n_iter_pts;               /* structureoptim_num_iter */
  int32_t max_n_segs;               /* structureoptim_max_segs */
  int32_t n_iter_segs;              /* structureoptim_num_iter_segs */
} plsvo_cand_structopt_params;

typedef struct plsvo_cand_structopt {   /* one stream */
  int32_t active;                   /* 0: this stream is left alone (the reference skips the stage on a frame that failed earlier) */
  int32_t frame_id;                 /* Frame::id_ */
  const uint8_t* pt_keep;           /* HOST keep masks in selection order (n_matches / n_ls_matches entries), or NULL: the resident */
  const uint8_t* seg_keep;          /* masks of plsvo_candidates_pose_optimize */
} plsvo_cand_structopt;

/* What the last call did to one stream.  Caller buffers (3 doubles per position), any may be NULL; cap_pt / cap_seg are INPUTS: the
 * entries each non-NULL point / segment buffer holds.  max_n_pts / max_n_segs of the call always suffice. */
typedef struct plsvo_cand_structopt_out {
  int32_t n_sel_pt, n_sel_seg;      /* selected entries (0 for an inactive stream) */
  int32_t cap_pt, cap_seg;          /* in: capacity of the caller's point / segment buffers, in entries */
  int32_t* pt_lm;                   /* landmark index, in feature order */
  int32_t* pt_iters;                /* residual evaluations executed (plsvo_structopt_out's pt_iters) */
  double* pt_pos;                   /* the position behind the entry's run */
  int32_t* seg_lm; int32_t* seg_iters; double* seg_spos; double* seg_epos;   /* a segment listed twice: the second entry holds the final position */
} plsvo_cand_structopt_out;

/* last_structure_optim_ per landmark of one stream (n_pt / n_seg entries).  A NULL array is skipped. */
typedef struct plsvo_cand_last_optim_in { const int32_t* pt_last_optim; const int32_t* seg_last_optim; } plsvo_cand_last_optim_in;
typedef struct plsvo_cand_last_optim_out { int32_t* pt_last_optim; int32_t* seg_last_optim; } plsvo_cand_last_optim_out;

/* optimize_structure: enqueue only, apart from the copy of the records and of host masks (which waits for the selection's counts); timed
 * under PLSVO_K_STRUCTOPT.  Its place in a run: after plsvo_candidates_pose_optimize, before plsvo_candidates_insert_keyframe; the next
 * plsvo_candidates_run projects with the moved positions.  PLSVO_E_STATE: no selection on the last run; NULL masks of an active stream
 * without a resident pose optimisation; a second call on the same run (the keys have moved on); the run closed by an insertion or an add;
 * an unfetched seed update pending.  PLSVO_E_INVALID (nothing written): another n than staged, NULL arguments with n > 0, NULL params, a
 * negative cap or iteration count.
 * structure_fetch: synchronises; PLSVO_E_STATE before the first optimize_structure since the tables were staged; PLSVO_E_INVALID, no
 * buffer of any stream written, when a stream selected more entries than the capacity it gives for a non-NULL buffer (the counts of
 * every stream are reported all the same, so the caller can size the buffers and fetch again).  A caller that follows the map needs
 * these few hundred bytes and no table fetch.
 * set_last_optim / fetch_last_optim: synchronous, valid from plsvo_candidates_stage on (PLSVO_E_STATE with an unfetched seed update
 * pending): they let a caller that restages carry the keys over. */
int plsvo_candidates_optimize_structure(plsvo_ctx* ctx, int n, const plsvo_cand_structopt* in, const plsvo_cand_structopt_params* params);
int plsvo_candidates_structure_fetch(plsvo_ctx* ctx, int n, plsvo_cand_structopt_out* out);
int plsvo_candidates_set_last_optim(plsvo_ctx* ctx, int n, const plsvo_cand_last_optim_in* in);
int plsvo_candidates_fetch_last_optim(plsvo_ctx* ctx, int n, plsvo_cand_last_optim_out* out);

/* ------------------------------------------------------------------------------------------ */
/* new map candidates: a depth-filter seed that converged becomes a landmark of the resident    */
/* tables, in place (one wave per stream).  It replaces what                    */
/* DepthFilter::updatePointSeeds / updateLineSeeds do with a converged seed                     */
/* (src/depth_filter.cpp:334-355, :439-462): `new Point(xyz_world, ftr)` /                      */
/* `new LineSeg(xyz_world_s, xyz_world_e, ftr)`, whose constructors (src/point.cpp:41-55,       */
/* :198-212) push the seed's feature as the landmark's ONE observation and set both             */
/* reprojection counters to 0, and the callbacks MapPointCandidates::newCandidatePoint /        */
/* MapSegmentCandidates::newCandidateSegment (src/map.cpp:285-290, :377-382, bound at           */
/* src/frame_handler_mono.cpp:88-95): type_ = TYPE_CANDIDATE and a push_back onto the map's     */
/* candidate list.  The seed's feature is not in its keyframe's feature list until the          */
/* candidate joins (addCandidatePointToFrame) -- what the resident tables assume of a candidate. */
/* Within a kind, input order = landmark index order = candidate-list order; points and         */
/* segments are separate landmark spaces.  The callbacks' depth_sigma2 arguments are unused by  */
/* the reference and are not part of this interface.  The landmark's position is an INPUT: the  */
/* pt_xyz_world / seg_xyz_world_s / _e plsvo_update_seeds reports, passed through unchanged.    */
/* A landmark deleted later keeps its row until plsvo_candidates_compact (below) reclaims it.    */
/* ------------------------------------------------------------------------------------------ */

#define PLSVO_LM_EVENT_NEW      8   /* a landmark appended by plsvo_candidates_add since the last selection */

/* Landmark rows per stream beyond what is staged, added by the NEXT and every later plsvo_candidates_stage: with room here a stream's
 * landmark rows and every per-landmark array, its candidate lists (staged count + extra), its filed / matcher rows
 * ((n_pt + extra_pt) + (n_pt_cand + extra_pt), likewise for segments) and its first-visit rows are laid out by capacity.  Each new
 * landmark also needs one observation entry: plsvo_cand_reserve's extra_pt_obs / extra_seg_obs; the two reserves combine.  NULL or
 * all zeros: every result, offset and byte is what it is without this call. */
typedef struct plsvo_cand_lm_reserve {
  int32_t extra_pt, extra_seg;
} plsvo_cand_lm_reserve;

/* One stream's new candidate landmarks: about 100 bytes per point and 200 per segment travel. */
typedef struct plsvo_cand_new {
  int32_t n_pt, n_seg;
  const double* pt_pos;             /* 3: Point::pos_ */
  const int32_t* pt_obs_kf;         /* the keyframe (table index as it stands now) of the seed's feature */
  const double* pt_obs_px;          /* 2 */
  const double* pt_obs_f;           /* 3 */
  const int32_t* pt_obs_level;
  const uint8_t* pt_obs_type;       /* PLSVO_FTR_* */
  const double* pt_obs_grad;        /* 2; may be NULL without edgelets (zeros are stored) */
  const double* seg_spos;           /* 3: LineSeg::spos_ */
  const double* seg_epos;           /* 3 */
  const int32_t* seg_obs_kf;
  const double* seg_obs_spx;        /* 2 */
  const double* seg_obs_epx;        /* 2 */
  const double* seg_obs_sf;         /* 3 */
  const double* seg_obs_ef;         /* 3 */
  const int32_t* seg_obs_level;
} plsvo_cand_new;

/* What the last plsvo_candidates_add did to one stream, and its sizes as they stand. */
typedef struct plsvo_cand_add_out {
  int32_t first_pt, first_seg;      /* index of the first new landmark per kind, -1 for none */
  int32_t n_added_pt, n_added_seg;
  int32_t n_pt, n_seg, n_pt_cand, n_seg_cand, n_pt_obs, n_seg_obs;
} plsvo_cand_add_out;

/* reserve_landmarks: host only; PLSVO_E_INVALID for a negative field.
 * lm_capacity: per stream the landmark rows its layout was made with at stage time (staged counts plus the reserve in force THEN), in
 * the fields of plsvo_cand_lm_reserve; its candidate lists hold the staged count plus the same room.  These are the sizes the
 * per-landmark buffers of plsvo_candidates_fetch_map, _fetch_quality and _set_quality need (set_quality reads, fetch_quality writes the
 * landmarks as they stand now).  PLSVO_E_STATE before a stage.
 * add: enqueue-only after the copy of the records.  Every check runs on the host before anything is written to any stream's tables:
 * PLSVO_E_INVALID for another n than staged, NULL in with n > 0, a negative count, a NULL array with a non-zero count (pt_obs_grad
 * excepted), an observation keyframe outside [0, n_kf) of the stream's table as it stands now, a level outside
 * [0, PLSVO_MAX_LEVELS), an unknown feature type, an edgelet without pt_obs_grad; PLSVO_E_CAPACITY when any stream lacks landmark rows
 * or observation entries of either kind (capacity is decided from the host's mirrors: no planning launch, no read-back);
 * PLSVO_E_STATE before a stage.  The new event bytes are PLSVO_LM_EVENT_NEW until the next selection clears them.
 * An add ends the open run as an insertion does: plsvo_candidates_match / _set_match / _select / _pose_optimize / _dev and
 * plsvo_candidates_insert_keyframe return PLSVO_E_STATE until the next plsvo_candidates_run; the run's fetches keep returning its
 * results (they index landmarks below the old counts, which have not moved).  An add after an insertion on the same run and several
 * adds in a row are legal.
 * add_fetch: synchronises; PLSVO_E_STATE before the first add since the tables were staged. */
int plsvo_candidates_reserve_landmarks(plsvo_ctx* ctx, const plsvo_cand_lm_reserve* reserve);
int plsvo_candidates_lm_capacity(plsvo_ctx* ctx, int n, plsvo_cand_lm_reserve* out);
int plsvo_candidates_add(plsvo_ctx* ctx, int n, const plsvo_cand_new* in);
int plsvo_candidates_add_fetch(plsvo_ctx* ctx, int n, plsvo_cand_add_out* out);

/* ------------------------------------------------------------------------------------------ */
/* compaction of the resident map tables: the landmark rows whose type is PLSVO_LM_DELETED      */
/* leave, in place (one wave per stream).  It is what Map::emptyTrash           */
/* (src/map.cpp:259-275) does for the reference's heap: list surgery, no arithmetic.  Per kind  */
/* (points and segments are separate landmark spaces) the live rows close up in a stable way -- */
/* remap[old] = number of live rows below old, -1 for a deleted row -- and everything of a row  */
/* moves with it bit for bit: position(s), type, n_failed_reproj_, n_succeeded_reproj_, the     */
/* event byte, the last_structure_optim_ key, the observation list.  The observation arrays     */
/* hold the live rows' lists in row order (a deleted row's list, emptied or left over, is       */
/* dropped), the keyframes' feature lists and the candidate lists are rewritten through the     */
/* remap.  Pinned where a precondition of the tables could be broken: a keyframe feature that   */
/* points at a deleted row becomes -1 (safeDelete*'s ftr->feat3D = NULL), a candidate entry     */
/* that does is erased by a stable compaction of its list (deleteCandidate*); both are counted. */
/* A freed row reads as one that was never used (its last_structure_optim_ key is 0).  Keyframe */
/* rows, feature-list lengths and order, -1 features and the seed tables do not change.  Order  */
/* is kept everywhere, so no result of any later frame changes.                                 */
/* ------------------------------------------------------------------------------------------ */

#define PLSVO_COMPACT_STANDBY  0    /* the stream is untouched, byte for byte */
#define PLSVO_COMPACT_ALWAYS   1
#define PLSVO_COMPACT_ROOM     2    /* a kind is compacted only where rows - n_landmarks < min_room: decided on the device, per kind */

typedef struct plsvo_cand_compact {
  int32_t mode;                     /* PLSVO_COMPACT_* */
  int32_t min_room_pt, min_room_seg;
  int32_t reserved0;
} plsvo_cand_compact;

/* What the last plsvo_candidates_compact did to one stream. */
typedef struct plsvo_cand_compact_out {
  int32_t ran_pt, ran_seg;          /* 1: the kind was compacted (also when no row of it was deleted) */
  int32_t n_pt_before, n_pt_after, n_seg_before, n_seg_after;
  int32_t n_pt_obs_before, n_pt_obs_after, n_seg_obs_before, n_seg_obs_after;
  int32_t n_pt_cand_before, n_pt_cand_after, n_seg_cand_before, n_seg_cand_after;
  int32_t n_repointed_pt, n_repointed_seg;       /* keyframe features that pointed at a deleted row */
  int32_t n_erased_pt_cand, n_erased_seg_cand;   /* candidate entries that did */
  int32_t* pt_remap;                /* n_pt_before entries, may be NULL; the identity where the kind did not run */
  int32_t* seg_remap;               /* n_seg_before entries, may be NULL */
} plsvo_cand_compact_out;

/* compact: one launch (timed under PLSVO_K_INSERT) and one synchronisation, like the insertion; the host's mirrors (landmark counts,
 * used observation entries, candidate counts) describe the new tables afterwards, so the capacity checks of plsvo_candidates_add, the
 * insertion, _fetch_map, _fetch_quality, _set_quality and plsvo_seeds_keyframe see the new sizes, and a repeated plsvo_seeds_update
 * finds the room on the device.  Every check runs before anything is written: PLSVO_E_INVALID for another n than staged, NULL in with
 * n > 0, an unknown mode, a negative threshold; PLSVO_E_STATE before a stage and between plsvo_seeds_update and its fetch.  A compaction
 * ends the open run as an add and an insertion do (plsvo_candidates_match / _set_match / _select / _pose_optimize / _dev /
 * _optimize_structure / _insert_keyframe return PLSVO_E_STATE until the next plsvo_candidates_run); the closed run's fetches keep
 * returning its results, in the OLD row numbers.  It is legal behind an insertion and behind adds.
 * compact_fetch: host only unless a remap is asked for; valid until the next call that moves the tables (a stage, an insertion, an add,
 * a seed update, another compaction), PLSVO_E_STATE afterwards and before the first compaction. */
int plsvo_candidates_compact(plsvo_ctx* ctx, int n, const plsvo_cand_compact* in);
int plsvo_candidates_compact_fetch(plsvo_ctx* ctx, int n, plsvo_cand_compact_out* out);

/* ------------------------------------------------------------------------------------------ */
/* keyframe stage on the resident tables: Frame::key_pts_ as a resident table, and              */
/* Map::getCloseKeyframes with the sort and the cut of Reprojector::reprojectMap                */
/* (src/map.cpp:158-179, src/reprojector.cpp:147-163) on it, feeding the candidate stage        */
/* without the host (one wave per stream).  The key-point table holds five      */
/* int32 per keyframe row of capacity: the POSITION of key_pts_[k] in that keyframe's           */
/* point-feature list (kf_pt_lm's CSR), -1 = NULL.  A feature's px is the observation of its    */
/* landmark whose pt_obs_kf is the keyframe (the insertion's precondition: it exists).          */
/* While the table is live, each entry point that changes the keyframes' feature lists keeps    */
/* it up in a small launch of its own behind its kernel:                                        */
/*  - plsvo_candidates_select: for every keyframe one of whose holders has lost its landmark     */
/*    (Map::safeDeletePoint -> Frame::removeKeyPoint, src/map.cpp:116-123, src/frame.cpp:143-154) */
/*    the NULL holders are dropped and Frame::setKeyPoints (:87-141) runs over the features that  */
/*    hold a landmark, in list order, the surviving holders staying unless a feature is strictly  */
/*    better (slots 3 and 4 compare x with cv, as the reference does);                           */
/*  - plsvo_candidates_insert_keyframe: the rows close up over remove_kf, the keyframes that     */
/*    lost a holder during the removal are rebuilt in the same way, and the new keyframe's row   */
/*    is the key points of this run's plsvo_candidates_keyframe_decide (positions in selection   */
/*    order), or, without one, setKeyPoints from five NULLs over its features that hold a        */
/*    landmark after the insertion.  Features that joined a keyframe are ordinary features       */
/*    from then on: only a rebuild picks them up;                                                */
/*  - plsvo_candidates_compact moves landmark rows, not feature positions: nothing to do;         */
/*  - plsvo_candidates_stage drops the table: call plsvo_candidates_set_keypts again.             */
/* Pinned where the device's form differs from the reference's:                                 */
/*  - the device sees a launch's deletions at once, the reference one by one.  A keyframe is     */
/*    rebuilt if and only if one of the deleted features was a holder when the launch began;     */
/*    afterwards every slot holds the best of the surviving features, a surviving holder winning  */
/*    ties, the lowest position among equal features.  The event-by-event form can differ only   */
/*    when two distinct features tie EXACTLY in a slot's value after an intermediate promotion    */
/*    (a feature G that is strictly better than a slot's surviving holder H takes the slot in    */
/*    the rebuild after the first deletion and is deleted itself later in the same launch; the   */
/*    reference's next rebuild fills the empty slot with the FIRST feature of H's value, which   */
/*    is another feature E when E ties with H exactly and stands before it; here H stays);       */
/*  - a holder position outside its keyframe's feature list counts as NULL.                      */
/* ------------------------------------------------------------------------------------------ */

/* One stream's key points: 5 * n_kf positions (-1 = NULL), or NULL: computed on the device by Frame::setKeyPoints from five NULLs over
 * each keyframe's features that hold a landmark -- what Frame::setKeyframe does to a fresh frame. */
typedef struct plsvo_cand_keypts {
  const int32_t* key_pts;
} plsvo_cand_keypts;

/* Caller buffer of 5 * keyframe CAPACITY entries (plsvo_candidates_capacity), or NULL: the first 5 * n_kf are the table, the rest -1. */
typedef struct plsvo_cand_keypts_out {
  int32_t* key_pts;
} plsvo_cand_keypts_out;

/* set_keypts: the staged keyframes get their key_pts_ and the table is LIVE from here to the next plsvo_candidates_stage; until it is
 * called every other entry point enqueues exactly what it enqueues without this section.  in == NULL: every stream as with a NULL
 * array.  Enqueue only: the caller's arrays are copied before it returns.
 * fetch_keypts: synchronous.
 * run_close: enqueue only.  plsvo_candidates_run with the overlap list decided on the device: `frames` are its records with
 * n_overlap == 0 and overlap_idx == NULL (the pose from T_f_w or d_T_f_w).  One launch per batch does getCloseKeyframes on the resident
 * kf_T, the live key-point table and the LIVE pt_pos of each key point's landmark, the stable sort by distance and the cut to
 * max_n_kfs, and writes the stream's overlap list and count where the candidate kernel reads them; the unchanged candidate launch
 * follows in the same enqueue.  plsvo_candidates_fetch's kf_count then needs n_kf entries per stream (those behind n_overlap are 0),
 * and every later stage of the run works with the device-decided list.
 * close_fetch: plsvo_close_kf_out per stream of the last run_close (close_idx / close_dist: buffers of n_kf entries or NULL); synchronises.
 * PLSVO_E_STATE: set_keypts without staged tables; fetch_keypts / run_close without a live table; close_fetch without a run_close as
 * the last run; any of them between plsvo_seeds_update and its fetch.  PLSVO_E_INVALID (nothing written): another n than staged, NULL
 * frames / out with n > 0, a key point below -1, a negative slot or max_n_kfs, a non-zero n_overlap or a non-NULL overlap_idx. */
int plsvo_candidates_set_keypts(plsvo_ctx* ctx, int n, const plsvo_cand_keypts* in);
int plsvo_candidates_fetch_keypts(plsvo_ctx* ctx, int n, plsvo_cand_keypts_out* out);
int plsvo_candidates_run_close(plsvo_ctx* ctx, int n, const plsvo_cand_frame* frames, int max_n_kfs);
int plsvo_candidates_close_fetch(plsvo_ctx* ctx, int n, plsvo_close_kf_out* out);

/* The keyframe decision on the resident selection: what plsvo_keyframe_decide computes with key_pts_prev all -1 -- getSceneDepth,
 * needNewKf, setKeyPoints, getFurthestKeyframe -- with every input read where it already lies on the device: the optimised pose
 * (plsvo_candidates_poses_dev), the new frame's features (the selection's f_pt_lm / f_pt_px / f_seg_lm) with the resident keep masks
 * as alive, the landmark positions FROM THE TABLES, not from the copy the selection gathered for the pose optimiser
 * (FrameHandlerBase::optimizeStructure, src/frame_handler_mono.cpp:340, runs before setKeyPoints / getSceneDepth, :351-352: a
 * plsvo_candidates_optimize_structure or _set_positions behind the selection is seen), kf_T and the run's resident overlap list (the
 * caller's of plsvo_candidates_run or the device's of plsvo_candidates_run_close).  Per stream only this record travels: */
typedef struct plsvo_cand_kf_decide {
  double T_last_w[7];               /* last_frame_->T_f_w_, which needNewKf measures from */
  const double* d_T_last_w;         /* NULL, or a DEVICE pointer to 7 doubles read instead */
  double kfselect_mindist_t;        /* Config::kfSelectMinDistT() */
  double kfselect_mindist_r;        /* Config::kfSelectMinDistR() */
  int32_t active;                   /* 0: the stream sits this call out; its record is what an earlier call of this run left (zeros before the first) */
  int32_t reserved0;
} plsvo_cand_kf_decide;

/* keyframe_decide: enqueue only, valid after plsvo_candidates_pose_optimize of a run, any number of times.  The decision records (56
 * bytes per stream) stay on the device: an insertion behind it, with a live key-point table, gives the new keyframe's row the decision's
 * key points (indices in selection order = positions in the new keyframe's feature list) instead of building it from five NULLs; a
 * key point whose feature the insertion leaves without a landmark is dropped and the row rebuilt, as for every other keyframe.
 * decide_fetch: synchronises; plsvo_kf_decide_out per stream, key_pts in selection order.  delta_t / delta_r are optional buffers of
 * n_overlap entries (after plsvo_candidates_run_close: of n_kf entries, the first n_overlap written); asking for them also brings the
 * deltas and the device-decided counts over the bus.
 * PLSVO_E_STATE: keyframe_decide before the pose optimisation of the last run or after an insertion, an add or a compaction closed it;
 * decide_fetch without a decision on the last run.  PLSVO_E_INVALID (nothing written): another n than staged, NULL in / out with n > 0. */
int plsvo_candidates_keyframe_decide(plsvo_ctx* ctx, int n, const plsvo_cand_kf_decide* in);
int plsvo_candidates_decide_fetch(plsvo_ctx* ctx, int n, plsvo_kf_decide_out* out);

/* ------------------------------------------------------------------------------------------ */
/* the next frame's alignment job from the resident selection, built on the device              */
/* replaces, per tracked frame, what the caller gathered on the host for                        */
/* SparseImgAlign::run(last_frame_, new_frame_) (src/frame_handler_mono.cpp:266-274): the       */
/* reference frame's features that still hold a landmark, f * ||pos_ - ref_frame->pos()||       */
/* (src/sparse_img_align.cpp:229-230, :327-330), LineFeat::length (src/feature.cpp:90), the      */
/* initial model (:80), and the patch-slot layout plsvo_align_stage computes on one host thread  */
/* (one wave per stream).  The reference frame is the frame the last run         */
/* tracked: its features are the last selection's, in selection order; a feature holds its       */
/* landmark when its keep byte is non-zero.                                                      */
/* PINNED: a feature whose landmark row is PLSVO_LM_DELETED at build time counts as              */
/* feat3D == NULL (Map::safeDeleteFrame, src/map.cpp:82-127, cuts such landmarks loose from the  */
/* new keyframe's features).  LEFT OUT: writing the alignment's cull back into a keyframe's own   */
/* segment features (src/sparse_img_align.cpp:687-688); the C++ adapter.  (A keyframe of the      */
/* tables as the reference frame is plsvo_candidates_align_build_kf below, the tracking-quality   */
/* gates, :315-321 and :335, plsvo_candidates_track_gate.)                                        */
/* ------------------------------------------------------------------------------------------ */

/* The resident alignment batch: per-stream CAPACITIES, by which its rows are laid out (stream s owns point rows from s * cap_pts,
 * segment rows from s * cap_seg, patch slots from s * slot_cap rounded up to 4), and SparseImgAlign's constructor arguments. */
typedef struct plsvo_cand_align_cfg {
  int32_t max_level, min_level;     /* src/sparse_img_align.cpp:40-52; levels of the configured pyramid */
  int32_t n_iter;                   /* 30 at the call sites */
  int32_t cap_pts, cap_seg;         /* kept point features / segment features (all of them, kept or not) of one stream */
  int32_t slot_cap;                 /* patch slots of one stream's largest level (plsvo_align_slot_layout's n_slots); at most 8064 */
  double eps;                       /* 1e-6 */
} plsvo_cand_align_cfg;

/* One stream's record of a build.  pose_source: PLSVO_INSERT_POSE_* -- where the reference frame's T_f_w is read (RESIDENT: the
 * optimised pose of plsvo_candidates_pose_optimize).  pt_keep / seg_keep: host masks in selection order (n_matches / n_ls_matches
 * bytes), or NULL for the pose optimiser's resident ones. */
typedef struct plsvo_cand_align_job {
  int32_t active;                   /* 0: the stream sits this build out; its job, poses and report are what an earlier build left (an empty job after the reserve) */
  int32_t ref_slot, cur_slot;       /* pyramid slots of the reference frame and of the frame to be aligned */
  int32_t pose_source;
  double T_f_w[7];
  const double* d_T_f_w;            /* a DEVICE pointer to 7 doubles (PLSVO_INSERT_POSE_DEV) */
  const uint8_t* pt_keep;
  const uint8_t* seg_keep;
} plsvo_cand_align_job;

#define PLSVO_ALIGN_JOB_OK      0
#define PLSVO_ALIGN_JOB_NO_ROOM 1   /* kept points > cap_pts, segments > cap_seg, a level's slots > slot_cap, or a segment of more than 2047 samples:
                                       the stream was dropped whole -- its job has no features and skip set, its composed pose is its reference pose */
typedef struct plsvo_cand_align_report {   /* 32 bytes per stream */
  int32_t n_pts, n_seg;             /* kept point features; segment features */
  int32_t n_seg_alive;              /* of those, the ones that hold a landmark */
  int32_t n_slots;                  /* patch slots of the finest level; 0 when the layout was not reached (cap_pts / cap_seg exceeded) or could not be made */
  int32_t long_mask;                /* bit l: level l has a segment of more than 64 samples */
  int32_t status;                   /* PLSVO_ALIGN_JOB_* */
  int32_t reserved0, reserved1;
} plsvo_cand_align_report;

/* Diagnostic view of one stream's built job (tests, like plsvo_align_fetch_records).  Every array is a caller buffer of the
 * CAPACITY'S size or NULL: pt_* cap_pts entries (2 / 3 doubles each), seg_* cap_seg, seg_code (max_level - min_level + 1) * cap_seg
 * int32, level-major from min_level (first slot | N << 20, or -1); the first n_pts / n_seg entries are written. */
typedef struct plsvo_cand_align_job_out {
  int32_t n_pts, n_seg, skip, long_mask;
  int32_t n_slots[PLSVO_MAX_LEVELS];
  int32_t ref_slot, cur_slot;
  int32_t n_patches;                /* the launch-order key of the stream's last build: points + samples summed over the levels */
  int32_t reserved0;
  double T0[7];                     /* the initial model T_cur_from_ref = T_ref * T_ref^-1 */
  double T_ref[7];                  /* the reference frame's T_f_w as the build read it */
  double T_f_w[7];                  /* the composed pose of the last plsvo_candidates_align_compose (the identity before the first) */
  double* pt_px; double* pt_xyz_ref;
  double* seg_spx; double* seg_epx; double* seg_len; double* seg_p_ref; double* seg_q_ref;
  uint8_t* seg_alive_in;
  int32_t* seg_code;
} plsvo_cand_align_job_out;

/* align_reserve: allocates the resident alignment batch for the staged streams (synchronous; every stream starts with an empty job).
 *   PLSVO_E_STATE without plsvo_candidates_stage or configured pyramids; PLSVO_E_INVALID for levels outside the configured pyramid,
 *   n_iter < 0, non-positive capacities, a camera other than the pyramids' level 0; PLSVO_E_CAPACITY for slot_cap > 8064 or slot tables beyond a
 *   workgroup's LDS in the shape a batch of the staged stream count launches with (few streams get many threads and more LDS per slot) or a batch beyond 2^31 rows.  A later plsvo_candidates_stage of another stream count drops it.
 * align_build: ENQUEUE ONLY with resident masks -- only the records travel (host masks cost one wait for the selection's counts).
 *   Its place is behind plsvo_candidates_pose_optimize, and behind _optimize_structure and _insert_keyframe (and _add) when the frame
 *   has them: it reads the landmark positions and types as they are then.  It must be ahead of plsvo_candidates_compact, which
 *   renumbers the rows the selection points at.  A successful build makes the built batch the context's STAGED ALIGNMENT BATCH,
 *   exactly as plsvo_align_stage would on the same inputs: it replaces a previously staged batch and invalidates a staged frame
 *   step; plsvo_align_run, _fetch, _poses_dev, _set_trace, _fetch_trace, _fetch_records, _chi2_ties, _work, _launch_order serve it
 *   unchanged.  The host's view of the batch holds the capacities: plsvo_align_fetch's seg_alive_out needs cap_seg bytes per stream
 *   (the first n_seg are the stream's), plsvo_align_fetch_records is bounded by slot_cap.  The first launch's order is most patches first
 *   (a stream that sat the build out counts with the patches of its last one); it is the order PLSVO_OPT_ALIGN_REORDER = 0 goes back to.
 *   PLSVO_E_STATE: no reserve (or one for another stream count); no selection on the last run; NULL masks or
 *   PLSVO_INSERT_POSE_RESIDENT without a resident pose optimisation; behind the run's compaction; between plsvo_seeds_update and its
 *   fetch.  PLSVO_E_INVALID (nothing enqueued): another n than staged, NULL jobs, an unknown pose source, PLSVO_INSERT_POSE_DEV
 *   without a pointer, a slot outside the pyramids.
 * align_compose: enqueue only, behind plsvo_align_run of the built batch: T_f_w(new) = T_cur_from_ref * T_ref per stream
 *   (src/sparse_img_align.cpp:92) into n * 7 doubles on the device.  PLSVO_E_STATE unless the staged alignment batch is the built one and has run.
 * align_poses_dev: that buffer (NULL before the first compose): what plsvo_cand_frame::d_T_f_w, plsvo_seed_frame::d_T_f_w and
 *   plsvo_cand_kf_decide::d_T_last_w take -- stream s at + 7 * s.
 * align_fetch: synchronises; the reports of the last build (a stream that sat it out: of its last one).
 * align_fetch_job: synchronises; PLSVO_E_INVALID for a stream outside the batch. */
int plsvo_candidates_align_reserve(plsvo_ctx* ctx, const plsvo_cand_align_cfg* cfg);
int plsvo_candidates_align_build(plsvo_ctx* ctx, int n, const plsvo_cand_align_job* jobs);
int plsvo_candidates_align_compose(plsvo_ctx* ctx);
const double* plsvo_candidates_align_poses_dev(plsvo_ctx* ctx);
int plsvo_candidates_align_fetch(plsvo_ctx* ctx, int n, plsvo_cand_align_report* out);
int plsvo_candidates_align_fetch_job(plsvo_ctx* ctx, int stream, plsvo_cand_align_job_out* out);

/* ------------------------------------------------------------------------------------------ */
/* the alignment job from a RESIDENT KEYFRAME as the reference frame           */
/* SparseImgAlign::run(ref_keyframe, new_frame_) of FrameHandlerMono::relocalizeFrame            */
/* (src/frame_handler_mono.cpp:408-436), its second alignment (last_frame_ = ref_keyframe;       */
/* processFrame(), :266-274) and the first frame of a sequence, with Map::getClosestKeyframe      */
/* (src/map.cpp:181-199) picking the row on request: one wave per stream writes the stream's     */
/* rows of the SAME resident alignment batch plsvo_candidates_align_reserve laid out, in the     */
/* same layout.  The keyframe's features are its lists in the tables (kf_pt_lm / kf_seg_lm); a    */
/* feature's px, f, sf, ef are those of the FIRST observation of its landmark whose obs_kf is     */
/* the keyframe (the pairing of the keyframe stage, also when a landmark is a feature of the      */
/* keyframe twice).  A point feature is kept when it has a landmark (>= 0) whose row is not       */
/* PLSVO_LM_DELETED (the pin of plsvo_candidates_align_build) and such an observation;            */
/* PLSVO_LM_CANDIDATE landmarks are kept (feat3D != NULL).  pt_xyz_ref is the STORED bearing      */
/* times ||pos - ref_pos|| ((*it)->f, src/sparse_img_align.cpp:229-230).  All segment features    */
/* are written, in order; PINNED: a dead one (the same three conditions) has no pixels in the     */
/* tables and gets zeros for pixels, length and the two vectors, seg_alive_in 0.                  */
/* relocalizeFrame ignores its T_cur_ref argument; that is restated as it is.                     */
/* LEFT OUT: writing the alignment's cull back into the keyframe's own segment features           */
/* (src/sparse_img_align.cpp:687-688); relocalizeFrameAtPose; processFirstFrame /                 */
/* processSecondFrame; the C++ adapter.                                                           */
/* ------------------------------------------------------------------------------------------ */
#define PLSVO_ALIGN_REF_CLOSEST (-1)  /* ref_kf: Map::getClosestKeyframe picks the row on the device */
#define PLSVO_ALIGN_INIT_HOST     0   /* T_init of the record (relocalizeFrame's first run(): new_frame_'s default-constructed T_f_w_, the identity) */
#define PLSVO_ALIGN_INIT_DEV      1   /* d_T_init */
#define PLSVO_ALIGN_INIT_KEYFRAME 2   /* the reference keyframe's own pose (:266 with last_frame_ = ref_keyframe): T0 = T_kf * T_kf^-1, not the literal
                                         identity; without a keyframe (PLSVO_ALIGN_JOB_NO_KEYFRAME) T_init of the record */
#define PLSVO_ALIGN_JOB_NO_KEYFRAME 2 /* plsvo_cand_align_report::status: PLSVO_ALIGN_REF_CLOSEST found no close keyframe (relocalizeFrame's
                                         "No reference keyframe", :413-417): an empty job with skip set whose reference pose, and so whose
                                         composed pose, is T_init */

/* One stream's record of a keyframe build.  T_last / d_T_last / last_source (PLSVO_INSERT_POSE_HOST or _DEV) and self_kf are read
 * for PLSVO_ALIGN_REF_CLOSEST only: last_frame_->T_f_w_, the pose getCloseKeyframes looks from, and the row of last_frame_ when it is
 * a keyframe of the table (else -1): the closest keyframe is the minimum by (distance, row) over the close keyframes other than
 * self_kf.  PINNED: with self_kf the only close keyframe the reference calls front() on an empty list; here that is "none". */
typedef struct plsvo_cand_align_kf_job {
  int32_t active;                   /* 0: the stream sits this build out, as in plsvo_cand_align_job */
  int32_t ref_kf;                   /* a keyframe row of the stream's table, or PLSVO_ALIGN_REF_CLOSEST */
  int32_t self_kf;
  int32_t cur_slot;                 /* pyramid slot of the frame to be aligned (the reference's is the keyframe's own) */
  int32_t init_source;              /* PLSVO_ALIGN_INIT_* */
  int32_t last_source;
  double T_init[7];
  double T_last[7];
  const double* d_T_init;           /* DEVICE pointers to 7 doubles */
  const double* d_T_last;
} plsvo_cand_align_kf_job;

/* align_build_kf: ENQUEUE ONLY; only the records travel.  It needs staged tables and the reserve -- no run, no selection, no pose
 *   optimisation -- and reads only the tables, so it is valid BEHIND plsvo_candidates_compact as well.  Like plsvo_candidates_align_build
 *   it makes the built batch the context's staged alignment batch, and the two compose on one batch: a stream active in one call sits
 *   the other out and keeps its rows, so tracking and relocalising streams run in ONE plsvo_align_run; plsvo_align_run, _fetch,
 *   plsvo_candidates_align_compose, _align_poses_dev, _align_fetch, _align_fetch_job serve the batch unchanged.  The report's
 *   reserved0 carries ref_kf + 1 (the row the job was built from; 0 for a build from the selection and for NO_KEYFRAME); NO_ROOM as in
 *   plsvo_candidates_align_build (a keyframe of more segment features than cap_seg is dropped before any scratch is used).
 *   PLSVO_E_STATE: no reserve (or one for another stream count); between plsvo_seeds_update and its fetch; PLSVO_ALIGN_REF_CLOSEST
 *   without a live key-point table (plsvo_candidates_set_keypts); the pyramids or the camera changed since the reserve.
 *   PLSVO_E_INVALID (nothing enqueued): another n than staged, NULL jobs, a row outside the stream's keyframes by the host's mirror (self_kf
 *   too), an unknown source, a source that needs a device pointer without one, cur_slot or the keyframe's slot outside the pyramids. */
int plsvo_candidates_align_build_kf(plsvo_ctx* ctx, int n, const plsvo_cand_align_kf_job* jobs);

/* ------------------------------------------------------------------------------------------ */
/* the tracking gates of a tracked frame, decided on the device                */
/* replaces, per tracked frame, the comparisons a caller made on fetched counts for             */
/* FrameHandlerMono::processFrame: "not enough matched features"                                */
/* (src/frame_handler_mono.cpp:315-321), fewer than 10 edges behind the pose optimisation        */
/* (:335), FrameHandlerBase::setTrackingQuality (src/frame_handler_base.cpp:173-190) and the     */
/* pose the frame carries forward (:318, :336; relocalizeFrame :432).  A lane per stream reads   */
/* the selection's n_matches / n_ls_matches and the pose optimiser's num_obs_pt / num_obs_ls     */
/* where they lie.  setTrackingQuality is restated literally: the segments' drop is computed and */
/* reported and decides nothing; :346-350 (TRACKING_INSUFFICIENT behind setTrackingQuality)      */
/* cannot be reached in the reference and is not built.                                          */
/* LEFT OUT: device-side masks that would let the later stages of a frame skip a failed stream   */
/* without the host (the caller fetches the 32-byte records ahead of the structure optimisation  */
/* and leaves such a stream out of the later calls); relocalizeFrameAtPose; processFirstFrame /  */
/* processSecondFrame; the C++ adapter.                                                          */
/* ------------------------------------------------------------------------------------------ */
#define PLSVO_GATE_TRACK 0            /* processFrame from STAGE_DEFAULT_FRAME */
#define PLSVO_GATE_RELOC 1            /* processFrame inside relocalizeFrame: every failure resets the pose (:432) */
#define PLSVO_GATE_OK           0
#define PLSVO_GATE_FAIL_MATCHES 1     /* n_matches + n_ls_matches < quality_min_fts (:315-321) */
#define PLSVO_GATE_FAIL_EDGES   2     /* num_obs_pt + num_obs_ls < 10 (:335) */
#define PLSVO_TRACKING_INSUFFICIENT 0 /* FrameHandlerBase::TrackingQuality, in its order */
#define PLSVO_TRACKING_BAD          1
#define PLSVO_TRACKING_GOOD         2
#define PLSVO_GATE_LAST_HOST     0    /* num_obs_last_pt / _ls of the record */
#define PLSVO_GATE_LAST_RESIDENT 1    /* the stream's counts of its last active gate since plsvo_candidates_stage */

/* One stream's record of a gate.  T_reset: last_frame_->T_f_w_ under PLSVO_GATE_TRACK, the last well localised pose under
 * PLSVO_GATE_RELOC; reset_source: PLSVO_INSERT_POSE_HOST (T_reset) or PLSVO_INSERT_POSE_DEV (d_T_reset). */
typedef struct plsvo_cand_gate {
  int32_t active;                   /* 0: the stream sits the call out; its record, carried pose and resident counts stay */
  int32_t mode;                     /* PLSVO_GATE_TRACK / _RELOC */
  int32_t quality_min_fts;          /* Config::qualityMinFts() (20) */
  int32_t quality_max_drop_fts;     /* int(Config::qualityMaxFtsDrop()) (50) */
  int32_t max_fts, max_fts_segs;    /* Config::maxFts(), Config::maxFtsSegs(): the clamps of the two drops */
  int32_t last_source;              /* PLSVO_GATE_LAST_* */
  int32_t num_obs_last_pt, num_obs_last_ls;   /* FrameHandlerBase::num_obs_last_pt / _ls (PLSVO_GATE_LAST_HOST) */
  int32_t reset_source;
  double T_reset[7];
  const double* d_T_reset;          /* a DEVICE pointer to 7 doubles */
} plsvo_cand_gate;

typedef struct plsvo_cand_gate_out {   /* 32 bytes per stream */
  int32_t result;                   /* PLSVO_GATE_* */
  int32_t tracking_quality;         /* PLSVO_TRACKING_*: INSUFFICIENT on either failure (finishFrameProcessingCommon), else setTrackingQuality's */
  int32_t n_matched;                /* n_matches + n_ls_matches */
  int32_t n_edges;                  /* num_obs_pt + num_obs_ls */
  int32_t drop_pt, drop_ls;         /* min(num_obs_last, max_fts) - num_obs, per kind */
  int32_t num_obs_last_pt, num_obs_last_ls;   /* the counts the drops were taken against */
} plsvo_cand_gate_out;

/* track_gate: ENQUEUE ONLY, behind plsvo_candidates_pose_optimize of a run, any number of times; only the records travel.  Per active
 *   stream it writes the 32-byte record, the pose carried forward (PLSVO_GATE_TRACK: FAIL_MATCHES gives T_reset, FAIL_EDGES and OK the
 *   optimised pose; PLSVO_GATE_RELOC: every failure gives T_reset) and the stream's resident num_obs_last_pt / _ls, which become this
 *   frame's n_matches / n_ls_matches whatever the result (Frame::nObs() is the size of the feature list).
 *   PLSVO_E_STATE: no resident pose optimisation on the last run; between plsvo_seeds_update and its fetch; PLSVO_GATE_LAST_RESIDENT
 *   before the first gate since plsvo_candidates_stage.  PLSVO_E_INVALID (nothing enqueued): another n than staged, NULL jobs, an
 *   unknown mode or source, PLSVO_INSERT_POSE_DEV without a pointer, a negative threshold, clamp or count.
 * gate_fetch: synchronises; the records (a stream that sat every call since the stage out reads as zeros) and, when poses is not NULL,
 *   the carried poses into n * 7 doubles.
 *   PLSVO_E_STATE without a gate since the stage; PLSVO_E_INVALID for another n or NULL out.
 * gate_poses_dev: the carried poses, n * 7 doubles on the device, stream s at + 7 * s (NULL before the first gate since the stage): what
 *   plsvo_cand_frame::d_T_f_w, plsvo_cand_align_job::d_T_f_w, plsvo_seed_frame::d_T_f_w, plsvo_cand_kf_decide::d_T_last_w and
 *   plsvo_cand_gate::d_T_reset take.  A stream that was never active holds zeros.  As d_T_reset of a gate it may alias only the
 *   stream's OWN row (+ 7 * s: each element is read and written by the same lane); another stream's row is written by that stream's
 *   lane in the same launch.  The buffer is laid out anew by the first gate behind a plsvo_candidates_stage: a pointer taken before
 *   the stage must not be used after it. */
int plsvo_candidates_track_gate(plsvo_ctx* ctx, int n, const plsvo_cand_gate* jobs);
int plsvo_candidates_gate_fetch(plsvo_ctx* ctx, int n, plsvo_cand_gate_out* out, double* poses);
const double* plsvo_candidates_gate_poses_dev(plsvo_ctx* ctx);

/* TUM-style trajectory record of a frame (app/run_pipeline.cpp:425-451): the camera pose in the world,
 * T_f_w^-1, as tx ty tz qx qy qz qw.  Returns 1 and fills out7 when the reference would write the line, 0 when
 * it skips the frame (a covariance entry outside (1e-16, 1e16), or an exactly-identity pose).  Host-only helper:
 * no device work, may be called with ctx == NULL. */
int plsvo_trajectory_record(const double T_f_w[7], const double cov[36], double out7[7]);

/* ------------------------------------------------------------------------------------------ */
/* depth-filter seed update (hot-path contract row (f) "next" #4, last item)                   */
/* replaces the per-seed bodies of DepthFilter::updatePointSeeds / updateLineSeeds             */
/* (src/depth_filter.cpp:270-365, :367-471) with everything they call:                         */
/* Matcher::findEpipolarMatchDirect (src/matcher.cpp:277-420) and                              */
/* findEpipolarMatchDirectSegmentEndpoint (:422-586), depthFromTriangulation (:133-146),       */
/* [ext] vk::patch_score::ZMSSD<4>, DepthFilter::computeTau (src/depth_filter.cpp:568-584),    */
/* updatePointSeed (:489-512), updateLineSeed (:514-566).                                      */
/* This call maps seed state -> seed state for lists the caller keeps: the batch-age test      */
/* (:289-292), the erasing and the converged-seed callbacks are the caller's.  plsvo_seeds_*   */
/* below keep the lists on the device.  The detector's grid occupancy stays on the host.       */
/* ------------------------------------------------------------------------------------------ */

#define PLSVO_SEED_NOT_VISIBLE 0    /* behind the camera or outside the image: unchanged (:296-304) */
#define PLSVO_SEED_NO_MATCH    1    /* epipolar search failed: b += 1 (:311-318) */
#define PLSVO_SEED_UPDATED     2    /* Bayesian update applied, seed stays */
#define PLSVO_SEED_CONVERGED   3    /* updated and sqrt(sigma2) < z_range/thresh: the host creates the landmark from xyz_world and removes the seed (:334-355) */
#define PLSVO_SEED_NAN         4    /* updated but z_inv_min was NaN: the host removes the seed (:356-360) */

/* float fields are the reference's float members of PointSeed / LineSeed (include/plsvo/depth_filter.h:60-96).
 * Point seed i: ref feature (frame pt_ref_frame[i], px, f, level, type, grad) + Beta/normal parameters.
 * Line seed i: Feature::px / f (what the reference hands to the end-point search for BOTH end points, :411-414),
 * LineFeat::sf / ef (used for visibility, tau and the landmark), level, and the two-ended parameters. */
typedef struct plsvo_seeds_in {
  plsvo_pinhole cam;
  int32_t n_pyr_levels;             /* Config::nPyrLevels() */
  int32_t align_max_iter;           /* Matcher::Options::align_max_iter (10) */
  int32_t max_epi_search_steps;     /* Matcher::Options::max_epi_search_steps (1000) */
  int32_t edgelet_filtering;        /* Matcher::Options::epi_search_edgelet_filtering (1) */
  double edgelet_max_angle;         /* Matcher::Options::epi_search_edgelet_max_angle (0.7) */
  double px_noise;                  /* 1.0 (:279-280) */
  double convergence_sigma2_thresh; /* DepthFilter::Options::seed_convergence_sigma2_thresh (200.0) */
  int32_t n_frames;
  int32_t n_pt;
  int32_t n_seg;
  int32_t reserved0;
  const double* frame_T;            /* 7*n_frames */
  const int32_t* frame_slot;        /* n_frames */
  /* point seeds */
  const int32_t* pt_ref_frame;      /* n_pt: it->ftr->frame */
  const int32_t* pt_cur_frame;      /* n_pt: the frame the seed is updated with */
  const double* pt_px;              /* 2*n_pt */
  const double* pt_f;               /* 3*n_pt */
  const int32_t* pt_level;          /* n_pt */
  const uint8_t* pt_type;           /* n_pt PLSVO_FTR_* */
  const double* pt_grad;            /* 2*n_pt (edgelets; may be NULL without edgelets) */
  const float* pt_a; const float* pt_b; const float* pt_mu; const float* pt_z_range; const float* pt_sigma2;
  /* line seeds */
  const int32_t* seg_ref_frame;
  const int32_t* seg_cur_frame;
  const double* seg_px;             /* 2*n_seg Feature::px */
  const double* seg_f;              /* 3*n_seg Feature::f  */
  const double* seg_sf;             /* 3*n_seg */
  const double* seg_ef;             /* 3*n_seg */
  const int32_t* seg_level;
  const float* seg_a; const float* seg_b; const float* seg_mu_s; const float* seg_mu_e;
  const float* seg_z_range_s; const float* seg_z_range_e; const float* seg_sigma2_s; const float* seg_sigma2_e;
} plsvo_seeds_in;

typedef struct plsvo_seeds_out {     /* caller buffers; any of them may be NULL */
  int32_t* pt_status;               /* n_pt PLSVO_SEED_* */
  float* pt_a; float* pt_b; float* pt_mu; float* pt_sigma2;
  double* pt_xyz_world;             /* 3*n_pt, valid for PLSVO_SEED_CONVERGED */
  double* pt_px_cur;                /* 2*n_pt Matcher::px_cur_ after a successful match (for setGridOccpuancy, :327-331) */
  double* pt_depth;                 /* n_pt   the triangulated depth z of a successful match */
  int32_t* seg_status;
  float* seg_a; float* seg_b; float* seg_mu_s; float* seg_mu_e; float* seg_sigma2_s; float* seg_sigma2_e;
  double* seg_xyz_world_s; double* seg_xyz_world_e;   /* 3*n_seg each */
  double* seg_depth_s; double* seg_depth_e;           /* n_seg each */
} plsvo_seeds_out;

int plsvo_update_seeds(plsvo_ctx* ctx, const plsvo_seeds_in* in, plsvo_seeds_out* out);

/* ------------------------------------------------------------------------------------------ */
/* depth-filter seed lists resident on the device: the list half of           */
/* DepthFilter -- initializeSeeds (src/depth_filter.cpp:177-191), removeKeyframe (:199-216),   */
/* and in updatePointSeeds / updateLineSeeds (:270-365, :367-471) the age test (:289-292), the */
/* erasing of converged and NaN seeds and the converged-seed callbacks (:334-360, :439-467).   */
/* The per-seed body is plsvo_update_seeds', bit for bit; a converged seed becomes a candidate */
/* landmark of the resident map tables exactly as plsvo_candidates_add writes one, without     */
/* leaving the device.  The seed tables belong to the staged candidate tables of the same ctx: */
/* ref_kf indexes the stream's resident keyframe table as it stands.                           */
/* Departures from the reference, on purpose: Seed::batch_counter (one static for both kinds   */
/* and every filter, :44) is one counter PER STREAM; removeKeyframe erases only the POINT      */
/* seeds of the keyframe and leaves line seeds pointing at a frame that may be gone -- here    */
/* the line seeds of a removed keyframe are erased too.                                        */
/* ------------------------------------------------------------------------------------------ */

#define PLSVO_SEED_AGED        5    /* batch_counter - batch_id > max_n_kfs: erased without an update (:289-292); resident lists only */
#define PLSVO_SEEDS_NO_ROOM    1    /* plsvo_seed_report.no_room */

/* Rows per stream and kind beyond the staged list lengths, for the NEXT and every later plsvo_seeds_stage. */
typedef struct plsvo_seed_reserve {
  int32_t extra_pt, extra_seg;
} plsvo_seed_reserve;

/* plsvo_seeds_in's parameters, and DepthFilter::Options::max_n_kfs */
typedef struct plsvo_seed_params {
  plsvo_pinhole cam;
  int32_t n_pyr_levels, align_max_iter, max_epi_search_steps, edgelet_filtering;
  double edgelet_max_angle, px_noise, convergence_sigma2_thresh;
  int32_t max_n_kfs, reserved0;
} plsvo_seed_params;

/* One stream's lists, in list order (input of the stage; caller buffers of plsvo_seeds_fetch_lists, each with room for the stream's
 * capacity rows, any of them NULL).  The float fields are plsvo_seeds_in's; spx / epx are LineFeat's end points in pixels, which ride
 * along for the landmark's observation only. */
typedef struct plsvo_seed_list {
  int32_t n_pt, n_seg, batch_counter, reserved0;
  int32_t* pt_ref_kf; int32_t* pt_batch_id;
  double* pt_px; double* pt_f; int32_t* pt_level; uint8_t* pt_type;
  double* pt_grad;                  /* 2 per seed; may be NULL at the stage without edgelets (zeros are stored) */
  float* pt_a; float* pt_b; float* pt_mu; float* pt_z_range; float* pt_sigma2;
  int32_t* seg_ref_kf; int32_t* seg_batch_id;
  double* seg_px; double* seg_f; double* seg_sf; double* seg_ef; double* seg_spx; double* seg_epx; int32_t* seg_level;
  float* seg_a; float* seg_b; float* seg_mu_s; float* seg_mu_e; float* seg_z_range_s; float* seg_z_range_e; float* seg_sigma2_s; float* seg_sigma2_e;
} plsvo_seed_list;

/* One stream's frame of an update.  pose_source: PLSVO_INSERT_POSE_* (RESIDENT: the optimised pose of plsvo_candidates_pose_optimize). */
typedef struct plsvo_seed_frame {
  int32_t active, cur_slot, pose_source, reserved0;
  double T_f_w[7];
  const double* d_T_f_w;
} plsvo_seed_frame;

/* What the last update did to one stream and its sizes as they stand.  pt / seg: rows per PLSVO_SEED_* status. */
typedef struct plsvo_seed_report {
  int32_t pt[6], seg[6];
  int32_t first_pt, first_seg;      /* index of the first new landmark per kind, -1 for none */
  int32_t n_pt_seeds, n_seg_seeds;  /* list lengths */
  int32_t n_pt, n_seg, n_pt_cand, n_seg_cand, n_pt_obs, n_seg_obs;   /* the map tables */
  int32_t no_room;                  /* PLSVO_SEEDS_NO_ROOM: the update of this stream was dropped as a whole */
  int32_t batch_counter;
} plsvo_seed_report;

/* One stream's keyframe event, applied in this order: removeKeyframe(removed_kf), ++batch_counter if new_batch, the new seeds
 * appended with ref_kf = new_kf (an index of the keyframe table as it stands NOW, after the insertion that closed it up). */
typedef struct plsvo_seed_kf {
  int32_t removed_kf;               /* -1: none */
  int32_t new_batch, new_kf, n_pt, n_seg, reserved0;
  double depth_mean, depth_min;     /* initializeSeeds' arguments, used as floats like the Seed constructor's (:53-74) */
  const double* pt_px; const double* pt_f; const int32_t* pt_level; const uint8_t* pt_type; const double* pt_grad;
  const double* seg_px; const double* seg_f; const double* seg_sf; const double* seg_ef; const double* seg_spx; const double* seg_epx; const int32_t* seg_level;
} plsvo_seed_kf;

/* The shadow rows of one stream: what the update launch leaves per seed, in the list order before that update.  Input of the
 * diagnostic plsvo_seeds_commit_rows (status, parameters and xyz_world; n_pt / n_seg must be the list lengths), caller buffers of
 * plsvo_seeds_fetch_rows (any of them NULL; n_pt / n_seg are written). */
typedef struct plsvo_seed_rows {
  int32_t n_pt, n_seg, active, reserved0;
  int32_t* pt_status; float* pt_a; float* pt_b; float* pt_mu; float* pt_sigma2; double* pt_xyz_world; double* pt_px_cur; double* pt_depth;
  int32_t* seg_status; float* seg_a; float* seg_b; float* seg_mu_s; float* seg_mu_e; float* seg_sigma2_s; float* seg_sigma2_e;
  double* seg_xyz_world_s; double* seg_xyz_world_e; double* seg_depth_s; double* seg_depth_e;
} plsvo_seed_rows;

/* Every check of every call runs on the host before anything is written; every call needs n == the staged n.
 * reserve: host only; PLSVO_E_INVALID for a negative field.  capacity: the rows per kind a stream's lists may hold (fields of
 *   plsvo_seed_reserve): the staged length plus the reserve in force at the stage.
 * stage: the lists with their batch ids and the stream's batch counter.  PLSVO_E_STATE without staged candidate tables of the same n
 *   or without pyramids; PLSVO_E_INVALID for a negative count, a NULL array with a non-zero count (pt_grad excepted), a ref_kf outside
 *   the stream's keyframe table, a level outside the pyramid, an unknown feature type, an edgelet without pt_grad under edgelet
 *   filtering, parameters plsvo_update_seeds refuses.  A later plsvo_candidates_stage drops the seed tables (the caller restages both):
 *   every seed call returns PLSVO_E_STATE until plsvo_seeds_stage is called again.
 * update: enqueue only -- the update launch (one lane per row, plsvo_update_seeds' body; the reference keyframe's pose and slot come
 *   from the resident keyframe table), then the commit launch (one wave per stream): aged, converged and NaN rows are erased, the
 *   list closes up in order, every converged row is appended to the map tables as plsvo_candidates_add would append it, in list
 *   order.  A stream whose map tables lack room for ALL its converged rows (landmark rows, observation entries, candidate lists) is
 *   reported PLSVO_SEEDS_NO_ROOM and neither its seed tables nor its map tables change; the other streams are not affected.  The
 *   caller restages with room and repeats the update.  It ends the open run as plsvo_candidates_add does and is legal behind an
 *   insertion.  PLSVO_E_INVALID for an unknown pose source, PLSVO_INSERT_POSE_DEV without a pointer, a negative slot or one outside
 *   the pyramids; PLSVO_E_STATE for PLSVO_INSERT_POSE_RESIDENT without a resident pose optimisation, and behind an unfetched update.
 * update_fetch: synchronises, returns the reports and refreshes the host's mirrors of the candidate tables (landmark counts, used
 *   observation entries, candidate counts), which plsvo_candidates_add, the insertion and the sizes of fetch_map / fetch_quality /
 *   set_quality depend on.  Between an update and this fetch every plsvo_candidates_* call that reads or moves the tables, and
 *   plsvo_seeds_keyframe / _fetch_lists / _fetch_rows / _commit_rows, return PLSVO_E_STATE; the fetches of the closed run keep working.
 * keyframe: enqueue only after the copy of the new seeds.  PLSVO_E_CAPACITY (nothing written) when a list would outgrow its rows,
 *   decided from the mirrored list lengths, which are exact after an update fetch and upper bounds after a keyframe event with a
 *   removal; PLSVO_E_INVALID for removed_kf outside [-1, n_kf] (the table as it stood before the insertion closed it up held at most
 *   one keyframe more), new_kf outside the table with new seeds, a level outside the pyramid, an unknown type, a non-positive depth,
 *   a NULL array with a non-zero count (pt_grad excepted without edgelets).
 * fetch_lists / fetch_rows: synchronise.  fetch_rows returns the last fetched update's rows (for setGridOccpuancy, :327-331,
 *   :432-436, and for tests); PLSVO_E_STATE before one.
 * commit_rows: a DIAGNOSTIC, synchronous, modelled on plsvo_candidates_set_match: uploads caller-made shadow rows in place of the
 *   update launch and runs the commit launch; plsvo_seeds_update_fetch follows it as it follows an update.  The row counts are checked
 *   against the mirrored list lengths: behind a keyframe event with a removal, plsvo_seeds_fetch_lists makes them exact first. */
int plsvo_seeds_reserve(plsvo_ctx* ctx, const plsvo_seed_reserve* reserve);
int plsvo_seeds_capacity(plsvo_ctx* ctx, int n, plsvo_seed_reserve* out);
int plsvo_seeds_stage(plsvo_ctx* ctx, int n, const plsvo_seed_params* params, const plsvo_seed_list* lists);
int plsvo_seeds_update(plsvo_ctx* ctx, int n, const plsvo_seed_frame* frames);
int plsvo_seeds_update_fetch(plsvo_ctx* ctx, int n, plsvo_seed_report* out);
int plsvo_seeds_keyframe(plsvo_ctx* ctx, int n, const plsvo_seed_kf* in);
int plsvo_seeds_fetch_lists(plsvo_ctx* ctx, int n, plsvo_seed_list* out);
int plsvo_seeds_fetch_rows(plsvo_ctx* ctx, int n, plsvo_seed_rows* out);
int plsvo_seeds_commit_rows(plsvo_ctx* ctx, int n, const plsvo_seed_rows* rows);

/* ------------------------------------------------------------------------------------------ */
/* a keyframe's point seeds started on the device from its FAST corners: the  */
/* creating half of DepthFilter::initializeSeeds (src/depth_filter.cpp:151-191) --             */
/* FastDetector::setExistingFeatures(frame->pt_fts_) (:161), the grid cells setGridOccpuancy   */
/* marked during the last update (:327-331), FastDetector::detect (:162-165,                   */
/* src/feature_detection.cpp:53-104), a PointSeed per new PointFeat (:184-186) -- without the  */
/* corners, the occupancy grid or the seeds crossing the bus.  Line seeds still travel as in   */
/* plsvo_seeds_keyframe (there is no device line detector).  Not covered: Frame::key_pts_, the */
/* C++ adapter; Seed::batch_counter stays per stream (see above).                              */
/* ------------------------------------------------------------------------------------------ */

#define PLSVO_SEED_OCC_SELECTED 1   /* FastDetector::setExistingFeatures(frame->pt_fts_), src/depth_filter.cpp:161: the point features the last
                                       plsvo_candidates_select wrote for the stream's new frame -- all n_matches of them, those the pose
                                       optimiser culled included (the reference leaves a culled feature in pt_fts_) */
#define PLSVO_SEED_OCC_UPDATED  2   /* setGridOccpuancy(matcher_.px_cur_) of the last fetched update, src/depth_filter.cpp:327-331: px_cur of every
                                       shadow row with status UPDATED, CONVERGED or NAN (the cell is marked before the convergence and
                                       NaN tests); rows NOT_VISIBLE, NO_MATCH and AGED mark nothing */

/* One stream's event, applied in this order: removeKeyframe(removed_kf) and ++batch_counter if new_batch, exactly as plsvo_seeds_keyframe;
 * the detector's grid for the configured level-0 size and params->cell_size (a cell is marked by the caller's byte or by a position of a
 * chosen source lying in it, cell = plsvo_detect_cell's; a position that is negative, not finite, or at or beyond the image size marks
 * nothing); FastDetector::detect on the pyramid slot of keyframe new_kf (the stream's resident slot) with that grid; one point seed per
 * valid cell in cell-index order behind the live rows -- ref_kf = new_kf, batch_id = the counter, px = (x_L << level, y_L << level),
 * type PLSVO_FTR_CORNER, grad (1, 0) (PointFeat's constructor), f = cam2world(px), a = b = 10 and mu, z_range, sigma2 as
 * plsvo_seeds_keyframe computes them; then the n_seg uploaded line seeds. */
typedef struct plsvo_seed_kf_detect {
  int32_t active;                   /* 0: the stream is not touched at all and costs no launch work */
  int32_t removed_kf;               /* -1: none */
  int32_t new_batch, new_kf;
  int32_t occ_sources;              /* PLSVO_SEED_OCC_* bits */
  int32_t n_seg;
  double depth_mean, depth_min;     /* as plsvo_seed_kf's */
  const uint8_t* d_occupancy;       /* DEVICE, cells bytes (cols * rows of plsvo_detect_grid), non-zero = occupied, OR-ed in; may be NULL */
  const double* seg_px; const double* seg_f; const double* seg_sf; const double* seg_ef; const double* seg_spx; const double* seg_epx; const int32_t* seg_level;
} plsvo_seed_kf_detect;

/* What the last event of a stream did; all zero for a stream no event has touched since the stage. */
typedef struct plsvo_seed_kf_report {
  int32_t n_new_pt, n_new_seg;      /* seeds appended (0 with no_room) */
  int32_t n_pt_seeds, n_seg_seeds;  /* list lengths behind the event */
  int32_t batch_counter;
  int32_t no_room;                  /* PLSVO_SEEDS_NO_ROOM: nothing of either kind was appended */
  int32_t n_occupied;               /* cells of the detector's grid that were marked */
  int32_t reserved0;
} plsvo_seed_kf_report;

/* keyframe_detect: ENQUEUE ONLY after the copy of the line seeds; the host waits for nothing.  Three launches whose sizes follow the
 *   ACTIVE streams: the occupancy grids, the detection (the detect_fast kernel through a slot table: the streams' keyframes sit in any
 *   slots and two streams may share one), the seed start.  The number of new point seeds is known to the device alone, so the point
 *   rows' room is decided there: when the live point rows (behind the removal) plus the new seeds exceed the rows the stream was laid
 *   out with (plsvo_seeds_capacity), NOTHING of either kind is appended and the report says PLSVO_SEEDS_NO_ROOM; the removal and the
 *   counter are applied either way.  The caller restages with room and repeats the event with removed_kf = -1, new_batch = 0: the
 *   result is then the reference's.  A caller that reserves `cells` point rows beyond its lists (plsvo_seeds_reserve) can never see
 *   no_room.  The segments' room is decided on the host from the mirrored lengths: PLSVO_E_CAPACITY, nothing written.  The detector's
 *   keys are left armed in every case: any detection may follow.
 *   Behind the call the host's mirrored list lengths are upper bounds until plsvo_seeds_keyframe_fetch, plsvo_seeds_fetch_lists or the
 *   next plsvo_seeds_update_fetch makes them exact: the point list's is old length + cells, capped at the stream's rows; the line
 *   list's is old length + n_seg, which a stream reported PLSVO_SEEDS_NO_ROOM did not append.
 *   PLSVO_E_STATE: no staged seed tables, an unfetched update, the pyramids not those of the stage, PLSVO_SEED_OCC_SELECTED without a
 *   selection on the context, PLSVO_SEED_OCC_UPDATED without a fetched update.  PLSVO_E_INVALID: whatever plsvo_hip_detect_fast_dev
 *   refuses in its params, n other than the staged n, and for an active stream new_kf outside the keyframe table, a keyframe slot
 *   outside the pyramids, unknown source bits, a non-positive depth, removed_kf outside [-1, n_kf], a negative n_seg, a NULL segment
 *   array with n_seg > 0, a segment level outside the pyramid.  Every check runs before anything is written or enqueued.
 * keyframe_fetch: synchronises, returns every stream's report and makes the mirrored list lengths exact, as plsvo_seeds_fetch_lists
 *   does.  A pipeline that goes straight on to the next frame's plsvo_seeds_update / _update_fetch needs neither; behind that update
 *   fetch this call costs a copy and no wait.  PLSVO_E_STATE before the first event since the stage and behind an unfetched update. */
int plsvo_seeds_keyframe_detect(plsvo_ctx* ctx, int n, const plsvo_detect_params* params, const plsvo_seed_kf_detect* in);
int plsvo_seeds_keyframe_fetch(plsvo_ctx* ctx, int n, plsvo_seed_kf_report* out);

/* ------------------------------------------------------------------------------------------ */
/* bootstrap: pyramidal KLT track of the first keyframe's corners.  Replaces  */
/* KltHomographyInit::addFirstFrame (src/initialization.cpp:40-54), ::addSecondFrame up to the */
/* disparity gate (:56-69), the list building of detectFeatures (:147-167) and trackKlt        */
/* (:170-215) with [ext] cv::calcOpticalFlowPyrLK, cv::buildOpticalFlowPyramid / pyrDown /     */
/* Scharr restated from upstream (tests/np_klt.py).  Stops in front of computeHomography       */
/* (:71-116).  Not covered: line detection, the error output's values, the C++ adapter.        */
/* ------------------------------------------------------------------------------------------ */
#define PLSVO_KLT_FAILURE     0   /* first frame: fewer than PLSVO_KLT_MIN_FIRST points (:44), nothing kept; second frame: n_tracked < init_min_tracked (:62) */
#define PLSVO_KLT_NO_KEYFRAME 1   /* median disparity < init_min_disparity (:68) */
#define PLSVO_KLT_TRACKED     2   /* both gates passed: the lists are ready for computeHomography */
#define PLSVO_KLT_INACTIVE    3   /* no first frame holds for the stream (never given, failed or dropped): nothing was done */
#define PLSVO_KLT_DROPPED     4   /* first frame: more points than cap_pts, nothing kept */
#define PLSVO_KLT_FIRST       5   /* addFirstFrame's SUCCESS: px_ref = px_cur = the points, nothing tracked yet */
#define PLSVO_KLT_MIN_FIRST   100
#define PLSVO_KLT_MAX_LEVEL   4   /* trackKlt's maxLevel (:190): at most five levels */
/* exit taken by calcOpticalFlowPyrLK at one level of one point (plsvo_klt_track_points) */
#define PLSVO_KLT_EXIT_NONE      0   /* the level does not exist (above the top level) */
#define PLSVO_KLT_EXIT_PREV_OOR  1   /* the window of prev lies outside the level */
#define PLSVO_KLT_EXIT_FLAT      2   /* minEig < min_eig or D < FLT_EPSILON */
#define PLSVO_KLT_EXIT_ITER_OOR  3   /* the window of next left the level in the iteration `iters` (0-based) */
#define PLSVO_KLT_EXIT_EPS       4   /* |delta|^2 <= eps^2 after `iters` iterations */
#define PLSVO_KLT_EXIT_OSC       5   /* delta + previous delta below 0.01 in both coordinates: half a step back */
#define PLSVO_KLT_EXIT_MAX_ITER  6   /* max_iter iterations */

typedef struct plsvo_klt_cfg {
  int32_t streams, cap_pts;          /* resident streams; points a stream's lists may hold */
  int32_t win;                       /* 30 (klt_win_size, :179); anything else is refused */
  int32_t max_level;                 /* 4 (:190), 0 .. PLSVO_KLT_MAX_LEVEL */
  int32_t max_iter;                  /* 30 (:180), 1 .. 255 */
  int32_t reserved0;
  double  eps;                       /* 0.001 (:181): the iteration stops at |delta|^2 <= eps * eps */
  double  min_eig;                   /* 1e-4, calcOpticalFlowPyrLK's default minEigThreshold */
} plsvo_klt_cfg;

/* One stream's first frame.  The list is the corners -- px = ((float)x, (float)y), f = cam2world(px) -- followed by the extra points
 * with the bearings given: the endpoint / midpoint / endpoint triples of :159-167 for segments the host detected (the midpoint's
 * bearing is (sf + ef) / 2, no cam2world result). */
typedef struct plsvo_klt_first {
  int32_t active;                    /* 0: the stream is not touched at all */
  int32_t slot;                      /* the pyramid slot of the reference frame; the caller leaves its level 0 as it is until the bootstrap ends */
  plsvo_pinhole cam;
  const plsvo_corner* d_corners;     /* DEVICE, the stream's records as plsvo_hip_detect_fast_dev left them (cell order), or NULL */
  const int32_t* d_count;            /* DEVICE, their count (required with d_corners) */
  int32_t n_host, n_extra;
  const float* host_px;              /* n_host x 2, read when d_corners is NULL */
  const float* extra_px;             /* n_extra x 2 */
  const double* extra_f;             /* n_extra x 3 */
} plsvo_klt_first;

typedef struct plsvo_klt_second { int32_t active, cur_slot; } plsvo_klt_second;
typedef struct plsvo_klt_params {
  int32_t init_min_tracked;          /* Config::initMinTracked(), 40 */
  int32_t reserved0;
  double  init_min_disparity;        /* Config::initMinDisparity(), 40.0 */
} plsvo_klt_params;

/* What the last call that touched a stream did; PLSVO_KLT_INACTIVE and zeros after plsvo_klt_reserve. */
typedef struct plsvo_klt_report {
  int32_t result;                    /* PLSVO_KLT_* */
  int32_t n_before, n_after;         /* list length in front of and behind the call (first frame: points offered, points kept) */
  int32_t levels;                    /* pyramid levels the tracker used (top level + 1) */
  double  median_disparity;          /* vk::getMedian(disparities_): the element of rank n_after / 2; 0 with an empty list and on a first frame */
  int32_t n_calls;                   /* second-frame calls since the first frame */
  int32_t reserved0;
} plsvo_klt_report;

/* A stream's lists in host memory (plsvo_klt_fetch_tracks; every pointer may be NULL) or on the device (plsvo_klt_tracks_dev: the
 * arrays of ALL streams, stream s from element s * cap_pts, valid for the first count[s] entries once the launches in flight have run). */
typedef struct plsvo_klt_tracks {
  int32_t n, cap_pts;
  float* px_ref; float* px_cur;      /* x 2 */
  double* f_ref; double* f_cur;      /* x 3; f_cur and disparity are valid behind a second frame */
  double* disparity;
  int32_t* count;                    /* tracks_dev only: per stream */
} plsvo_klt_tracks;

/* reserve: lays out the lists and the KLT pyramid store (levels 1 .. L of two frames per stream, OpenCV's pyrDown of level 0 -- not the
 *   slots' half-sampled levels) for the configured pyramids' level-0 size; every stream starts PLSVO_KLT_INACTIVE.  PLSVO_E_STATE
 *   without configured pyramids; PLSVO_E_INVALID for NULL cfg, streams or cap_pts below 1, win other than 30, max_level outside
 *   0 .. PLSVO_KLT_MAX_LEVEL, max_iter outside 1 .. 255, eps or min_eig negative or not finite.
 * first_frame: ENQUEUE ONLY after the copy of the host lists: the lists of the active streams and the KLT pyramid of their slots.
 *   Fewer than PLSVO_KLT_MIN_FIRST points: PLSVO_KLT_FAILURE; more than cap_pts: PLSVO_KLT_DROPPED; nothing is kept in both cases.
 * second_frame: ENQUEUE ONLY, for any subset of the batch: the KLT pyramid of cur_slot, the track of every list entry from its px_cur
 *   (OPTFLOW_USE_INITIAL_FLOW), then per stream the stable compaction of px_ref / px_cur / f_ref over status == 0, f_cur, the
 *   disparities, their median and the gates.  The lists are left compacted whatever the result, so the next call starts from the kept px_cur.
 * Both: PLSVO_E_STATE without a reserve or when the pyramids were reconfigured since; PLSVO_E_INVALID (nothing written or enqueued)
 *   for another n than reserved, NULL in / params with n > 0 and, for an active stream, a slot outside the pyramids, a camera that is
 *   not the pyramids' level-0 size or has a non-finite or zero focal length, d_corners without d_count, a negative count, a NULL
 *   array with a non-zero count, a negative init_min_tracked or a non-finite init_min_disparity.
 * fetch: synchronises; every stream's report.  PLSVO_E_STATE without a reserve, PLSVO_E_INVALID for another n or NULL out.
 * fetch_tracks: synchronises; out->n and the arrays that are not NULL (room for cap_pts entries).  PLSVO_E_INVALID for a stream
 *   outside the batch or NULL out.  tracks_dev: no synchronisation.
 * The pyramid launches are timed under PLSVO_K_HALFSAMPLE, the track under PLSVO_K_MATCH, the list launches under PLSVO_K_NEWCAND. */
int plsvo_klt_reserve(plsvo_ctx* ctx, const plsvo_klt_cfg* cfg);
int plsvo_klt_first_frame(plsvo_ctx* ctx, int n, const plsvo_klt_first* in);
int plsvo_klt_second_frame(plsvo_ctx* ctx, int n, const plsvo_klt_second* in, const plsvo_klt_params* params);
int plsvo_klt_fetch(plsvo_ctx* ctx, int n, plsvo_klt_report* report);
int plsvo_klt_fetch_tracks(plsvo_ctx* ctx, int stream, plsvo_klt_tracks* out);
int plsvo_klt_tracks_dev(plsvo_ctx* ctx, plsvo_klt_tracks* out);
/* Host only, no ctx: the top level L of calcOpticalFlowPyrLK's pyramid for a level-0 size (the first level whose next size has
 * w <= win or h <= win, at most max_level) and the sizes of levels 0 .. L (w, h: room for PLSVO_KLT_MAX_LEVEL + 1, may be NULL).
 * Returns L, or PLSVO_E_INVALID for a size or win below 1 or max_level outside 0 .. PLSVO_KLT_MAX_LEVEL. */
int plsvo_klt_levels(int width, int height, int win, int max_level, int32_t* w, int32_t* h);
/* Diagnostics (tests; like plsvo_hip_detect_stages for the detector).  download_level: level 1 .. L of a stream's KLT pyramid,
 * which = 0 the reference frame's, 1 the last current frame's; synchronises; PLSVO_E_INVALID for a level the store does not hold.
 * track_points: STATELESS -- builds the KLT pyramids of two slots in a scratch store and runs the production track kernel on n
 * arbitrary prev / next points (x 2 floats each) under cfg (streams and cap_pts are not read); next_out: n x 2, status: n bytes,
 * exit_code / iters: n x (PLSVO_KLT_MAX_LEVEL + 1) bytes indexed by level.  Needs no reserve and leaves the resident lists alone. */
int plsvo_klt_download_level(plsvo_ctx* ctx, int stream, int which, int level, uint8_t* out);
int plsvo_klt_track_points(plsvo_ctx* ctx, const plsvo_klt_cfg* cfg, int ref_slot, int cur_slot, int n, const float* prev, const float* next_in,
                           float* next_out, uint8_t* status, uint8_t* exit_code, uint8_t* iters);

/* ------------------------------------------------------------------------------------------ */
/* multi-GPU: gather of per-stream pose records (new; the reference is single-process)         */
/* ------------------------------------------------------------------------------------------ */

/* The per-stream record a rank publishes after a frame step: what FrameHandlerMono::processFrame decides on
 * afterwards -- the pose it keeps (src/frame_handler_mono.cpp:92, :327-329), SparseImgAlign::run's return value (:272-274), the pose
 * optimiser's surviving observations (sfba_n_edges_final = num_obs_pt + num_obs_ls, :327-335) -- so that the rank that holds the
 * gathered table sees which streams lost tracking without a second exchange.  Fixed size: 96 bytes. */
#define PLSVO_REC_ALIGN      0x01   /* an alignment batch contributed (n_tracked, PLSVO_REC_ALIGN_STOP, PLSVO_REC_ALIGN_ERROR valid) */
#define PLSVO_REC_ALIGN_STOP 0x02   /* the alignment's solver raised stop_ (NaN in solve, src/sparse_img_align.cpp:700) */
#define PLSVO_REC_ALIGN_ERROR 0x04  /* device-side capacity / consistency error (plsvo_align_out.status bit 1) */
#define PLSVO_REC_POSEOPT    0x08   /* a pose-optimisation batch contributed (T_f_w is its result; num_obs_*, error_final valid) */
#define PLSVO_REC_POSEOPT_EMPTY 0x10 /* optimizeGaussNewton returned early: no observation (src/pose_optimizer.cpp:88-89) */
typedef struct plsvo_pose_record {
  double T_f_w[7];                  /* qx qy qz qw tx ty tz: pose_optimizer's T_f_w when PLSVO_REC_POSEOPT, else the alignment's T_cur_from_ref */
  uint64_t n_tracked;               /* SparseImgAlign::run's return value, n_meas_ / patch_area_ (src/sparse_img_align.cpp:94) */
  uint64_t num_obs_pt;              /* optimizeGaussNewton's num_obs_pt (src/pose_optimizer.cpp:218-226) */
  uint64_t num_obs_ls;              /* ... num_obs_ls (:239-245) */
  double error_final;               /* ... error_final (:247-251) */
  int32_t status;                   /* PLSVO_REC_* */
  int32_t stream;                   /* index of the stream in the publishing context's batch */
} plsvo_pose_record;

/* Writes one record per stream of the resident batch into device memory (d_dst: n records), enqueued on the ctx stream after the
 * launches that produce them: the resident frame step (plsvo_chain_stage) if one is staged and no staged pose-optimisation batch has
 * run since it was staged and last ran, else the staged alignment and
 * pose-optimisation batches that have run -- both when they have the same number of jobs (one job of each per stream), otherwise the
 * one that ran last.  *n_out (may be NULL) receives the record count. */
int plsvo_pack_pose_records(plsvo_ctx* ctx, plsvo_pose_record* d_dst, int* n_out);
/* The same records in host memory (out: n records, n = the resident batch's size): packs into a ctx-owned device buffer, copies,
 * synchronises the ctx stream.  For a single-process host that wants the table without a communicator. */
int plsvo_fetch_pose_records(plsvo_ctx* ctx, int n, plsvo_pose_record* out);

/* All-gather of n_local pose records (device memory) over an RCCL communicator (ncclComm_t passed as void*), enqueued on the ctx
 * stream: d_all receives world_size*n_local records, rank-major (96 B per stream: 768 B per rank for BASELINE configs[3]).  No other
 * collective exists on this path (streams are independent). */
int plsvo_gather_poses(plsvo_ctx* ctx, void* rccl_comm, const plsvo_pose_record* d_local, int n_local,
                       plsvo_pose_record* d_all);

/* ------------------------------------------------------------------------------------------ */
/* timing (hipEvent pairs recorded on the ctx stream around each kernel family)                */
/* ------------------------------------------------------------------------------------------ */
#define PLSVO_K_ALIGN_INIT    0
#define PLSVO_K_ALIGN_LEVEL   1   /* the residual/Jacobian + GN kernel (dominant) */
#define PLSVO_K_POSEOPT       2
#define PLSVO_K_HALFSAMPLE    3
#define PLSVO_K_STRUCTOPT     4
#define PLSVO_K_MATCH         5
#define PLSVO_K_SEEDS         6   /* plsvo_update_seeds and the update launch of plsvo_seeds_update */
#define PLSVO_K_KEYFRAME      7   /* plsvo_close_keyframes / plsvo_keyframe_decide: the launch alone, without packing and copies */
#define PLSVO_K_CANDIDATES    8   /* plsvo_candidates_run: the re-arm and the launch alone (the resident match counts under PLSVO_K_MATCH) */
#define PLSVO_K_SELECT        9   /* plsvo_candidates_select: the re-arm and the launch alone */
#define PLSVO_K_INSERT        10  /* plsvo_candidates_insert_keyframe: the launch that changes the tables (the planning launch is timed by the caller's clock) */
#define PLSVO_K_NEWCAND       11  /* plsvo_candidates_add: the launch alone; the commit launch of plsvo_seeds_update, plsvo_seeds_keyframe's, the three of plsvo_seeds_keyframe_detect */
#define PLSVO_K_COUNT         12
int plsvo_hip_set_profiling(plsvo_ctx* ctx, int enable);
/* accumulated GPU time and launch count of kernel family k since the last reset (synchronises) */
int plsvo_hip_kernel_time(plsvo_ctx* ctx, int k, double* total_ms, int64_t* launches);
int plsvo_hip_reset_profiling(plsvo_ctx* ctx);

/* library / device info */
const char* plsvo_hip_version(void);
/* compile-time experiment switches of THIS build of the alignment kernel, space-separated ("" for the default build; "byte_cache",
 * "lds_img": pl-svo_amd/csrc/Makefile's A/B targets).  bench.py prices its roofline with the bytes the build really moves. */
const char* plsvo_hip_build_flags(void);
int plsvo_hip_device_info(plsvo_ctx* ctx, char* name, int name_len, int* cu_count, size_t* hbm_bytes);

#ifdef __cplusplus
}
#endif
#endif /* PLSVO_HIP_H_ */
