// plsvo_dev.hpp -- device-side data layout (HBM) shared by the kernels and the C-ABI host code.
//
// Layout principles (MI355X-first):
//   * every batch is a set of flat SoA arrays; a job is an (offset, count) pair into them -- no pointers
//     chased on the device, fully coalesced feature reads;
//   * pyramids live in one slab: slot s, level l at base + s*slot_bytes + off[l], rows tight
//     (stride == level width), each level 256-byte aligned, so staging a level into LDS is one
//     linear 16-byte-per-lane copy;
//   * per-level alignment cache (reference-patch intensity + image gradient, 3 floats per pixel, and the
//     per-patch 3-D point) is written once per level and re-read every Gauss-Newton iteration by the
//     same lanes in the same order (coalesced float4).
#pragma once
#include <stdint.h>

#include "../../include/plsvo_hip.h"

namespace plsvo_hip {

// byte offset of level `level` inside a pyramid slot: every level is followed by >= 64 bytes of slack and
// starts on a 256-byte boundary (one formula for host and device)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline unsigned int pyr_level_offset(int width, int height, int level) {
  unsigned long long off = 0;
  for (int l = 0; l < level; ++l) off += (((unsigned long long)(width >> l) * (unsigned long long)(height >> l) + 64) + 255) & ~255ull;
  return (unsigned int)off;
}

// TILED MIRROR of the pyramids, read by the alignment kernel (written by tile_level_kernel whenever a slot changes).  A level is
// cut into tiles of 16 x 8 pixels = 128 B = one L2 line, tiles row-major, pixel (x, y) at
//     ((y >> 3) * tiles_x + (x >> 4)) * 128 + (y & 7) * 16 + (x & 15),        tiles_x = ceil(w / 16)
// A 5x5 window of a row-major level touches five lines (one per image row: 640 B fetched for 25 B used); in tiles it touches
// (1 + 4/16)(1 + 4/8) = 1.9 lines on average.  The launch runs within a few per cent of the achievable HBM rate, so lines are time.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline unsigned int pyr_tiled_level_offset(int width, int height, int level) {
  unsigned long long off = 0;
  for (int l = 0; l < level; ++l) {
    const unsigned long long tiles = (unsigned long long)(((width >> l) + 15) >> 4) * (unsigned long long)(((height >> l) + 7) >> 3);
    off += (tiles * 128 + 255) & ~255ull;
  }
  return (unsigned int)off;
}
#if defined(__HIPCC__)
__device__ __forceinline__ int tiled_row_offset(int tiles_x, int y) { return (((y >> 3) * tiles_x) << 7) + ((y & 7) << 4); }
__device__ __forceinline__ int tiled_col_offset(int x) { return ((x >> 4) << 7) + (x & 15); }
#endif

// alignment launch shapes from this many threads per frame on are LATENCY shapes (a frame owns most of a CU): four lanes per slot in the
// pixel pass, the reference patches kept as FLOAT rows (192 B per slot, L2-resident) instead of the 64-byte record the throughput shapes rebuild
constexpr int kQuadMinThreads = 256;

struct PyrDesc {
  const uint8_t* base;
  unsigned long long slot_bytes;
  const uint8_t* tbase;               // tiled mirror: slot s at tbase + s * tslot_bytes, level l at + pyr_tiled_level_offset(w, h, l)
  unsigned long long tslot_bytes;
  int n_slots, n_levels;
  int w[PLSVO_MAX_LEVELS], h[PLSVO_MAX_LEVELS];
  unsigned int off[PLSVO_MAX_LEVELS];
};

struct AlignJobDev {
  int ref_slot, cur_slot;
  double fx, fy, cx, cy;
  int width, height;
  int max_level, min_level, n_iter, skip;   // skip: no features at all (src/sparse_img_align.cpp:58-62)
  double eps;
  int pt_off, n_pts, seg_off, n_seg;        // into the batch feature arrays
  int patch_off, patch_cap;                 // into the batch patch-cache arrays (slots)
  int n_slots[PLSVO_MAX_LEVELS];            // patch slots of the static layout, per level (host: align_slot_layout)
  int long_mask;                            // bit l: some segment has more than 64 samples at level l (two-pass level)
  int ldlt_flavour;                         // 320 / 330: zero-pivot rule of Eigen's LDLT (plsvo_wave.hpp::wave_solve6_core)
};

struct AlignStateDev {
  double T[7];                 // current model T_cur_from_ref
  double chi2;                 // solver chi2_
  unsigned long long n_meas;   // n_meas_ of the last computeResiduals
  double H[36];                // H_ of the last computeResiduals
  int stop;                    // solver stop_
  int log_count;
  int iters[PLSVO_MAX_LEVELS];
  unsigned long long patch_levels, patch_iters;  // work counters
  unsigned long long patch_iters_pt;             // of patch_iters, those of point features that wrote 64 B of chi2 terms to HBM
  int error;                   // device-side capacity/consistency error
  int chi2_ties;               // Gauss-Newton iterations whose accept / roll-back decision was taken on the exact float chi2 sums
  int chi2_unarmed;            // near ties met while the per-pixel terms of one of the two iterations had not been kept
  int reserved2;
  unsigned long long phase_ticks[8];  // only filled by -DPLSVO_TIMING builds (s_memtime ticks per phase)
};

struct AlignBatchDev {
  const AlignJobDev* jobs;
  AlignStateDev* state;
  const double* T0;            // 7 per job
  const double* pt_px;         // 2 per point
  const double* pt_xyz;        // 3 per point
  const double* seg_spx;       // 2 per segment
  const double* seg_epx;
  const double* seg_len;       // 1
  const double* seg_p;         // 3
  const double* seg_q;         // 3
  const uint8_t* seg_alive_in; // 1 (may be null)
  uint8_t* seg_alive;          // 1, working copy / result
  // static slot layout of the segments: seg_slot[(level - slot_level0) * slot_stride + segment] = first slot | N << 20, or -1
  const int* seg_slot;
  int slot_level0, slot_stride;
  // per-level patch cache (capacity = sum over jobs of patch_cap slots)
  double* patch_xyz;           // 3 per slot: 3-D point in the ref frame
  float* patch_uvref;          // 2 per slot: ref pixel position at the level (float, as Patch::setPosition)
  float* cache_ref;            // 64 bytes per slot: the reference patch's byte record (7 rows of 8 image bytes + the two sub-pixel fractions, align_refpatch.hpp);
                               // latency shapes (>= kQuadMinThreads threads per frame): 192 bytes per slot, four rows of {ref[4], dx[4], dy[4]} floats
  // per-pixel terms of the solver's chi2 for the POINT features, double-buffered by iteration parity (plane 0 / 1, chi_plane
  // floats apart): 16 per point of the batch, res*res*w (src/sparse_img_align.cpp:484).  Written by every iteration, read only when
  // two successive chi2 values are too close for the double-precision sums to order them the way the reference's sequential
  // float sums do (align_kernels.hip::exact_chi2_pair).
  float* chi_terms;
  unsigned long long chi_plane;
  int chi_lds_pts;             // > 0: the two planes live in LDS instead (capacity in points per plane): small batches, where a
  int reserved_lds;            //      workgroup has LDS to spare and nothing to hide a global store's acknowledge behind
  double* poses;               // 7 per job: final model, contiguous (what a device-side consumer / the RCCL gather reads)
  PyrDesc pyr;
  plsvo_align_iterlog* log;    // log_cap per job, or null
  int log_cap;
  int n_jobs;
  const int* order;            // launch order: workgroup w works on job order[w] (jobs with the most patches first), or null
  // TWO WORKGROUPS PER FRAME (latency shapes, at most cu_count / 2 frames): rank 0 owns the point slots, rank 1 the segment slots (the host
  // layout starts the segments at a multiple of 64); every iteration the two exchange their 32 partial sums through `xbuf` (64 tagged
  // 8-byte granules per rank and parity, plsvo_wave.hpp::pair_allgather32) and both run the solver on the identical totals.
  int* work_key;               // 1 per job, or null: the patch-iterations the job's last launch evaluated (what the next launch's order is sorted by)
  int pair;                    // 0 = one workgroup per frame, 1 = two
  unsigned int xseq0;          // first sequence number of this launch's exchanges (launch number << 10: never repeats in the buffer's life)
  unsigned long long* xbuf;    // 2 (parity) x 2 (rank) x 64 granules per frame
  // TAIL SPLIT (one wave per frame, batches of many rounds): the last tail_n entries of the launch order run as TWO workgroups of the
  // same launch -- the coarse levels first of all, the finest level last of all -- and hand the frame's state over through
  // AlignStateDev / seg_alive and one flag word each (align_kernels.hip::align_fused_kernel).  0 = every frame is one workgroup.
  int tail_n;
  int static_solve;            // wave-uniform: 1 = the 6x6 solve takes the static pivot order when the diagonals allow it (plsvo_wave.hpp::wave_solve6_core),
                               //               0 = always the per-step pivot search (PLSVO_OPT_ALIGN_STATIC_SOLVE); bit-identical results
  unsigned int* tail_flag;     // tail_n words, zeroed before every launch; 1 = the coarse part of tail frame t has published its state
  uint8_t* seg_alive_tail;     // a coarse part's working copy of the segment flags (layout of seg_alive): it never stores into seg_alive or the
                               // state with ordinary stores, so no dirty byte of its L2 can land on what the fine part writes later
};

struct PoseJobDev {
  double T0[7];
  double fx, reproj_thresh;
  int n_iter, n_iter_ref;
  int pt_off, n_pts, seg_off, n_seg;
  int ldlt_flavour, reserved0;
};

struct PoseStateDev {
  double T[7];
  double cov[36];
  double estimated_scale, error_init, error_final;
  unsigned long long num_obs_pt, num_obs_ls;
  int iters, iters_ref, status, log_count;
  unsigned long long pt_iters, seg_iters;   // work counters
  unsigned long long phase_ticks[8];        // only filled by -DPLSVO_TIMING builds (s_memtime ticks per phase)
};

struct PoseBatchDev {
  const PoseJobDev* jobs;
  PoseStateDev* state;
  const double* pt_f;          // 3 per point
  const double* pt_pos;        // 3
  const int* pt_level;
  const double* seg_line;      // 3 per segment
  const double* seg_spos;
  const double* seg_epos;
  const int* seg_level;
  uint8_t* pt_keep;
  uint8_t* seg_keep;
  float* scratch_f32;          // per feature, for the float medians (errors)
  double* scratch_f64;         // 5 per feature: chi2_vec_init (2x), chi2_vec_final, and two per point for its normalised observation
  plsvo_poseopt_iterlog* log;
  int log_cap;
  int n_jobs;
  const int* order;            // launch slot -> job, or null (identity): a RE-RUN of a staged batch takes its frames sorted by work_key, most first
  int* work_key;               // 1 per job, or null: the feature-iterations the job's last launch evaluated
};

struct StructBatchDev {
  const double* frame_T;
  const double* pt_pos; const int* pt_obs_off; const int* pt_obs_frame; const double* pt_obs_f;
  const double* seg_spos; const double* seg_epos; const int* seg_obs_off; const int* seg_obs_frame;
  const double* seg_obs_sf; const double* seg_obs_ef;
  double* pt_pos_out; double* seg_spos_out; double* seg_epos_out; int* pt_iters; int* seg_iters;
  int n_pts, n_seg, n_iter_pts, n_iter_segs;
};

// direct feature matching: flat candidate arrays (include/plsvo_hip.h plsvo_match_in), one lane per candidate
struct MatchBatchDev {
  const uint8_t* pyr_base; unsigned long long slot_bytes;
  int width, height;                // level-0 size of every pyramid slot
  double fx, fy, cx, cy; int cam_width, cam_height;
  int n, n_pyr_levels, align_max_iter;
  const double* frame_T; const int* frame_slot; const int* cur_frame; const int* ref_frame;
  const double* ref_px; const double* ref_f; const int* ref_level; const uint8_t* ref_type; const double* ref_grad;
  const double* pos; const double* px_cur;
  double* px_out; uint8_t* found; int* search_level; int* n_iter;
  const uint8_t* active;            // optional (resident frame step): candidates with 0 are reported "not found" without any work
  // plsvo_match_warp_patches only (match_direct_kernel<true>; the <false> instantiation never reads them): any may be null
  double* diag_A; uint8_t* diag_warped; uint8_t* diag_patch; uint8_t* diag_staged;
};

// depth-filter seeds (include/plsvo_hip.h plsvo_seeds_in / plsvo_seeds_out), one lane per seed
struct SeedsBatchDev {
  const uint8_t* pyr_base; unsigned long long slot_bytes;
  int width, height;
  double fx, fy, cx, cy; int cam_width, cam_height;
  int n_pyr_levels, align_max_iter, max_epi_search_steps, edgelet_filtering;
  double edgelet_max_angle, px_error_angle, convergence_sigma2_thresh;
  int n_pt, n_seg;
  const double* frame_T; const int* frame_slot;
  const int* pt_ref_frame; const int* pt_cur_frame; const double* pt_px; const double* pt_f; const int* pt_level; const uint8_t* pt_type;
  const double* pt_grad; const float* pt_a; const float* pt_b; const float* pt_mu; const float* pt_z_range; const float* pt_sigma2;
  const int* seg_ref_frame; const int* seg_cur_frame; const double* seg_px; const double* seg_f; const double* seg_sf; const double* seg_ef;
  const int* seg_level; const float* seg_a; const float* seg_b; const float* seg_mu_s; const float* seg_mu_e; const float* seg_z_range_s;
  const float* seg_z_range_e; const float* seg_sigma2_s; const float* seg_sigma2_e;
  // outputs
  int* o_pt_status; float* o_pt_a; float* o_pt_b; float* o_pt_mu; float* o_pt_sigma2; double* o_pt_xyz; double* o_pt_px; double* o_pt_depth;
  int* o_seg_status; float* o_seg_a; float* o_seg_b; float* o_seg_mu_s; float* o_seg_mu_e; float* o_seg_sigma2_s; float* o_seg_sigma2_e;
  double* o_seg_xyz_s; double* o_seg_xyz_e; double* o_seg_depth_s; double* o_seg_depth_e;
};

// resident frame step (chain_kernels.hip): one job = one stream's new frame
struct ChainJobDev {
  double T_prev[7], T_kf[7];        // previous frame's and keyframe's T_f_w
  int kf_slot, cur_slot;            // pyramid slots
  int cand_off, n_pt, n_seg;        // candidates of the job: [points | segment start points | segment end points] from cand_off
  int po_pt_off, po_seg_off;        // where its selected features go in the pose optimiser's input arrays
  int reserved0;
};
struct ChainBatchDev {
  const ChainJobDev* jobs; int n_jobs, n_cand;
  const double* align_poses;        // 7 per job: T_cur_from_ref of the alignment launch
  double* frame_T; int* frame_slot; // 2 per job: [keyframe, new frame]
  const int* cand_job; const double* pos; const uint8_t* active_in;
  const int* cell; uint8_t* active;                                  // reprojection result / worth matching
  const double* m_px; const uint8_t* found; const int* search_level; // matcher result
  double fx, fy, cx, cy;
  int n_cells, cell_rule, max_fts; const int* cell_order;
  // the segments' grid (gridls_): 0 cells = every matched segment becomes a feature
  const double* proj_px;            // 2 per candidate: the projection the reprojection kernel wrote (what files a segment in its cells)
  int seg_cell_size, seg_n_cols, seg_n_cells, max_fts_segs; const int* seg_cell_order;
  PoseJobDev* po_jobs; double* pt_f; double* pt_pos; int* pt_level; double* seg_line; double* seg_spos; double* seg_epos; int* seg_level;
  int* sel_pt; int* sel_seg; int* n_sel;
  double reproj_thresh; int po_n_iter, ldlt_flavour;
};

struct ReprojBatchDev {
  double fx, fy, cx, cy; int cam_width, cam_height;
  int n, cell_size, grid_n_cols, boundary;
  const double* frame_T; const int* frame; const double* pos;
  double* px; int* cell;
};

// keyframe stage (keyframe_device.hpp, include/plsvo_hip.h plsvo_close_keyframes / plsvo_keyframe_decide): one wave per stream; the
// streams' tables and feature lists are concatenated, a job holds its offsets (in entries, not bytes)
struct CloseKfJobDev {
  double T[7];
  double fx, fy, cx, cy;
  int width, height;
  int n_kf, max_n_kfs;
  long long kf_off;                 // first keyframe of the stream in kf_T / keypt_* / tmp_dist / close_*
};
struct CloseKfBatchDev {
  const CloseKfJobDev* jobs; int n_jobs;
  const double* kf_T; const double* keypt_pos; const uint8_t* keypt_valid;
  double* tmp_dist;                 // per keyframe: its distance, -1 = not close
  int* close_idx; double* close_dist;
  int* counts;                      // 2 per job: n_close, n_overlap
};
struct KfDecideJobDev {
  double T_new[7], T_last[7];
  const double* d_T_new;            // device pointer read instead of T_new, or null
  double min_t, min_r;
  int width, height;
  int n_pt, n_seg, n_kf, n_ov;
  long long pt_off, seg_off, kf_off, ov_off, depth_off;
  int key_prev[5]; int reserved0;
};
struct KfDecideOutDev {
  double depth_mean, depth_min;
  int has_depth, n_depth, need_new_kf, blocking;
  int key_pts[5]; int furthest_kf;
};
struct KfDecideBatchDev {
  const KfDecideJobDev* jobs; KfDecideOutDev* out; int n_jobs;
  const double* pt_px; const double* pt_pos; const uint8_t* pt_alive;
  const double* seg_spos; const double* seg_epos; const uint8_t* seg_alive;
  const double* kf_T; const int* overlap_idx;
  unsigned long long* depth_keys;   // n_pt + 2 * n_seg per job from depth_off: the order-preserving keys of the depths (all ones = dead)
  double* delta_t; double* delta_r; // per overlap entry
};

// map candidates (candidates_device.hpp, include/plsvo_hip.h plsvo_candidates_*): one wave per stream.  The streams' map tables are
// concatenated and stay resident; a stream's record holds its counts and offsets (in entries, not bytes).  CSR offset arrays keep the
// caller's stream-relative values: kf_pt_off of stream s has n_kf + 1 entries from kf_off + s, pt_obs_off n_pt + 1 from pt_off + s.
struct CandMapDev {
  int n_kf, n_pt, n_seg, n_pt_cand, n_seg_cand;
  int cap_pt, cap_seg;              // the stream's filed rows as laid out: landmark rows + candidate entries of CAPACITY (the counts without a landmark reserve)
  int stream;                       // s
  long long kf_off;                 // keyframes: kf_T, kf_pos
  long long kfpt_off, kfseg_off;    // the keyframes' feature lists
  long long pt_off, seg_off;        // landmarks
  long long ptobs_off, segobs_off;  // observations
  long long ptc_off, segc_off;      // the map's candidate lists (and their failure flags)
  long long opt_off, oseg_off;      // filed landmarks: scratch in filing order, results in output order (capacity rows)
  long long m_off;                  // the matcher's candidates: cap_pt + 2 * cap_seg entries
  long long f_off;                  // the matcher's frame table: n_kf keyframes, then the new frame
  long long vis_pt_off, vis_seg_off;// first-visit words, rows padded to 64 words
};
struct CandJobDev {                 // one stream's frame (plsvo_candidates_run)
  double T[7];
  const double* d_T;                // device pointer read instead of T, or null
  int cur_slot, n_ov;
  long long ov_off;                 // overlap list and the counts per overlap keyframe
};
struct CandBatchDev {
  const CandMapDev* maps; const CandJobDev* jobs; int n_jobs;
  double fx, fy, cx, cy; int cam_width, cam_height;
  int cell_size, grid_n_cols, seg_cell_size, seg_grid_n_cols, boundary;
  // staged tables
  const double* kf_T; const int* kf_pt_off; const int* kf_pt_lm; const int* kf_seg_off; const int* kf_seg_lm;
  const double* pt_pos; const int* pt_type; const int* pt_obs_off;
  const int* pt_obs_kf; const double* pt_obs_px; const double* pt_obs_f; const int* pt_obs_level; const uint8_t* pt_obs_type; const double* pt_obs_grad;
  const double* seg_spos; const double* seg_epos; const int* seg_type; const int* seg_obs_off;
  const int* seg_obs_kf; const double* seg_obs_spx; const double* seg_obs_epx; const double* seg_obs_sf; const double* seg_obs_ef; const int* seg_obs_level;
  const int* pt_cand; const int* seg_cand;
  const int* overlap_idx;           // per run
  // scratch
  unsigned int* visit;              // all ones before EVERY launch: the lowest visit index of a landmark (atomicMin)
  double* kf_pos;                   // 3 per keyframe: Frame::pos()
  int* t_pt_lm; double* t_pt_px; int* t_pt_cell;        // filed points in filing order
  int* t_seg_lm; double* t_seg_px; int* t_seg_cell;     // filed segments: 4 doubles, 2 cells
  // results
  int* counts;                      // 2 per job: n_filed_pt, n_filed_seg
  int* o_pt_lm; double* o_pt_px; int* o_pt_cell; int* o_pt_obs; uint8_t* o_pt_view; uint8_t* o_pt_active;
  int* o_seg_lm; double* o_seg_px; int* o_seg_cell; int* o_seg_obs; uint8_t* o_seg_view; uint8_t* o_seg_active;
  int* kf_count; uint8_t* pt_cand_failed; uint8_t* seg_cand_failed;
  // what MatchBatchDev reads
  double* frame_T; int* frame_slot;
  int* m_cur_frame; int* m_ref_frame; double* m_ref_px; double* m_ref_f; int* m_ref_level; uint8_t* m_ref_type; double* m_ref_grad;
  double* m_pos; double* m_px_cur; uint8_t* m_active;
};

// cell selection of the map candidates (select_device.hpp, include/plsvo_hip.h plsvo_candidates_select): one wave per stream, on the
// arrays the candidate stage (c) and the resident match left on the device.  Per-landmark arrays follow pt_off / seg_off, feature rows
// opt_off (points, at most one per filed point) and 2 * oseg_off (segments, at most two per filed segment).
struct SelectBatchDev {
  CandBatchDev c;
  const uint8_t* found; const double* px_out; const int* search_level;   // the resident match (MatchBatchDev), entries from m_off
  int n_cells, seg_n_cells, max_fts, max_fts_segs, n_pyr_levels;
  const int* cell_order; const int* cell_pos;             // visit position -> cell and its inverse (n_cells entries each)
  const int* seg_cell_order; const int* seg_cell_pos;
  // resident landmark quality
  int* pt_nfail; int* pt_nsucc; int* seg_nfail; int* seg_nsucc;
  uint8_t* pt_event; uint8_t* seg_event;                  // zero before EVERY launch: kSel* bits
  unsigned int* cell_win;                                 // n_cells words per stream, all ones before EVERY launch: the cell's first success
  // the new frame's features, in the order refine() adds them
  int* f_pt_lm; double* f_pt_px; int* f_pt_level; uint8_t* f_pt_type; double* f_pt_grad;
  int* f_seg_lm; double* f_seg_px; int* f_seg_level;
  int* scalars;                                           // 3 per stream: n_matches, n_ls_matches, n_trials
  // pose-optimiser input (PoseBatchDev reads these)
  PoseJobDev* po_jobs; double* pt_f; double* pt_pos; int* pt_level; double* seg_line; double* seg_spos; double* seg_epos; int* seg_level;
  double reproj_thresh; int po_n_iter, ldlt_flavour;
};

// keyframe insertion into the resident map tables (insert_device.hpp, include/plsvo_hip.h plsvo_candidates_insert_keyframe): one wave
// per stream, two launches -- the plan decides and counts in scratch only, the commit builds the new lists in a staging copy of the
// stream's rows and copies them back.  A stream's rows are laid out by capacity (plsvo_candidates_reserve), so they never move.
struct InsertJobDev {               // one stream's record, about 100 bytes
  double T[7];                      // the new keyframe's T_f_w
  const double* d_T;                // device pointer read instead of T, or null
  const uint8_t* pt_keep; const uint8_t* seg_keep;   // the pose optimiser's keep masks in selection order (device)
  int is_kf, remove_kf, kf_slot, reserved0;
};
struct InsertPlanDev {              // what the plan finds: the stream's sizes after the insertion
  int n_kf, new_kf, n_kf_pt, n_kf_seg, n_pt_obs, n_seg_obs, n_pt_cand, n_seg_cand, n_joined_pt, n_joined_seg, n_deleted_pt, n_deleted_seg;
};
struct InsertKindDev {              // one kind of landmark: scratch per landmark (pt_off / seg_off), per candidate entry, per new feature; staging
  unsigned int* f0; unsigned int* f1;   // lowest feature index of the new frame that holds the landmark (all ones: none); highest + 1
  int* cnt;                         // features of the removed keyframe that hold it; bit 16 up: a candidate of the removed keyframe
  int* len; int* erase;             // the new observation list's length; observations in the removed keyframe to erase, -1 = deleted here
  int* cand_kf;                     // per candidate entry: the keyframe its original feature joins, -1 = stays, -2 = deleted with the removed keyframe
  int* new_lm;                      // the new frame's feature list
  int* kf_off2; int* kf_lm2; int* obs_off2; int* obs_kf2; int* obs_level2;
  double* obs_a2; double* obs_b2; double* obs_c2; double* obs_d2; uint8_t* obs_type2;   // points: px, f, grad; segments: spx, epx, sf, ef
};
struct InsertBatchDev {
  SelectBatchDev s;
  const InsertJobDev* jobs; InsertPlanDev* plan;
  InsertKindDev pt, seg;
};
// new candidate landmarks appended to the resident map tables (newcand_device.hpp, include/plsvo_hip.h plsvo_candidates_add): one wave
// per stream.  The records of all streams are concatenated per kind; a stream's begin at pt_at / seg_at.  Its landmark rows, candidate
// list and observation entries have room behind their used part (plsvo_candidates_reserve_landmarks, plsvo_candidates_reserve); the
// host has checked that room against its mirrors before the launch.
struct NewCandJobDev {
  int n_pt, n_seg;
  long long pt_at, seg_at;
};
struct NewCandBatchDev {
  CandBatchDev c;
  int* pt_nfail; int* pt_nsucc; int* seg_nfail; int* seg_nsucc; uint8_t* pt_event; uint8_t* seg_event;   // the resident landmark quality
  const NewCandJobDev* jobs;
  const double* pt_pos; const int* pt_obs_kf; const double* pt_obs_px; const double* pt_obs_f; const int* pt_obs_level; const uint8_t* pt_obs_type;
  const double* pt_obs_grad;        // always present (zeros where the caller gave none)
  const double* seg_spos; const double* seg_epos; const int* seg_obs_kf; const double* seg_obs_spx; const double* seg_obs_epx; const double* seg_obs_sf;
  const double* seg_obs_ef; const int* seg_obs_level;
};
struct PositionsBatchDev {          // plsvo_candidates_set_positions: moved landmarks scattered into the resident tables (global landmark rows)
  int n_pt, n_seg;
  const long long* pt_at; const double* pt_src; const long long* seg_at; const double* seg_ssrc; const double* seg_esrc;
  double* pt_pos; double* seg_spos; double* seg_epos;
};
// structure optimisation on the resident map tables (structsel_device.hpp, include/plsvo_hip.h plsvo_candidates_optimize_structure): one
// wave per stream chooses the least recently refined landmarks among the selection's kept features and refines them in place.
struct StructSelJobDev {            // one stream's record
  const uint8_t* pt_keep; const uint8_t* seg_keep;   // keep masks in selection order (device), whole-batch arrays: rows from opt_off / 2 * oseg_off
  int active, frame_id;
};
struct StructSelBatchDev {
  SelectBatchDev s;
  const StructSelJobDev* jobs;
  int* pt_last_optim; int* seg_last_optim;           // last_structure_optim_ per landmark row of capacity (pt_off / seg_off)
  int max_n_pts, n_iter_pts, max_n_segs, n_iter_segs;   // the caps are also the report's rows per stream
  // the report: 2 counts per stream; per selected entry its landmark, residual evaluations and position(s) behind its run
  int* r_counts; int* r_pt_lm; int* r_pt_iters; double* r_pt_pos; int* r_seg_lm; int* r_seg_iters; double* r_seg_spos; double* r_seg_epos;
};

// compaction of the resident map tables (compact_device.hpp, include/plsvo_hip.h plsvo_candidates_compact): one wave per stream closes
// the stream's rows up over its deleted landmarks, in place.
struct CompactJobDev {              // one stream's record
  int mode, min_room_pt, min_room_seg;               // 0 = stand by, 1 = compact, 2 = a kind only where rows - n_lm < min_room
  int rows_pt, rows_seg, reserved0;                  // the landmark rows the stream was laid out with (CandStreamHost)
};
struct CompactReportDev {           // plsvo_cand_compact_out's counts, field for field
  int ran_pt, ran_seg, n_pt_before, n_pt_after, n_seg_before, n_seg_after, n_pt_obs_before, n_pt_obs_after, n_seg_obs_before, n_seg_obs_after;
  int n_pt_cand_before, n_pt_cand_after, n_seg_cand_before, n_seg_cand_after, n_repointed_pt, n_repointed_seg, n_erased_pt_cand, n_erased_seg_cand;
};
struct CompactBatchDev {
  CandBatchDev c;
  int* pt_nfail; int* pt_nsucc; int* seg_nfail; int* seg_nsucc; uint8_t* pt_event; uint8_t* seg_event;   // the resident landmark quality
  int* pt_key; int* seg_key;                         // last_structure_optim_ per landmark row (StructSelBatchDev)
  const CompactJobDev* jobs; CompactReportDev* report;
  int* pt_remap; int* seg_remap;                     // per landmark row (pt_off / seg_off): its new row, -1 = deleted; written where the kind ran
};

// keyframe stage on the resident map tables (keystage_device.hpp, include/plsvo_hip.h plsvo_candidates_set_keypts / _run_close): one wave
// per stream.  The key-point table holds five entries per keyframe row of CAPACITY (from 5 * kf_off): the position of the key point in
// the keyframe's point-feature list, -1 = NULL.
constexpr int kKeyPtsStandBy = 0, kKeyPtsFresh = 1, kKeyPtsUpkeep = 2;   // KeyPtsJobDev::mode
struct KeyPtsJobDev {               // one stream's record of map_keypts_kernel
  int mode;                         // stand by; every row from five NULLs; the rows one of whose holders has lost its landmark
  int remove_kf;                    // -1, or the row an insertion took out of the keyframe table: the rows above it close up first
  int new_row;                      // kKeyPtsRow*: the LAST row is a new keyframe's, built from five NULLs or from the run's decision record
  int reserved0;
};
constexpr int kKeyPtsRowOld = 0, kKeyPtsRowFresh = 1, kKeyPtsRowDecided = 2;
struct KeyStageBatchDev {
  CandBatchDev c;                   // the resident tables; c.jobs / c.overlap_idx / c.kf_count are the run's rows, which map_close_kernel WRITES
  int* keypts;
  const KfDecideOutDev* decided;    // the run's decision records (kKeyPtsRowDecided), or null
  const KeyPtsJobDev* kp_jobs;      // map_keypts_kernel
  const int* ov_room;               // map_close_kernel: per stream the entries of its overlap row (the keyframe count the host laid it out for)
  int max_n_kfs;
  double* tmp_dist;                 // per keyframe row (kf_off): its distance, -1 = not close
  int* close_idx; double* close_dist;   // per keyframe row (kf_off)
  int* close_counts;                // 2 per stream: n_close, n_overlap
};

// the keyframe decision on the resident selection (keystage_device.hpp's map_keyframe_decide_kernel, plsvo_candidates_keyframe_decide)
struct KeyDecideJobDev {            // one stream's record: 88 bytes
  double T_last[7];
  const double* d_T_last;           // device pointer read instead of T_last, or null
  double min_t, min_r;
  int active, reserved0;            // 0: the stream's record of an earlier decision is left as it is
};
struct KeyDecideBatchDev {
  SelectBatchDev s;                 // the selection's features (f_pt_lm / f_pt_px / f_seg_lm, scalars) and, in s.c, the tables and the run's overlap rows
  const KeyDecideJobDev* jobs; KfDecideOutDev* out;
  const double* poses;              // 7 per stream: the optimised T_f_w (plsvo_candidates_poses_dev)
  const uint8_t* pt_keep; const uint8_t* seg_keep;   // the pose optimiser's keep masks, feature rows from opt_off / 2 * oseg_off
  unsigned long long* depth_keys;   // per stream from opt_off + 4 * oseg_off: n_matches + 2 * n_ls_matches keys (a segment that won both its cells is a feature twice)
  double* delta_t; double* delta_r; // per overlap entry, laid out like the run's overlap rows
};

// the next frame's alignment job from the resident selection (alignjob_device.hpp, include/plsvo_hip.h plsvo_candidates_align_build):
// one wave per stream writes the stream's rows of an alignment batch laid out by CAPACITY -- point rows from job * cap_pts, segment rows
// and slot codes from job * cap_seg, patch slots from job * patch_cap -- so no prefix sum is needed and the rows never move
constexpr int kAlignJobOk = 0, kAlignJobNoRoom = 1;   // AlignBuildReportDev::status (PLSVO_ALIGN_JOB_*)
constexpr int kAlignJobBinGroups = 2, kAlignJobBins = 64 * kAlignJobBinGroups;   // wave-rounds the short segments of one level may open, in groups of 64
constexpr int kAlignJobMaxSlotCap = 64 * (kAlignJobBins - 2);                    // a level of at most this many slots never runs out of them (8064: more than a workgroup's LDS tables hold)
struct AlignBuildJobDev {           // one stream's record
  double T[7];                      // the reference frame's T_f_w
  const double* d_T;                // device pointer read instead of T, or null
  const uint8_t* pt_keep; const uint8_t* seg_keep;   // keep masks in selection order (device), whole-batch arrays: rows from opt_off / 2 * oseg_off
  int active, ref_slot, cur_slot, reserved0;
};
struct AlignBuildReportDev {        // plsvo_cand_align_report, field for field: 32 bytes
  int n_pts, n_seg, n_seg_alive, n_slots, long_mask, status, reserved0, reserved1;
};
struct AlignBuildBatchDev {
  SelectBatchDev s;                 // the selection's features (f_pt_lm / f_pt_px / f_seg_lm / f_seg_px, scalars) and, in s.c, the tables
  const AlignBuildJobDev* jobs; AlignBuildReportDev* report;
  // the resident alignment batch (what AlignBatchDev reads)
  AlignJobDev* a_jobs; double* T0; double* T_ref;
  double* pt_px; double* pt_xyz; double* seg_spx; double* seg_epx; double* seg_len; double* seg_p; double* seg_q; uint8_t* seg_alive_in;
  int* seg_slot;                    // [(level - min_level) * n_jobs * cap_seg + job * cap_seg + segment]
  int* seg_rank;                    // scratch, cap_seg per stream: the short segments of a level in packing order, N << 20 | segment
  int* work_key;                    // per stream: the patches summed over the levels, the key of the build's launch order (kept for a stream that sits a build out)
  int cap_pts, cap_seg, slot_cap, patch_cap;   // per stream; patch_cap = slot_cap rounded up to 4
  int max_level, min_level, n_iter, seg_align, ldlt_flavour, reserved0;
  double eps;
};
struct AlignPoseBatchDev {          // map_align_pose_kernel: T_f_w(new) = T_cur_from_ref * T_ref
  const double* align_poses; const double* T_ref; double* out; int n_jobs;
};

// the alignment job from a RESIDENT KEYFRAME as the reference frame (alignjob_device.hpp map_align_kf_job_kernel, include/plsvo_hip.h
// plsvo_candidates_align_build_kf): the same resident alignment batch, one stream's rows per wave
constexpr int kAlignJobNoKeyframe = 2;                // AlignBuildReportDev::status (PLSVO_ALIGN_JOB_NO_KEYFRAME)
constexpr int kAlignRefClosest = -1;                  // AlignKfJobDev::ref_kf (PLSVO_ALIGN_REF_CLOSEST)
constexpr int kAlignInitHost = 0, kAlignInitDev = 1, kAlignInitKeyframe = 2;   // AlignKfJobDev::init_source (PLSVO_ALIGN_INIT_*)
struct AlignKfJobDev {              // one stream's record: 152 bytes
  double T_init[7];                 // the frame's initial T_f_w (kAlignInitHost; kAlignInitKeyframe without a keyframe)
  double T_last[7];                 // last_frame_->T_f_w_, the frame Map::getClosestKeyframe looks from (kAlignRefClosest)
  const double* d_T_init;           // device pointers read instead (kAlignInitDev; T_last: whenever non-null)
  const double* d_T_last;
  int active, ref_kf, self_kf, init_source, cur_slot, reserved0;
};
struct AlignKfBatchDev {
  AlignBuildBatchDev a;             // the tables (a.s.c) and the resident alignment batch; the selection's rows are not read
  const AlignKfJobDev* jobs;
  const int* keypts;                // the live key-point table, 5 per keyframe row of capacity (kAlignRefClosest), or null
  int* seg_obs;                     // scratch, cap_seg per stream: per segment feature of the keyframe its observation's index, -1 dead
};

// the tracking gates of FrameHandlerMono::processFrame on the resident selection and pose optimisation (alignjob_device.hpp
// map_track_gate_kernel, include/plsvo_hip.h plsvo_candidates_track_gate): a lane per stream
constexpr int kGateTrack = 0, kGateReloc = 1;                       // TrackGateJobDev::mode (PLSVO_GATE_TRACK / _RELOC)
constexpr int kGateOk = 0, kGateFailMatches = 1, kGateFailEdges = 2;   // TrackGateOutDev::result (PLSVO_GATE_*)
constexpr int kTrackInsufficient = 0, kTrackBad = 1, kTrackGood = 2;   // TrackGateOutDev::quality: FrameHandlerBase::TrackingQuality, in its order
struct TrackGateJobDev {            // one stream's record: 104 bytes
  double T_reset[7];                // last_frame_->T_f_w_ (the last well localised pose under kGateReloc)
  const double* d_T_reset;          // device pointer read instead of T_reset, or null
  int active, mode;                 // 0: the stream's record, carried pose and counts are left as they are
  int quality_min_fts, quality_max_drop_fts, max_fts, max_fts_segs;
  int last_resident;                // non-zero: num_obs_last_pt / _ls are the resident ones (this stream's last active call)
  int num_obs_last_pt, num_obs_last_ls, reserved0;
};
struct TrackGateOutDev {            // plsvo_cand_gate_out, field for field: 32 bytes
  int result, quality, n_matched, n_edges, drop_pt, drop_ls;
  int num_obs_last_pt, num_obs_last_ls;   // the counts the drops were taken against
};
struct TrackGateBatchDev {
  const TrackGateJobDev* jobs; TrackGateOutDev* out;
  const int* scalars;               // the selection's, 3 per stream: n_matches, n_ls_matches, n_trials
  const PoseStateDev* state;        // the pose optimiser's record per stream (num_obs_pt, num_obs_ls)
  const double* poses;              // 7 per stream: the optimised T_f_w
  double* carried;                  // 7 per stream: the pose carried forward
  int* obs_last;                    // 2 per stream: num_obs_last_pt, num_obs_last_ls
  int n_jobs, reserved0;
};

// corner detection (detect_device.hpp, include/plsvo_hip.h plsvo_hip_detect_fast): tile geometry and the launch record
constexpr int kDetTileW = 64, kDetTileH = 32;          // pixels of a tile that one workgroup decides
constexpr int kDetImgX0 = 8, kDetImgY0 = 5;            // LDS image origin = tile origin - (8, 5): a halo of 5 (Shi-Tomasi: x - 5 .. x + 4), 8 keeps rows dword-aligned
constexpr int kDetImgW = kDetTileW + 16, kDetImgH = kDetTileH + 10;   // 80 x 42 bytes
constexpr int kDetScoreW = 68, kDetScoreH = kDetTileH + 2;            // scores of the tile + a ring of 1 (66 x 34, rows padded to 68)
constexpr int kDetCellCap = 128;                       // cells of one tile reduced in LDS (640 x 480, cell 25: at most 12 x 6 at level 2)
constexpr int kDetThreads = 256;

struct DetectLaunch {
  const uint8_t* pyr;                 // first slot of the call (slot 0 with a slot table)
  unsigned long long slot_bytes;
  int n_lv;                           // levels of this launch; entry i is pyramid level level[i]
  int level[PLSVO_MAX_LEVELS], w[PLSVO_MAX_LEVELS], h[PLSVO_MAX_LEVELS], tiles_x[PLSVO_MAX_LEVELS];
  unsigned int off[PLSVO_MAX_LEVELS];
  int tile_begin[PLSVO_MAX_LEVELS + 1];   // blockIdx.x in [tile_begin[i], tile_begin[i + 1]) works on entry i
  int fast_b;                         // FAST threshold b
  float thr;                          // (float)detection_threshold: a candidate must score above it
  int cell, cols, n_cells;
  const uint8_t* occupancy;           // n_cells per slot, or null
  unsigned long long* keys;           // n_cells per slot
  uint8_t* stage_score;               // detect_stages only: W_L * H_L each (one slot, one level)
  uint8_t* stage_survives;
  const int* slot_table;              // detect_fast_kernel<false, true> only: position i of the launch reads slot slot_table[i], not slot i; occupancy and keys stay rows of the POSITION
};

// depth-filter seed lists resident on the device (seedlist_device.hpp, include/plsvo_hip.h plsvo_seeds_*): flat SoA rows for the whole
// batch; a stream owns cap_pt / cap_seg rows per kind (multiples of the update kernel's workgroup) from pt_off / seg_off.  The rows are
// SeedsBatchDev's input arrays (pt_ref_frame holds ref_kf, an index into the stream's resident keyframe table), the shadow rows its
// outputs; the map tables are the candidate stage's.
struct SeedStreamDev {
  int n_pt, n_seg;                  // live rows per kind, in list order
  int batch_counter;                // Seed::batch_counter, per stream
  int cap_pt, cap_seg;              // rows as laid out
  int rows_pt, rows_seg, rows_pt_cand, rows_seg_cand, cap_pt_obs, cap_seg_obs;   // the stream's room in the map tables (CandStreamHost)
  int reserved0;
  long long pt_off, seg_off;
};
struct SeedFrameDev {               // one stream's frame of an update
  double T[7];
  const double* d_T;                // device pointer read instead of T, or null
  int active, cur_slot;
};
struct SeedReportDev {              // plsvo_seed_report, field for field
  int pt[6], seg[6];                // rows per PLSVO_SEED_* status
  int first_pt, first_seg, n_pt_seeds, n_seg_seeds, n_pt, n_seg, n_pt_cand, n_seg_cand, n_pt_obs, n_seg_obs, no_room, batch_counter;
};
struct SeedKfJobDev {               // one stream's keyframe event
  int removed_kf, new_batch, new_kf, n_pt, n_seg, reserved0;
  float mu, z_range, sigma2, reserved1;   // the constructor's values (src/depth_filter.cpp:53-74), computed on the host in float
  long long pt_at, seg_at;          // the stream's new seeds in the uploaded arrays
};
struct SeedListBatchDev {
  SeedsBatchDev s;                  // rows in, shadow rows out; frame_T / frame_slot: the candidate stage's frame table (rows from f_off)
  NewCandBatchDev m;                // the map tables and the resident landmark quality (its records are not used)
  SeedStreamDev* streams; const SeedFrameDev* frames; SeedReportDev* report;
  const int* blk_stream;            // per workgroup of the update launch: its stream
  int n_blk_pt, n_blk, n_jobs, max_n_kfs;
  int* pt_batch_id; int* seg_batch_id; double* seg_spx; double* seg_epx;   // rows SeedsBatchDev does not have
  // a keyframe event's upload
  const SeedKfJobDev* kf_jobs;
  const double* k_pt_px; const double* k_pt_f; const int* k_pt_level; const uint8_t* k_pt_type; const double* k_pt_grad;
  const double* k_seg_px; const double* k_seg_f; const double* k_seg_sf; const double* k_seg_ef; const double* k_seg_spx; const double* k_seg_epx; const int* k_seg_level;
};

// a keyframe's point seeds started from its FAST corners (seedlist_device.hpp, include/plsvo_hip.h plsvo_seeds_keyframe_detect): one
// wave per ACTIVE stream in both launches; position p of the launches serves stream jobs[p].stream, and the occupancy row, the key
// row and the slot table entry of the detection between them are rows of the position
struct SeedStartJobDev {
  int stream, removed_kf, new_batch, new_kf, occ_sources, n_seg;
  int n_upd_rows;                   // shadow rows of the last fetched update (OCC_UPDATED)
  int lim_pt;                       // point rows the stream was laid out with
  float mu, z_range, sigma2, reserved0;   // the constructor's values, as SeedKfJobDev's
  long long seg_at;                 // the stream's line seeds in the uploaded arrays
  const uint8_t* d_occ;             // the caller's occupancy bytes, or null
};
struct SeedStartReportDev {         // plsvo_seed_kf_report, field for field
  int n_new_pt, n_new_seg, n_pt_seeds, n_seg_seeds, batch_counter, no_room, n_occupied, reserved0;
};
struct SeedStartBatchDev {
  SeedListBatchDev l;               // the rows, the streams' records, the uploaded line seeds (k_seg_*)
  const SeedStartJobDev* jobs; int n_act;
  int cell, cols, n_cells, width, height;
  const double* f_pt_px; const int* scalars;   // the last selection's features (SelectBatchDev), rows from the stream's opt_off
  uint8_t* occ;                     // n_cells per position, zero before the occupancy launch
  int* slots;                       // the detection's slot table, written by the occupancy launch
  unsigned long long* keys;         // n_cells per position: read, and re-armed, by the start launch
  SeedStartReportDev* report;       // per STREAM
};

// bootstrap KLT (klt_device.hpp, include/plsvo_hip.h plsvo_klt_*).  The KLT pyramids are OpenCV's pyrDown of a slot's level 0, kept in a
// store of their own: pyramid k at store + k * pyr_bytes, level l >= 1 at + off[l] (256-byte aligned, rows tight); stream s owns
// pyramid 2 s (reference frame) and 2 s + 1 (current frame).  Lists are stream-major with cap_pts entries per stream.
constexpr int kKltWin = 30, kKltLevels = PLSVO_KLT_MAX_LEVEL + 1, kKltWaves = 4;
struct KltLevelsDev {
  int n_lv;                          // top level + 1
  int w[kKltLevels], h[kKltLevels];
  unsigned int off[kKltLevels];      // off[0]: level 0 inside a pyramid SLOT
  unsigned long long pyr_bytes;
};
struct KltRowDev { int stream, ref_slot, cur_slot, reserved0; };   // one launch row: an active stream
struct KltStreamDev { double fx, fy, cx, cy; int started, n_calls; };
struct KltFirstDev {
  int stream, n_host, n_extra, reserved0;
  double fx, fy, cx, cy;
  const plsvo_corner* d_corners; const int32_t* d_count;
  long long host_at, extra_at;       // the stream's entries in the uploaded arrays
};
struct KltBatchDev {
  const uint8_t* pyr; unsigned long long slot_bytes;
  uint8_t* store;
  KltLevelsDev lv;
  const KltRowDev* rows; int n_rows;
  int cap_pts, max_iter, min_tracked;
  double eps2, min_eig, min_disparity;
  float* px_ref; float* px_cur; double* f_ref; double* f_cur; double* disparity;
  float* next; uint8_t* status;      // the track launch's results, per list entry
  int* count; KltStreamDev* st; unsigned long long* keys; plsvo_klt_report* report;
  uint8_t* diag_exit; uint8_t* diag_iters;   // plsvo_klt_track_points only: kKltLevels per point
  // a first frame's upload
  const KltFirstDev* first; const float* host_px; const float* extra_px; const double* extra_f;
};

inline int detect_tiles(int w, int h, int* tiles_x) {
  *tiles_x = (w + kDetTileW - 1) / kDetTileW;
  return *tiles_x * ((h + kDetTileH - 1) / kDetTileH);
}


}  // namespace plsvo_hip
