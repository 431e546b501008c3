// capi_ctx.hpp -- what the translation units of the C ABI (plsvo_capi.hip, capi_candidates.hip) share: the kernels' launch functions, the
// device buffers, the context, the error and timing macros, the launch order; staging and readback: capi_transfer.hpp.  Internal: no part of include/plsvo_hip.h, hidden from the dynamic symbol table.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/plsvo_hip.h"
#include "plsvo_dev.hpp"

#define PLSVO_LOCAL __attribute__((visibility("hidden")))

namespace plsvo_hip {
// kernels (align_kernels.hip, poseopt_kernels.hip, pyramid_kernels.hip)
size_t align_level_lds_bytes(int threads, int cap, int scap, int chi_lds_pts);
hipError_t launch_align_reorder(const int* work_key, int n, int* order_out, int shift, hipStream_t stream);   // (the pose optimiser's batches use it too)
hipError_t launch_align_levels(const AlignBatchDev& b, int cap, int scap, int level_hi, int level_lo, int do_init, int threads, size_t lds,
                               hipStream_t stream);
hipError_t launch_pose_opt(const PoseBatchDev& b, double* d_poses, int threads, int select, hipStream_t stream);
hipError_t launch_structopt(const StructBatchDev& s, hipStream_t stream);
hipError_t launch_structopt_solve3(const double* A, const double* b, double* x, int n, hipStream_t stream);
hipError_t launch_match_direct(const MatchBatchDev& b, hipStream_t stream);
hipError_t launch_match_warp_patches(const MatchBatchDev& b, hipStream_t stream);
hipError_t launch_reproject(const ReprojBatchDev& b, hipStream_t stream);
hipError_t launch_update_seeds(const SeedsBatchDev& b, hipStream_t stream);
hipError_t launch_close_keyframes(const CloseKfBatchDev& b, hipStream_t stream);     // keyframe_device.hpp, in seeds_kernels.hip
hipError_t launch_keyframe_decide(const KfDecideBatchDev& b, hipStream_t stream);
hipError_t launch_map_candidates(const CandBatchDev& b, hipStream_t stream);         // candidates_device.hpp, in seeds_kernels.hip
hipError_t launch_map_select(const SelectBatchDev& b, hipStream_t stream);            // select_device.hpp, in seeds_kernels.hip
hipError_t launch_map_insert_plan(const InsertBatchDev& b, hipStream_t stream);       // insert_device.hpp, in seeds_kernels.hip
hipError_t launch_map_insert(const InsertBatchDev& b, hipStream_t stream);
hipError_t launch_map_set_positions(const PositionsBatchDev& b, hipStream_t stream);
hipError_t launch_map_optimize_structure(const StructSelBatchDev& b, hipStream_t stream);   // structsel_device.hpp, in seeds_kernels.hip
hipError_t launch_map_add_candidates(const NewCandBatchDev& b, hipStream_t stream);   // newcand_device.hpp, in seeds_kernels.hip
hipError_t launch_map_compact(const CompactBatchDev& b, hipStream_t stream);           // compact_device.hpp, in seeds_kernels.hip
hipError_t launch_map_keypts(const KeyStageBatchDev& b, hipStream_t stream);          // keystage_device.hpp, in seeds_kernels.hip
hipError_t launch_map_close(const KeyStageBatchDev& b, hipStream_t stream);
hipError_t launch_map_keyframe_decide(const KeyDecideBatchDev& b, hipStream_t stream);
hipError_t launch_map_align_job(const AlignBuildBatchDev& b, hipStream_t stream);      // alignjob_device.hpp, in seeds_kernels.hip
hipError_t launch_map_align_pose(const AlignPoseBatchDev& b, hipStream_t stream);
hipError_t launch_map_align_kf_job(const AlignKfBatchDev& b, hipStream_t stream);
hipError_t launch_map_track_gate(const TrackGateBatchDev& b, hipStream_t stream);
hipError_t launch_update_seeds_resident(const SeedListBatchDev& b, hipStream_t stream);   // seedlist_device.hpp, in seeds_kernels.hip
hipError_t launch_seeds_commit(const SeedListBatchDev& b, hipStream_t stream);
hipError_t launch_seeds_keyframe(const SeedListBatchDev& b, hipStream_t stream);
hipError_t launch_seeds_occupancy(const SeedStartBatchDev& b, hipStream_t stream);
hipError_t launch_seeds_start(const SeedStartBatchDev& b, hipStream_t stream);
hipError_t launch_halfsample(const uint8_t* src, size_t src_pitch, int in_w, int in_h, int in_stride, uint8_t* dst,
                             size_t dst_pitch, int n_slots, int rounding, hipStream_t stream);
hipError_t launch_copy_level0(const uint8_t* src, size_t src_pitch, int w, int h, int stride, uint8_t* dst, size_t dst_pitch,
                              int n_slots, hipStream_t stream);
hipError_t launch_chain_pose(const ChainBatchDev& b, hipStream_t stream);
hipError_t launch_pack_pose_records(const AlignStateDev* ast, const PoseStateDev* pst, int n, plsvo_pose_record* dst, hipStream_t stream);
hipError_t launch_chain_active(const ChainBatchDev& b, hipStream_t stream);
hipError_t launch_chain_select(const ChainBatchDev& b, hipStream_t stream);
hipError_t launch_tile_level(const uint8_t* src, size_t src_pitch, int w, int h, uint8_t* dst, size_t dst_pitch, int n_slots, hipStream_t stream);
hipError_t launch_rectify(const uint8_t* raw, size_t raw_pitch, int stride, int flip, const uint32_t* map, int w, int h, uint8_t* dst,
                          size_t dst_pitch, int n_slots, hipStream_t stream);
hipError_t launch_detect_fast(const DetectLaunch& a, int n_slots, hipStream_t stream);
hipError_t launch_detect_stages(const DetectLaunch& a, hipStream_t stream);
hipError_t launch_detect_compact(unsigned long long* keys, int n_cells, plsvo_corner* corners, int32_t* counts, int n_slots, hipStream_t stream);
hipError_t launch_klt_pyrdown(const KltBatchDev& b, int level, int which, hipStream_t stream);   // klt_device.hpp, in seeds_kernels.hip
hipError_t launch_klt_first(const KltBatchDev& b, int n_jobs, hipStream_t stream);
hipError_t launch_klt_track(const KltBatchDev& b, int max_pts, hipStream_t stream);
hipError_t launch_klt_commit(const KltBatchDev& b, hipStream_t stream);
}  // namespace plsvo_hip

using namespace plsvo_hip;

struct PLSVO_LOCAL DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
    size_t want = std::max(bytes, (size_t)256);
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct PLSVO_LOCAL EventPair { hipEvent_t a, b; };

// Launch order of a RE-RUN resident batch (alignment, pose optimiser): a launch records per job the work it evaluated (key), one small kernel
// behind it (align_kernels.hip::align_reorder_kernel) sorts the jobs most-work-first into the OTHER of two order buffers -- the running
// launch's is never written -- for the next launch.  WHETHER a launch reorders, and what its order is when it does not, is the run functions' decision.
struct plsvo_ctx;
struct PLSVO_LOCAL LaunchOrder {
  DevBuf key, order[2];
  int next = 0;                                        // the order buffer the next sort writes
  int* arm(plsvo_ctx* c, int n);                       // the key of n jobs; a fresh buffer starts at zero work (jobs that leave the kernel early never write theirs).  nullptr: failed, c->err says why
  const int* sort(plsvo_ctx* c, int n, int shift);     // behind the launch that wrote the key: the next launch's order (nullptr: failed)
  void release() { key.release(); order[0].release(); order[1].release(); }
};

struct PLSVO_LOCAL CandStreamHost {      // map candidates: one stream's host mirror of the resident tables' sizes
  int cap_kf, cap_kf_pt, cap_kf_seg, cap_pt_obs, cap_seg_obs;   // capacities the layout was made with: keyframes, features per kind, observations per kind
  int n_kf_pt, n_kf_seg, n_pt_obs, n_seg_obs;                   // used sizes of the last four
  int rows_pt, rows_seg, rows_pt_cand, rows_seg_cand;           // landmark rows and candidate-list rows the layout was made with
  int fetch_pt_cand, fetch_seg_cand;                            // candidate counts a run's fetch reports (an add does not move them)
};
struct PLSVO_LOCAL CandFetchSections {   // ... and where each fetched array starts in cd_d_work, in carve order
  size_t counts, pt_lm, pt_px, pt_cell, pt_obs, pt_view, pt_active, seg_lm, seg_px, seg_cell, seg_obs, seg_view, seg_active, pt_cand_failed, seg_cand_failed;
};

// The pose optimiser's device work set, one per caller of launch_pose_opt: the staged batch (p_w), the frame step (ch_w), the map candidates (cs_w)
struct PLSVO_LOCAL PoseWork {
  DevBuf state, ptkeep, segkeep, s32, s64, poses;
  int ensure(plsvo_ctx* c, size_t n_jobs, size_t n_pt, size_t n_seg);   // room for a batch of n_jobs frames over n_pt points and n_seg segments
  void bind(PoseBatchDev& b) const {
    b.state = state.as<PoseStateDev>(); b.pt_keep = ptkeep.as<uint8_t>(); b.seg_keep = segkeep.as<uint8_t>();
    b.scratch_f32 = s32.as<float>(); b.scratch_f64 = s64.as<double>();
  }
  template <typename B> void bind_resident(PoseBatchDev& q, const B& b, int n) const {   // jobs and features written on the device: ChainBatchDev, SelectBatchDev
    q = PoseBatchDev{}; bind(q); q.jobs = b.po_jobs; q.n_jobs = n;
    q.pt_f = b.pt_f; q.pt_pos = b.pt_pos; q.pt_level = b.pt_level; q.seg_line = b.seg_line; q.seg_spos = b.seg_spos; q.seg_epos = b.seg_epos; q.seg_level = b.seg_level;
  }
  void release() { for (DevBuf* b : { &state, &ptkeep, &segkeep, &s32, &s64, &poses }) b->release(); }
};

struct plsvo_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;
  int cu_count = 0;
  size_t lds_per_block = 65536;
  // experiment switches, read from the environment ONCE, at plsvo_hip_create (never on a launch path)
  int env_align_threads = 0, env_align_lds_pad = 0, env_poseopt_threads = 0;
  bool env_align_per_level = false, env_align_no_lpt = false, env_host_timing = false;
  int ldlt_flavour = 320;   // plsvo_hip_set_option(PLSVO_OPT_LDLT_FLAVOUR)

  // pyramids (row-major slab: half-sampler, matcher, depth filter, download) and their tiled mirror (alignment kernel)
  DevBuf pyr_tiled;
  DevBuf pyr_slab;
  PyrDesc pyr{};
  DevBuf pyr_upload;  // staging for level-0 uploads
  // rectification maps (plsvo_hip_config_rectify): packed words of pyramid_kernels.hip::rectify_kernel, one map per camera
  struct RectifyMap { DevBuf map; int w = 0, h = 0; bool identity = false, flip = false; };
  RectifyMap rect[PLSVO_MAX_RECTIFY_MAPS];
  int rect_n = 0;
  // corner detection (plsvo_hip_detect_fast*): one 64-bit key per (slot, cell), 0 between calls (detect_device.hpp); staging of the host form
  DevBuf det_keys, det_occ, det_corners, det_counts, det_stage;

  // alignment batch
  int a_n = 0;
  bool a_staged = false;
  std::vector<AlignJobDev> a_jobs;
  std::vector<int> a_nseg_off;  // per job seg offset (host copy)
  int a_total_seg = 0;
  int a_gmax = -1, a_gmin = 99;
  int a_cap[PLSVO_MAX_LEVELS]{};
  int a_scap = 4;   // max segments of one job
  int a_trace_cap = 0;
  DevBuf a_d_state, a_d_alive;   // (inputs: a_d_blob)
  DevBuf a_d_pxyz, a_d_puv, a_d_cref, a_d_chi, a_d_log, a_d_poses;
  int a_run_threads = 0;                    // threads per frame of the last plsvo_align_run (plsvo_align_fetch_records)
  size_t a_patch_total = 0;                 // patch slots of the staged batch (all jobs, all levels' maximum)
  int a_seg_align = 32;                     // the staged layout's segment alignment (64: two workgroups per frame are possible)
  LaunchOrder a_order;                      // launch order of a RE-RUN resident batch, from the patch-iterations its last launch evaluated
  bool env_align_no_reorder = false;
  const int* a_stage_order = nullptr;          // the staged batch's own order (most patches first), inside a_d_blob
  bool a_one_shot = false, p_one_shot = false;   // set around the run of a one-shot batch call: its launch order is never consumed
  int env_align_reorder_min = 0;            //   PLSVO_ALIGN_REORDER_MIN: smallest batch that is re-ordered (tests; default 16 frames per CU)
  // tail split of the one-wave-per-frame alignment launch (align_kernels.hip): PLSVO_OPT_ALIGN_TAIL_SPLIT, and for tests and measurements
  // PLSVO_ALIGN_TAIL_MIN (smallest batch that is split; default four times the resident workgroups), PLSVO_ALIGN_TAIL_K (tail set in
  // multiples of the resident workgroups; default 2), PLSVO_ALIGN_TAIL_FRAMES (the tail set itself, in frames)
  bool opt_align_tail_split = true;
  int env_align_tail_min = 0, env_align_tail_k = 0, env_align_tail_frames = 0;
  DevBuf a_d_tailflag;                      //   one flag word per tail frame, zeroed before every launch
  DevBuf a_d_alive_tail;                    //   the coarse parts' working copy of the segment flags
  DevBuf a_d_xbuf;                          // two workgroups per frame: their exchange granules (2 KB per frame, zeroed once)
  unsigned int x_launch = 0;                // launches that used it (tags = launch << 10 | exchange: never repeated)
  bool env_align_no_pair = false;
  AlignBatchDev a_b{};

  // pose-opt batch
  int p_n = 0;
  bool p_staged = false;
  std::vector<PoseJobDev> p_jobs;
  int p_total_pt = 0, p_total_seg = 0;
  int p_trace_cap = 0;
  PoseWork p_w;                             // (inputs: p_d_blob)
  DevBuf p_d_log;
  PoseBatchDev p_b{};
  LaunchOrder p_order;                      // as a_order, from its last launch's feature-iterations
  int p_key_shift = 0;
  bool env_poseopt_no_reorder = false;
  int env_poseopt_reorder_min = 0;          //   PLSVO_POSEOPT_REORDER_MIN (tests)
  // row refill of the row shape's Gauss-Newton loop (poseopt_kernels.hip: three launches): PLSVO_OPT_POSEOPT_REFILL, and for tests and
  // measurements PLSVO_POSEOPT_REFILL_MIN (smallest batch that takes it, in frames; default: more than two frames per resident row) and
  // PLSVO_POSEOPT_REFILL_WAVES (workgroups of the persistent kernel; default: the resident ones)
  bool opt_poseopt_refill = true;
  int env_poseopt_refill_min = 0, env_poseopt_refill_waves = 0;
  // medians of the row kernels (poseopt_select.hpp): values once into registers, rank finish -- PLSVO_OPT_POSEOPT_SELECT; false = row_radix_select everywhere
  bool opt_poseopt_select = true;
  // 6x6 solve of the alignment (plsvo_wave.hpp::wave_solve6_core): pivot order sorted once, no per-step search -- PLSVO_OPT_ALIGN_STATIC_SOLVE; false = the search in every step
  bool opt_align_static_solve = true;
  bool p_any_ref = false;                   //   a job of the staged batch has a refinement loop (n_iter_ref > 0): pose_opt_rows_kernel
  int p_refill_frames = 0;                  //   frames the last pose-optimiser launch ran through the three launches
  DevBuf p_d_carry, p_d_refill_next;        //   PoseRefillCarry per job; the queue's counter

  // resident frame step (plsvo_chain_*): candidates, glue state, pose-optimiser input written on the device
  bool ch_staged = false;
  int ch_n = 0, ch_ncand = 0, ch_npt_cap = 0, ch_nseg_cap = 0;
  std::vector<ChainJobDev> ch_jobs;
  DevBuf ch_d_blob, ch_d_work, ch_d_po;
  ChainBatchDev ch_b{};
  MatchBatchDev ch_match{};
  ReprojBatchDev ch_reproj{};
  PoseBatchDev ch_pose{};
  PoseWork ch_w;
  DevBuf rec_d;   // plsvo_fetch_pose_records
  // map candidates (plsvo_candidates_*): the staged tables (cd_d_blob), results / scratch / the matcher's arrays (cd_d_work), a run's frames
  bool cd_staged = false, cd_ran = false, cd_matched = false;
  int cd_n = 0, cd_max_level = 0;
  std::vector<CandMapDev> cd_maps;
  std::vector<int> cd_kf_slot, cd_cur_slot;
  std::vector<int64_t> cd_m_off, cd_f_off;
  std::vector<long long> cd_ov_off;         // per stream of the last run: where its overlap list starts (n + 1 entries)
  CandFetchSections cd_off{};               // sections of the fetched part of cd_d_work
  size_t cd_fetch_bytes = 0, cd_vis_off = 0, cd_vis_bytes = 0, cd_total_m = 0, cd_total_f = 0;
  plsvo_cand_params cd_params{};
  DevBuf cd_d_blob, cd_d_work, cd_d_run, cd_d_kfcount;
  CandBatchDev cd_b{};
  MatchBatchDev cd_match{};
  // their cell selection (plsvo_candidates_select ..): the resident landmark quality (cs_d_q: counters, then the event bytes), the
  // launch's scratch, the features and the pose optimiser's input (cs_d_work), the visit orders of the two grids (cs_d_order)
  bool cs_selected = false, cs_posed = false;
  size_t cd_t_pt = 0, cd_t_seg = 0, cd_t_ptc = 0, cd_t_segc = 0, cd_t_opt = 0, cd_t_oseg = 0;
  std::vector<int> cs_order;                // what cs_d_order holds: order, positions, for the points' grid and the segments'
  DevBuf cs_d_q, cs_d_work, cs_d_order;
  PoseWork cs_w;
  SelectBatchDev cs_b{};
  PoseBatchDev cs_pose{};
  // keyframe insertion (plsvo_candidates_insert_keyframe ..): the room plsvo_candidates_reserve asks for (ci_reserve: the next stage's),
  // per stream its capacities and used sizes (cd_host), the capacity totals, the last insertion's report; scratch and staging rows
  // (ci_d_work), a call's records and host masks (ci_d_in)
  plsvo_cand_reserve ci_reserve{};
  std::vector<CandStreamHost> cd_host;
  size_t ci_t_kf = 0, ci_t_kfpt = 0, ci_t_kfseg = 0, ci_t_ptobs = 0, ci_t_segobs = 0, cd_blob_bytes = 0;
  bool ci_inserted = false, ci_have_out = false;
  std::vector<InsertPlanDev> ci_last;
  DevBuf ci_d_work, ci_d_in, ci_d_plan, ci_d_pos;
  // structure optimisation on the resident tables (plsvo_candidates_optimize_structure ..): last_structure_optim_ per landmark row of
  // capacity, an allocation of its own zeroed at stage time (co_d_key: points, then segments); a call's records and host masks (co_d_in);
  // the report (co_d_rep) and the launch that wrote it (co_b); whether this run was optimised, whether there is a report since the stage
  bool co_done = false, co_have_out = false;
  DevBuf co_d_key, co_d_in, co_d_rep;
  size_t co_rep_bytes = 0;
  StructSelBatchDev co_b{};
  // new candidate landmarks (plsvo_candidates_add ..): the landmark room plsvo_candidates_reserve_landmarks asks for (cn_reserve: the next
  // stage's), per stream the rows its layout was made with and the candidate counts a run's fetch reports (cd_host), whether an add
  // closed the open run, the last report
  plsvo_cand_lm_reserve cn_reserve{};
  bool cn_closed = false, cn_have_out = false;
  std::vector<plsvo_cand_add_out> cn_last;
  DevBuf cn_d_in;
  // compaction over the deleted landmark rows (plsvo_candidates_compact ..): whether one closed the open run, the last report (valid until
  // the tables move again), a call's records (cc_d_in), the reports and the per-landmark remap scratch (cc_d_work: points, then segments)
  bool cc_closed = false, cc_have_out = false;
  std::vector<CompactReportDev> cc_last;
  DevBuf cc_d_in, cc_d_work;
  size_t cc_remap_off = 0, cc_remap_seg = 0, cc_work_end = 0;   // sections of cc_d_work: the two remaps, the end
  // keyframe stage on the resident tables (plsvo_candidates_set_keypts ..): the key-point table, 5 per keyframe row of capacity, and
  // whether it is live (ck_d_keypts, ck_live); a call's upload and the standing "upkeep" records of every stream (ck_d_in, ck_d_upkeep);
  // the close launch's results, then its scratch (ck_d_work), whether the last run was a run_close, the launch that describes both
  bool ck_live = false, ck_have_close = false;
  DevBuf ck_d_keypts, ck_d_in, ck_d_upkeep, ck_d_work;
  size_t ck_fetch_bytes = 0;
  KeyStageBatchDev ck_b{};
  // the keyframe decision on the resident selection (plsvo_candidates_keyframe_decide): the last run's job records and overlap rows on
  // the device (inside cd_d_run), a call's records (ck_d_dec_in), the decision records / deltas / depth keys (ck_d_dec: zeroed when it
  // grows, a stream that sits a call out keeps its record), whether this run has a decision
  const CandJobDev* cd_run_jobs = nullptr; const int* cd_run_ov = nullptr;
  bool ck_decided = false;
  std::vector<uint8_t> ck_dec_active;        // per stream: a decision of this run was active for it
  DevBuf ck_d_dec_in, ck_d_dec;
  KeyDecideBatchDev ck_dec_b{};
  // the next frame's alignment job built from the selection (plsvo_candidates_align_*): the reserve's configuration and stream count, the
  // resident alignment batch laid out by capacity (aj_d_batch: what a_b points at while aj_built), a call's records and host masks
  // (aj_d_in), the reports / the reference poses / the composed poses (aj_d_out), per stream the pyramid slots of its last build (the
  // host's a_jobs mirror needs them), whether the staged alignment batch is the built one, whether its poses were composed
  bool aj_reserved = false, aj_built = false, aj_composed = false;
  int aj_n = 0;
  plsvo_cand_align_cfg aj_cfg{};
  std::vector<int> aj_slots;
  DevBuf aj_d_batch, aj_d_in, aj_d_out, aj_d_order;   // (aj_d_order: the build's own launch order, which no later launch's re-ordering writes)
  AlignBuildBatchDev aj_b{};              // the batch's sections (the selection, the records and the key are bound per call)
  AlignPoseBatchDev aj_pose{};
  int* aj_seg_obs = nullptr;              // a keyframe build's scratch inside aj_d_batch: cap_seg observation indices per stream
  std::vector<std::vector<int>> aj_kf_slots;   // per stream built against its CLOSEST keyframe: every keyframe slot it may have picked (the tiled mirror's upkeep)
  DevBuf aj_d_kf_in;                      // a keyframe build's records
  // the tracking gates behind the pose optimisation (plsvo_candidates_track_gate ..): a call's records (tg_d_in); the gate records, the
  // carried poses and num_obs_last_pt / _ls per stream (tg_d_out: zeroed at the first gate behind a stage, a stream that sits a call
  // out keeps its rows), the stream count they were laid out for, whether there is a gate since the stage
  bool tg_have = false;
  int tg_n = 0;
  DevBuf tg_d_in, tg_d_out;
  TrackGateBatchDev tg_b{};
  // resident seed lists (plsvo_seeds_*): the room plsvo_seeds_reserve asks for (the next stage's), per stream the host mirror of its
  // record (sd_host: list lengths, upper bounds between a keyframe event and the next update fetch) and the rows it may fill (sd_lim);
  // the tables (sd_d_tab: records, workgroup map, rows), shadow rows and reports (sd_d_work), a call's upload (sd_d_in).  A candidate
  // restage drops them (sd_staged); between an update and its fetch the candidate tables are the device's alone (sd_pending)
  plsvo_seed_reserve sd_reserve{};
  bool sd_staged = false, sd_pending = false, sd_have_report = false;
  int sd_n = 0, sd_max_level = 0;
  plsvo_seed_params sd_params{};
  std::vector<SeedStreamDev> sd_host;
  std::vector<int> sd_lim;                  // 2 per stream: rows a list may hold (staged count + reserve)
  std::vector<SeedReportDev> sd_last;
  size_t sd_tab_bytes = 0, sd_t_pt = 0, sd_t_seg = 0;
  DevBuf sd_d_tab, sd_d_work, sd_d_in;
  SeedListBatchDev sd_b{};
  // seeds started from a keyframe's corners (plsvo_seeds_keyframe_detect): the occupancy rows and the slot table of the active streams
  // (sk_d_occ, sk_d_slots: per position of the launch), the reports (sk_d_report: per stream, zeroed at plsvo_seeds_stage)
  bool sk_have_report = false;
  DevBuf sk_d_occ, sk_d_slots, sk_d_report;
  // bootstrap KLT (plsvo_klt_*, capi_klt.hpp): the reserve's configuration, the level-0 size and slab it was laid out for, per stream the
  // reference slot of its first frame; the KLT pyramid store (kl_d_store), the lists / results / records (kl_d_lists), a call's rows and
  // host lists (kl_d_in), the diagnostic's store and arrays (kl_d_diag)
  bool kl_reserved = false;
  plsvo_klt_cfg kl_cfg{};
  const uint8_t* kl_pyr_base = nullptr;
  std::vector<int> kl_ref_slot;
  DevBuf kl_d_store, kl_d_lists, kl_d_in, kl_d_diag;
  KltBatchDev kl_b{};
  unsigned long long run_seq = 0, a_run_seq = 0, p_run_seq = 0, ch_run_seq = 0;   // which resident batch ran last, 0 = not since it was staged (plsvo_pack_pose_records)
  unsigned long long ch_stage_seq = 0;      // when the frame step was staged, on the same count: a pose-optimisation batch that ran later describes the streams now

  // structure optimisation (one-shot batches)
  DevBuf s_d_in, s_d_out;

  // staging: one blob per batch type (Blob), pinned bounce buffer for small ones
  DevBuf a_d_blob, p_d_blob;
  // pinned bounce buffers of the stage calls: two, used in turn, each guarded by an event recorded behind its last DMA
  void* pinned[2] = { nullptr, nullptr };
  size_t pinned_cap[2] = { 0, 0 };
  hipEvent_t pinned_done[2] = { nullptr, nullptr };
  int pinned_next = 0;
  // the same for whole pyramids (plsvo_hip_upload_pyramid packs a frame's levels into one pinned image of its slot: ONE DMA, no wait)
  void* pyr_pinned[2] = { nullptr, nullptr };
  size_t pyr_pinned_cap[2] = { 0, 0 };
  hipEvent_t pyr_pinned_done[2] = { nullptr, nullptr };
  int pyr_pinned_next = 0;
  // slots whose TILED mirror is stale: an uploaded pyramid is re-tiled only when a launch that reads the mirror (the one-wave-per-frame
  // shape of the alignment) is about to use it -- a per-frame caller never pays the four tile launches
  std::vector<uint8_t> tiled_stale;
  int tiled_stale_count = 0;
  // results of a fetch come back through a pinned buffer (device-to-PAGEABLE copies are staged and waited for one by one by the driver)
  void* dl_pinned = nullptr;
  size_t dl_pinned_cap = 0;

  // profiling
  bool profiling = false;
  std::vector<EventPair> ev[PLSVO_K_COUNT];
  std::vector<EventPair> ev_pool;
  double ev_ms[PLSVO_K_COUNT]{};
  int64_t ev_launches[PLSVO_K_COUNT]{};
};

#define CTX_CHECK(ctx) do { if (!(ctx)) return PLSVO_E_INVALID; } while (0)
#define HIP_FAIL_IF(ctx, e, what)                                                               \
  do {                                                                                          \
    if ((e) != hipSuccess) {                                                                    \
      (ctx)->err = std::string(what) + ": " + hipGetErrorString(e);                             \
      return PLSVO_E_HIP;                                                                       \
    }                                                                                           \
  } while (0)
#define HIP_TRY(ctx, expr) do { const hipError_t e__ = (expr); HIP_FAIL_IF(ctx, e__, #expr); } while (0)
static inline int fail(plsvo_ctx* ctx, int code, const std::string& msg) { ctx->err = msg; return code; }

PLSVO_LOCAL void prof_begin(plsvo_ctx* c, int k, EventPair* ep);   // helpers both units use, defined in plsvo_capi.hip
PLSVO_LOCAL void prof_end(plsvo_ctx* c, int k, EventPair* ep);
// HIP_TRY of a launch expression between the two events of kernel family k: the event pair goes back to the pool whether the launch failed or not
#define HIP_TRY_TIMED(ctx, k, expr)                                                             \
  do {                                                                                          \
    EventPair ep__{};                                                                           \
    prof_begin((ctx), (k), &ep__);                                                              \
    const hipError_t e__ = (expr);                                                              \
    prof_end((ctx), (k), &ep__);                                                                \
    HIP_FAIL_IF(ctx, e__, #expr);                                                               \
  } while (0)

#include "capi_transfer.hpp"

inline int* LaunchOrder::arm(plsvo_ctx* c, int n) {
  const auto grow = [&]() -> int {
    HIP_TRY(c, key.ensure((size_t)n * sizeof(int)));
    HIP_TRY(c, hipMemsetAsync(key.p, 0, key.cap, c->stream));
    return PLSVO_OK;
  };
  return (key.cap >= (size_t)n * sizeof(int) || grow() == PLSVO_OK) ? key.as<int>() : nullptr;
}
inline const int* LaunchOrder::sort(plsvo_ctx* c, int n, int shift) {
  DevBuf& ob = order[next];
  const auto enqueue = [&]() -> int {
    HIP_TRY(c, ob.ensure((size_t)n * sizeof(int)));
    HIP_TRY(c, launch_align_reorder(key.as<int>(), n, ob.as<int>(), shift, c->stream));
    return PLSVO_OK;
  };
  if (enqueue() != PLSVO_OK) return nullptr;
  next ^= 1;
  return ob.as<int>();
}

PLSVO_LOCAL int pose_opt_threads(const plsvo_ctx* c, int n, long feats);
// launch configuration of the fused alignment kernel for n_jobs frames of at most `cap` slots, `scap` segments, `max_pts` points (defined in plsvo_capi.hip)
PLSVO_LOCAL void pick_align_config(const plsvo_ctx* c, int n_jobs, int cap, int scap, int max_pts, int* threads, size_t* lds, int* chi_lds_pts);
// corner detection, shared by plsvo_hip_detect_fast(_dev) and plsvo_seeds_keyframe_detect (defined in plsvo_capi.hip).  detect_check_params:
// everything the detect entry points refuse in their params, for n launch positions; the pyramids are configured and p is not NULL.
// detect_enqueue_keys: the detection launch alone -- position i reads slot first_slot + i, or d_slot_table[i] when a table is given --
// into the context's armed key rows
PLSVO_LOCAL int detect_check_params(plsvo_ctx* c, int n, const plsvo_detect_params* p, const char* what, int* cols, int* rows);
PLSVO_LOCAL int detect_enqueue_keys(plsvo_ctx* c, int first_slot, const int* d_slot_table, int n, const plsvo_detect_params* p, int cells, int cols, const uint8_t* d_occ);
PLSVO_LOCAL void pose_state_to_out(const PoseStateDev& s, plsvo_poseopt_out& o);   // everything but the keep masks, whose two pointers it leaves as they are
