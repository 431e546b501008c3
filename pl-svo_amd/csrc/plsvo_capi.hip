// plsvo_capi.hip -- implementation of the C ABI declared in include/plsvo_hip.h.
// Host side only: context, HBM buffers, staging of flattened features, kernel launches, result fetch,
// hipEvent timing, RCCL gather.  All device work is enqueued on the ctx stream; nothing here computes
// any part of the hot path on the CPU (there is no fallback).
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/plsvo_hip.h"
#include "plsvo_dev.hpp"
#include "plsvo_math.hpp"
#include "poseopt_refill.hpp"
#include "poseopt_select.hpp"

namespace plsvo_hip {
// kernels (align_kernels.hip, poseopt_kernels.hip, pyramid_kernels.hip)
size_t align_level_lds_bytes(int threads, int cap, int scap, int chi_lds_pts);
hipError_t launch_align_reorder(const int* work_key, int n, int* order_out, int shift, hipStream_t stream);   // (the pose optimiser's batches use it too)
hipError_t launch_align_levels(const AlignBatchDev& b, int cap, int scap, int level_hi, int level_lo, int do_init, int threads, size_t lds,
                               hipStream_t stream);
hipError_t launch_pose_opt(const PoseBatchDev& b, double* d_poses, int threads, int select, hipStream_t stream);
hipError_t launch_structopt(const StructBatchDev& s, hipStream_t stream);
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
hipError_t launch_map_add_candidates(const NewCandBatchDev& b, hipStream_t stream);   // newcand_device.hpp, in seeds_kernels.hip
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
}  // namespace plsvo_hip

using namespace plsvo_hip;

static thread_local std::string g_create_error;

namespace {

struct DevBuf {
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

struct EventPair { hipEvent_t a, b; };

// All input arrays of a staged batch travel as ONE host-to-device copy: sections of a single blob, each 256-byte aligned.
// (A single-frame call used to pay a dozen small pageable copies; small blobs go through a pinned staging buffer.)
struct Blob {
  std::vector<uint8_t> host;
  template <typename T> size_t add(const std::vector<T>& v) {
    const size_t off = (host.size() + 255) & ~(size_t)255;
    host.resize(off + std::max(v.size() * sizeof(T), (size_t)16));
    if (!v.empty()) memcpy(host.data() + off, v.data(), v.size() * sizeof(T));
    return off;
  }
  // a section of n elements to be filled in place: take the pointers (at<T>) only after the LAST reserve / add, which may move the blob
  template <typename T> size_t reserve(size_t n) {
    const size_t off = (host.size() + 255) & ~(size_t)255;
    host.resize(off + std::max(n * sizeof(T), (size_t)16));
    return off;
  }
  template <typename T> T* at(size_t off) { return reinterpret_cast<T*>(host.data() + off); }
};

}  // namespace

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
  size_t a_patch_total = 0;                 // patch slots of the staged batch (all jobs, all levels' maximum)
  int a_seg_align = 32;                     // the staged layout's segment alignment (64: two workgroups per frame are possible)
  DevBuf a_d_workkey;                       // per job: the patch-iterations its last launch evaluated
  DevBuf a_d_order[2];                      // launch order of a RE-RUN resident batch: sorted on the device by the last launch's measured work
  int a_order_next = 0;                     //   (align_kernels.hip::align_reorder_kernel); the buffer the next reorder writes
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
  DevBuf p_d_state, p_d_ptkeep, p_d_segkeep;   // (inputs: p_d_blob)
  DevBuf p_d_s32, p_d_s64, p_d_log, p_d_poses;
  PoseBatchDev p_b{};
  DevBuf p_d_workkey, p_d_order[2];         // as a_d_workkey / a_d_order: the launch order of a re-run staged batch, from its last launch's feature-iterations
  int p_order_next = 0, p_key_shift = 0;
  bool env_poseopt_no_reorder = false;
  int env_poseopt_reorder_min = 0;          //   PLSVO_POSEOPT_REORDER_MIN (tests)
  // row refill of the row shape's Gauss-Newton loop (poseopt_kernels.hip: three launches): PLSVO_OPT_POSEOPT_REFILL, and for tests and
  // measurements PLSVO_POSEOPT_REFILL_MIN (smallest batch that takes it, in frames; default: more than two frames per resident row) and
  // PLSVO_POSEOPT_REFILL_WAVES (workgroups of the persistent kernel; default: the resident ones)
  bool opt_poseopt_refill = true;
  int env_poseopt_refill_min = 0, env_poseopt_refill_waves = 0;
  // medians of the row kernels (poseopt_select.hpp): values once into registers, rank finish -- PLSVO_OPT_POSEOPT_SELECT; false = row_radix_select everywhere
  bool opt_poseopt_select = true;
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
  DevBuf ch_d_state, ch_d_ptkeep, ch_d_segkeep, ch_d_s32, ch_d_s64, ch_d_poses;
  DevBuf rec_d;   // plsvo_fetch_pose_records
  // map candidates (plsvo_candidates_*): the staged tables (cd_d_blob), results / scratch / the matcher's arrays (cd_d_work), a run's frames
  bool cd_staged = false, cd_ran = false, cd_matched = false;
  int cd_n = 0, cd_max_level = 0;
  std::vector<CandMapDev> cd_maps;
  std::vector<int> cd_kf_slot, cd_cur_slot;
  std::vector<int64_t> cd_m_off, cd_f_off;
  std::vector<long long> cd_ov_off;         // per stream of the last run: where its overlap list starts (n + 1 entries)
  std::vector<size_t> cd_off;               // sections of the fetched part of cd_d_work
  size_t cd_fetch_bytes = 0, cd_vis_off = 0, cd_vis_bytes = 0, cd_total_m = 0, cd_total_f = 0;
  plsvo_cand_params cd_params{};
  DevBuf cd_d_blob, cd_d_work, cd_d_run, cd_d_kfcount;
  CandBatchDev cd_b{};
  MatchBatchDev cd_match{};
  // their cell selection (plsvo_candidates_select ..): the resident landmark quality (cs_d_q: counters, then the event bytes), the
  // launch's scratch, the features and the pose optimiser's input (cs_d_work), the visit orders of the two grids (cs_d_order)
  bool cs_selected = false, cs_posed = false;
  size_t cd_t_pt = 0, cd_t_seg = 0, cd_t_ptc = 0, cd_t_segc = 0, cd_t_opt = 0, cd_t_oseg = 0;
  size_t cs_ev_off = 0, cs_win_bytes = 0;
  std::vector<int> cs_order;                // what cs_d_order holds: order, positions, for the points' grid and the segments'
  DevBuf cs_d_q, cs_d_work, cs_d_order, cs_d_state, cs_d_ptkeep, cs_d_segkeep, cs_d_s32, cs_d_s64, cs_d_poses;
  SelectBatchDev cs_b{};
  PoseBatchDev cs_pose{};
  // keyframe insertion (plsvo_candidates_insert_keyframe ..): the room plsvo_candidates_reserve asks for (ci_reserve: the next stage's),
  // per stream its capacities (ci_cap: keyframes, features per kind, observations per kind) and used sizes (ci_used: the last four),
  // the capacity totals, the last insertion's report; scratch and staging rows (ci_d_work), a call's records and host masks (ci_d_in)
  plsvo_cand_reserve ci_reserve{};
  std::vector<int> ci_cap, ci_used;
  size_t ci_t_kf = 0, ci_t_kfpt = 0, ci_t_kfseg = 0, ci_t_ptobs = 0, ci_t_segobs = 0, cd_blob_bytes = 0;
  bool ci_inserted = false, ci_have_out = false;
  std::vector<InsertPlanDev> ci_last;
  DevBuf ci_d_work, ci_d_in, ci_d_plan, ci_d_pos;
  // new candidate landmarks (plsvo_candidates_add ..): the landmark room plsvo_candidates_reserve_landmarks asks for (cn_reserve: the next
  // stage's), per stream the rows its layout was made with (cn_cap: point rows, segment rows, point candidates, segment candidates), the
  // candidate counts a run's fetch reports (cd_fetch_cand: an add does not move them), whether an add closed the open run, the last report
  plsvo_cand_lm_reserve cn_reserve{};
  std::vector<int> cn_cap, cd_fetch_cand;
  bool cn_closed = false, cn_have_out = false;
  std::vector<plsvo_cand_add_out> cn_last;
  DevBuf cn_d_in;
  unsigned long long run_seq = 0, a_run_seq = 0, p_run_seq = 0, ch_run_seq = 0;   // which resident batch ran last, 0 = not since it was staged (plsvo_pack_pose_records)

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
#define HIP_TRY(ctx, expr)                                                                      \
  do {                                                                                          \
    hipError_t e__ = (expr);                                                                    \
    if (e__ != hipSuccess) {                                                                    \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e__);                          \
      return PLSVO_E_HIP;                                                                       \
    }                                                                                           \
  } while (0)
static int fail(plsvo_ctx* ctx, int code, const std::string& msg) { ctx->err = msg; return code; }

// ---- profiling helpers ----------------------------------------------------------------------
static void prof_begin(plsvo_ctx* c, int k, EventPair* ep) {
  if (!c->profiling) return;
  if (!c->ev_pool.empty()) { *ep = c->ev_pool.back(); c->ev_pool.pop_back(); }
  else { (void)hipEventCreate(&ep->a); (void)hipEventCreate(&ep->b); }
  (void)hipEventRecord(ep->a, c->stream);
  (void)k;
}
static void prof_end(plsvo_ctx* c, int k, EventPair* ep) {
  if (!c->profiling) return;
  (void)hipEventRecord(ep->b, c->stream);
  c->ev[k].push_back(*ep);
}
static void prof_collect(plsvo_ctx* c) {
  for (int k = 0; k < PLSVO_K_COUNT; ++k) {
    for (auto& ep : c->ev[k]) {
      float ms = 0.f;
      if (hipEventSynchronize(ep.b) == hipSuccess && hipEventElapsedTime(&ms, ep.a, ep.b) == hipSuccess) {
        c->ev_ms[k] += (double)ms; c->ev_launches[k] += 1;
      }
      c->ev_pool.push_back(ep);
    }
    c->ev[k].clear();
  }
}

// ---- context ---------------------------------------------------------------------------------
extern "C" const char* plsvo_hip_version(void) { return "plsvo_hip 0.1 (gfx950)"; }

static int create_ctx(int device_id, void* stream, bool use_given_stream, plsvo_ctx** out);
static bool env_flag(const char* name) { const char* s = getenv(name); return s && *s && strcmp(s, "0") != 0; }   // set and not "0"
extern "C" int plsvo_hip_create(int device_id, void* stream, plsvo_ctx** out) { return create_ctx(device_id, stream, stream != nullptr, out); }
extern "C" int plsvo_hip_create_on_stream(int device_id, void* stream, plsvo_ctx** out) { return create_ctx(device_id, stream, true, out); }

static int create_ctx(int device_id, void* stream, bool use_given_stream, plsvo_ctx** out) {
  if (!out) return PLSVO_E_INVALID;
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    g_create_error = std::string("no HIP device available (") + (e != hipSuccess ? hipGetErrorString(e) : "count=0") +
                     "); plsvo_hip has no CPU fallback";
    return PLSVO_E_NODEVICE;
  }
  if (device_id < 0 || device_id >= n) { g_create_error = "device_id out of range"; return PLSVO_E_INVALID; }
  if ((e = hipSetDevice(device_id)) != hipSuccess) { g_create_error = hipGetErrorString(e); return PLSVO_E_HIP; }
  plsvo_ctx* c = new plsvo_ctx();
  c->device = device_id;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) {
    c->cu_count = prop.multiProcessorCount;
    c->lds_per_block = prop.sharedMemPerBlock;
    int optin = 0;
    if (hipDeviceGetAttribute(&optin, hipDeviceAttributeMaxSharedMemoryPerBlock, device_id) == hipSuccess && optin > 0)
      c->lds_per_block = std::max(c->lds_per_block, (size_t)optin);
  }
  if (use_given_stream) { c->stream = reinterpret_cast<hipStream_t>(stream); c->own_stream = false; }   // NULL = HIP's default stream
  else {
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) {
      g_create_error = hipGetErrorString(e); delete c; return PLSVO_E_HIP;
    }
    c->own_stream = true;
  }
  if (const char* s = getenv("PLSVO_LDS_LIMIT")) c->lds_per_block = (size_t)atol(s);
  if (const char* s = getenv("PLSVO_ALIGN_THREADS")) { const int v = atoi(s); if (v == 64 || v == 128 || v == 256 || v == 512) c->env_align_threads = v; }
  if (const char* s = getenv("PLSVO_ALIGN_LDS_PAD")) c->env_align_lds_pad = std::max(0, atoi(s));
  if (const char* s = getenv("PLSVO_POSEOPT_THREADS")) { const int v = atoi(s); if (v == 16 || v == 64 || v == 256 || v == 512) c->env_poseopt_threads = v; }
  if (const char* s = getenv("PLSVO_ALIGN_PER_LEVEL")) c->env_align_per_level = atoi(s) != 0;
  c->env_align_no_lpt = env_flag("PLSVO_ALIGN_NO_LPT");
  c->env_align_no_pair = env_flag("PLSVO_ALIGN_NO_PAIR");   // (A/B: one workgroup per frame also for small batches)
  c->env_align_no_reorder = env_flag("PLSVO_ALIGN_NO_REORDER");   // (A/B: keep the stage call's patch-count order for every launch)
  if (const char* s = getenv("PLSVO_ALIGN_REORDER_MIN")) c->env_align_reorder_min = atoi(s);
  if (const char* s = getenv("PLSVO_ALIGN_TAIL_SPLIT")) c->opt_align_tail_split = atoi(s) != 0;
  if (const char* s = getenv("PLSVO_ALIGN_TAIL_MIN")) c->env_align_tail_min = atoi(s);
  if (const char* s = getenv("PLSVO_ALIGN_TAIL_K")) c->env_align_tail_k = atoi(s);
  if (const char* s = getenv("PLSVO_ALIGN_TAIL_FRAMES")) c->env_align_tail_frames = atoi(s);
  c->env_poseopt_no_reorder = env_flag("PLSVO_POSEOPT_NO_REORDER");
  if (const char* s = getenv("PLSVO_POSEOPT_REORDER_MIN")) c->env_poseopt_reorder_min = atoi(s);
  if (const char* s = getenv("PLSVO_POSEOPT_REFILL")) c->opt_poseopt_refill = atoi(s) != 0;
  if (const char* s = getenv("PLSVO_POSEOPT_SELECT")) c->opt_poseopt_select = atoi(s) != 0;
  if (const char* s = getenv("PLSVO_POSEOPT_REFILL_MIN")) c->env_poseopt_refill_min = atoi(s);
  if (const char* s = getenv("PLSVO_POSEOPT_REFILL_WAVES")) c->env_poseopt_refill_waves = atoi(s);
  c->env_host_timing = getenv("PLSVO_HOST_TIMING") != nullptr;
  *out = c;
  return PLSVO_OK;
}

extern "C" void plsvo_hip_destroy(plsvo_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  prof_collect(c);
  for (auto& ep : c->ev_pool) { (void)hipEventDestroy(ep.a); (void)hipEventDestroy(ep.b); }
  c->a_d_tailflag.release(); c->a_d_alive_tail.release(); c->a_d_xbuf.release(); c->a_d_order[0].release(); c->a_d_order[1].release(); c->a_d_workkey.release(); c->p_d_workkey.release(); c->p_d_order[0].release(); c->p_d_order[1].release();
  c->p_d_carry.release(); c->p_d_refill_next.release();
  c->cd_d_blob.release(); c->cd_d_work.release(); c->cd_d_run.release(); c->cd_d_kfcount.release();
  for (DevBuf* b : { &c->ci_d_work, &c->ci_d_in, &c->ci_d_plan, &c->ci_d_pos, &c->cn_d_in }) b->release();
  for (DevBuf* b : { &c->cs_d_q, &c->cs_d_work, &c->cs_d_order, &c->cs_d_state, &c->cs_d_ptkeep, &c->cs_d_segkeep, &c->cs_d_s32, &c->cs_d_s64, &c->cs_d_poses }) b->release();
  DevBuf* bufs[] = { &c->pyr_slab, &c->pyr_tiled, &c->pyr_upload, &c->a_d_blob, &c->a_d_state, &c->a_d_alive, &c->a_d_pxyz, &c->a_d_puv, &c->a_d_cref,
                     &c->a_d_chi, &c->a_d_log, &c->a_d_poses, &c->p_d_blob, &c->p_d_state, &c->p_d_ptkeep, &c->p_d_segkeep, &c->p_d_s32, &c->p_d_s64,
                     &c->p_d_log, &c->p_d_poses, &c->s_d_in, &c->s_d_out, &c->ch_d_blob, &c->ch_d_work, &c->ch_d_po, &c->ch_d_state,
                     &c->ch_d_ptkeep, &c->ch_d_segkeep, &c->ch_d_s32, &c->ch_d_s64, &c->ch_d_poses, &c->rec_d };
  for (DevBuf* b : bufs) b->release();
  for (auto& r : c->rect) r.map.release();
  c->det_keys.release(); c->det_occ.release(); c->det_corners.release(); c->det_counts.release(); c->det_stage.release();
  for (int k = 0; k < 2; ++k) { if (c->pinned[k]) (void)hipHostFree(c->pinned[k]); if (c->pinned_done[k]) (void)hipEventDestroy(c->pinned_done[k]); }
  for (int k = 0; k < 2; ++k) { if (c->pyr_pinned[k]) (void)hipHostFree(c->pyr_pinned[k]); if (c->pyr_pinned_done[k]) (void)hipEventDestroy(c->pyr_pinned_done[k]); }
  if (c->dl_pinned) (void)hipHostFree(c->dl_pinned);
  if (c->own_stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

extern "C" int plsvo_hip_set_option(plsvo_ctx* c, int option, int value) {
  CTX_CHECK(c);
  if (option == PLSVO_OPT_LDLT_FLAVOUR) {
    if (value != 320 && value != 330) return fail(c, PLSVO_E_INVALID, "set_option: the LDLT flavour is 320 (Eigen 3.1 ... 3.2.1) or 330 (Eigen 3.2.2 and later)");
    c->ldlt_flavour = value;
    c->a_staged = false; c->p_staged = false;   // the rule travels with the staged jobs
    return PLSVO_OK;
  }
  if (option == PLSVO_OPT_ALIGN_THREADS) {
    if (value != 0 && value != 64 && value != 128 && value != 256 && value != 512) return fail(c, PLSVO_E_INVALID, "set_option: alignment launch shape is 0 (automatic), 64, 128, 256 or 512 threads per frame");
    c->env_align_threads = value;
    return PLSVO_OK;
  }
  if (option == PLSVO_OPT_POSEOPT_THREADS) {
    if (value != 0 && value != 16 && value != 64 && value != 256 && value != 512) return fail(c, PLSVO_E_INVALID, "set_option: pose-optimiser launch shape is 0 (automatic), 16 (a 16-lane row per frame, four frames per wave), 64, 256 or 512 threads per frame");
    c->env_poseopt_threads = value;
    return PLSVO_OK;
  }
  if (option == PLSVO_OPT_ALIGN_REORDER || option == PLSVO_OPT_POSEOPT_REORDER) {
    if (value != 0 && value != 1) return fail(c, PLSVO_E_INVALID, "set_option: the launch-order refresh is 0 (keep the stage order) or 1 (refresh from the last launch's measured work)");
    if (option == PLSVO_OPT_ALIGN_REORDER) {
      c->env_align_no_reorder = value == 0;
      if (value == 0 && c->a_staged && c->a_d_blob.p) c->a_b.order = c->a_stage_order;   // back to the stage call's order
    } else {
      c->env_poseopt_no_reorder = value == 0;
    }
    return PLSVO_OK;
  }
  if (option == PLSVO_OPT_ALIGN_TAIL_SPLIT) {
    if (value != 0 && value != 1) return fail(c, PLSVO_E_INVALID, "set_option: the alignment's tail split is 0 (one workgroup per frame throughout) or 1 (the frames that start last run as a coarse and a fine part)");
    c->opt_align_tail_split = value != 0;
    return PLSVO_OK;
  }
  if (option == PLSVO_OPT_POSEOPT_REFILL) {
    if (value != 0 && value != 1) return fail(c, PLSVO_E_INVALID, "set_option: the pose optimiser's row refill is 0 (four frames of a wave in lock step) or 1 (rows take their next frame from a queue)");
    c->opt_poseopt_refill = value != 0;
    return PLSVO_OK;
  }
  if (option == PLSVO_OPT_POSEOPT_SELECT) {
    if (value != 0 && value != 1) return fail(c, PLSVO_E_INVALID, "set_option: the row kernels' median select is 0 (radix select over memory, every digit) or 1 (values in registers, rank finish)");
    c->opt_poseopt_select = value != 0;
    return PLSVO_OK;
  }
  return fail(c, PLSVO_E_INVALID, "set_option: unknown option");
}

extern "C" const char* plsvo_hip_last_error(const plsvo_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }
extern "C" void* plsvo_hip_stream(plsvo_ctx* c) { return c ? reinterpret_cast<void*>(c->stream) : nullptr; }
extern "C" int plsvo_hip_synchronize(plsvo_ctx* c) { CTX_CHECK(c); HIP_TRY(c, hipStreamSynchronize(c->stream)); return PLSVO_OK; }

extern "C" int plsvo_hip_device_info(plsvo_ctx* c, char* name, int name_len, int* cu_count, size_t* hbm_bytes) {
  CTX_CHECK(c);
  hipDeviceProp_t prop;
  HIP_TRY(c, hipGetDeviceProperties(&prop, c->device));
  if (name && name_len > 0) { snprintf(name, (size_t)name_len, "%s (%s)", prop.name, prop.gcnArchName); }
  if (cu_count) *cu_count = prop.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = prop.totalGlobalMem;
  return PLSVO_OK;
}

// ---- pyramids ----------------------------------------------------------------------------------
extern "C" int plsvo_hip_config_pyramids(plsvo_ctx* c, int n_slots, int width, int height, int n_levels) {
  CTX_CHECK(c);
  if (n_slots <= 0 || width <= 0 || height <= 0 || n_levels <= 0 || n_levels > PLSVO_MAX_LEVELS) return fail(c, PLSVO_E_INVALID, "config_pyramids: bad arguments");
  HIP_TRY(c, hipSetDevice(c->device));
  PyrDesc d{};
  size_t off = 0;
  for (int l = 0; l < n_levels; ++l) {
    d.w[l] = width >> l; d.h[l] = height >> l;
    if (d.w[l] <= 0 || d.h[l] <= 0) return fail(c, PLSVO_E_INVALID, "config_pyramids: too many levels for this image size");
    d.off[l] = pyr_level_offset(width, height, l);
    off = (size_t)pyr_level_offset(width, height, l + 1);           // >= 64 bytes of slack after every level (gather over-read)
  }
  d.slot_bytes = off; d.n_slots = n_slots; d.n_levels = n_levels;
  d.tslot_bytes = pyr_tiled_level_offset(width, height, n_levels);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, c->pyr_slab.ensure((size_t)n_slots * off + 256));
  HIP_TRY(c, hipMemsetAsync(c->pyr_slab.p, 0, (size_t)n_slots * off + 256, c->stream));
  HIP_TRY(c, c->pyr_tiled.ensure((size_t)n_slots * d.tslot_bytes + 256));
  HIP_TRY(c, hipMemsetAsync(c->pyr_tiled.p, 0, (size_t)n_slots * d.tslot_bytes + 256, c->stream));
  d.base = c->pyr_slab.as<uint8_t>();
  d.tbase = c->pyr_tiled.as<uint8_t>();
  c->pyr = d;
  c->tiled_stale.assign((size_t)n_slots, 0); c->tiled_stale_count = 0;
  c->a_staged = false;
  c->ch_staged = false;
  return PLSVO_OK;
}

static int check_slot(plsvo_ctx* c, int slot) {
  if (!c->pyr.base) return fail(c, PLSVO_E_STATE, "pyramids not configured");
  if (slot < 0 || slot >= c->pyr.n_slots) return fail(c, PLSVO_E_CAPACITY, "pyramid slot out of range");
  return PLSVO_OK;
}

// refresh the tiled mirror of slots [first_slot, first_slot + n), levels [0, n_levels): enqueued after whatever wrote the slab
static int retile(plsvo_ctx* c, int first_slot, int n, int n_levels) {
  const uint8_t* src = c->pyr_slab.as<uint8_t>() + (size_t)first_slot * c->pyr.slot_bytes;
  uint8_t* dst = c->pyr_tiled.as<uint8_t>() + (size_t)first_slot * c->pyr.tslot_bytes;
  for (int l = 0; l < n_levels; ++l)
    HIP_TRY(c, launch_tile_level(src + c->pyr.off[l], c->pyr.slot_bytes, c->pyr.w[l], c->pyr.h[l],
                                 dst + pyr_tiled_level_offset(c->pyr.w[0], c->pyr.h[0], l), c->pyr.tslot_bytes, n, c->stream));
  return PLSVO_OK;
}

// the tiled mirror of every slot in [first, first + n) is current again (whoever calls this has just enqueued retile() for them)
static void mark_tiled_fresh(plsvo_ctx* c, int first, int n) {
  if (c->tiled_stale_count == 0) return;
  for (int s = first; s < first + n && s < (int)c->tiled_stale.size(); ++s)
    if (c->tiled_stale[(size_t)s]) { c->tiled_stale[(size_t)s] = 0; --c->tiled_stale_count; }
}
// re-tile the stale slots among `slots` (a launch that reads the mirror is about to be enqueued behind this)
static int retile_stale(plsvo_ctx* c, const std::vector<int>& slots) {
  if (c->tiled_stale_count == 0) return PLSVO_OK;
  for (int sl : slots) {
    if (sl < 0 || sl >= (int)c->tiled_stale.size() || !c->tiled_stale[(size_t)sl]) continue;
    int rc = retile(c, sl, 1, c->pyr.n_levels); if (rc) return rc;
    c->tiled_stale[(size_t)sl] = 0; --c->tiled_stale_count;
    if (c->tiled_stale_count == 0) break;
  }
  return PLSVO_OK;
}

extern "C" int plsvo_hip_upload_pyramid(plsvo_ctx* c, int slot, int n_levels, const uint8_t* const* level_ptr, const int* width,
                                        const int* height, const int* stride_bytes) {
  CTX_CHECK(c);
  int rc = check_slot(c, slot); if (rc) return rc;
  if (!level_ptr || !width || !height || !stride_bytes || n_levels <= 0 || n_levels > c->pyr.n_levels) return fail(c, PLSVO_E_INVALID, "upload_pyramid: bad arguments");
  HIP_TRY(c, hipSetDevice(c->device));
  for (int l = 0; l < n_levels; ++l) {
    if (!level_ptr[l] || width[l] != c->pyr.w[l] || height[l] != c->pyr.h[l] || stride_bytes[l] < width[l])
      return fail(c, PLSVO_E_INVALID, "upload_pyramid: level size does not match the configured pyramid");
  }
  uint8_t* const slot_dst = c->pyr_slab.as<uint8_t>() + (size_t)slot * c->pyr.slot_bytes;
  // The levels are packed into a pinned image of the slot (rows tight, every level at its offset) and cross PCIe as ONE copy enqueued on
  // the stream: the caller's buffers are free when the call returns, nothing is waited for, and whatever is launched next on the stream
  // reads the new pyramid.  (Until round 4: one pageable 2-D copy per level -- each staged by the driver -- four tile launches and a stream
  // synchronisation, ~45 us of a 0.4 ms SparseImgAlign::run.)  Two pinned images, each guarded by an event behind its last DMA.
  const size_t image_bytes = (size_t)c->pyr.off[n_levels - 1] + (size_t)width[n_levels - 1] * (size_t)height[n_levels - 1];
  const int k = c->pyr_pinned_next;
  if (!c->pyr_pinned_done[k] && hipEventCreate(&c->pyr_pinned_done[k]) != hipSuccess) c->pyr_pinned_done[k] = nullptr;
  bool packed = false;
  if (c->pyr_pinned_done[k]) {
    HIP_TRY(c, hipEventSynchronize(c->pyr_pinned_done[k]));   // the DMA that last read this image has landed (no-op when never recorded)
    if (c->pyr_pinned_cap[k] < image_bytes) {
      if (c->pyr_pinned[k]) (void)hipHostFree(c->pyr_pinned[k]);
      c->pyr_pinned[k] = nullptr; c->pyr_pinned_cap[k] = 0;
      if (hipHostMalloc(&c->pyr_pinned[k], (size_t)c->pyr.slot_bytes, hipHostMallocDefault) == hipSuccess) {
        c->pyr_pinned_cap[k] = (size_t)c->pyr.slot_bytes;
        memset(c->pyr_pinned[k], 0, c->pyr_pinned_cap[k]);   // (the slack between the levels travels with them)
      }
    }
    if (c->pyr_pinned[k]) {
      uint8_t* const img = static_cast<uint8_t*>(c->pyr_pinned[k]);
      for (int l = 0; l < n_levels; ++l) {
        uint8_t* d = img + c->pyr.off[l];
        const size_t w = (size_t)width[l];
        if ((size_t)stride_bytes[l] == w) memcpy(d, level_ptr[l], w * (size_t)height[l]);
        else for (int y = 0; y < height[l]; ++y) memcpy(d + (size_t)y * w, level_ptr[l] + (size_t)y * (size_t)stride_bytes[l], w);
      }
      HIP_TRY(c, hipMemcpyAsync(slot_dst, img, image_bytes, hipMemcpyHostToDevice, c->stream));
      HIP_TRY(c, hipEventRecord(c->pyr_pinned_done[k], c->stream));
      c->pyr_pinned_next = k ^ 1;
      packed = true;
    }
  }
  if (!packed) {   // no pinned memory: straight from the caller's buffers, which must stay untouched until the copies have landed
    for (int l = 0; l < n_levels; ++l)
      HIP_TRY(c, hipMemcpy2DAsync(slot_dst + c->pyr.off[l], (size_t)width[l], level_ptr[l], (size_t)stride_bytes[l], (size_t)width[l], (size_t)height[l],
                                  hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  if (!c->tiled_stale[(size_t)slot]) { c->tiled_stale[(size_t)slot] = 1; ++c->tiled_stale_count; }
  return PLSVO_OK;
}

static int build_levels(plsvo_ctx* c, int first_slot, int n, int rounding) {
  uint8_t* base = c->pyr_slab.as<uint8_t>() + (size_t)first_slot * c->pyr.slot_bytes;
  for (int l = 1; l < c->pyr.n_levels; ++l) {
    EventPair ep{}; prof_begin(c, PLSVO_K_HALFSAMPLE, &ep);
    HIP_TRY(c, launch_halfsample(base + c->pyr.off[l - 1], c->pyr.slot_bytes, c->pyr.w[l - 1], c->pyr.h[l - 1], c->pyr.w[l - 1],
                                 base + c->pyr.off[l], c->pyr.slot_bytes, n, rounding, c->stream));
    prof_end(c, PLSVO_K_HALFSAMPLE, &ep);
  }
  // (the slots count as fresh only once their tile launches are enqueued: a failed launch leaves them stale and the next launch that
  //  reads the mirror tries again -- ADVICE r05)
  const int rc_t = retile(c, first_slot, n, c->pyr.n_levels);
  if (rc_t) {
    for (int s = first_slot; s < first_slot + n && s < (int)c->tiled_stale.size(); ++s)
      if (!c->tiled_stale[(size_t)s]) { c->tiled_stale[(size_t)s] = 1; ++c->tiled_stale_count; }
    return rc_t;
  }
  mark_tiled_fresh(c, first_slot, n);
  return PLSVO_OK;
}

extern "C" int plsvo_hip_build_pyramid(plsvo_ctx* c, int slot, const uint8_t* level0, int stride_bytes, int rounding) {
  CTX_CHECK(c);
  int rc = check_slot(c, slot); if (rc) return rc;
  if (!level0 || stride_bytes < c->pyr.w[0]) return fail(c, PLSVO_E_INVALID, "build_pyramid: bad arguments");
  HIP_TRY(c, hipSetDevice(c->device));
  uint8_t* dst = c->pyr_slab.as<uint8_t>() + (size_t)slot * c->pyr.slot_bytes + c->pyr.off[0];
  HIP_TRY(c, hipMemcpy2DAsync(dst, (size_t)c->pyr.w[0], level0, (size_t)stride_bytes, (size_t)c->pyr.w[0], (size_t)c->pyr.h[0],
                              hipMemcpyHostToDevice, c->stream));
  rc = build_levels(c, slot, 1, rounding); if (rc) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PLSVO_OK;
}

extern "C" int plsvo_hip_build_pyramids_dev(plsvo_ctx* c, int first_slot, int n, const void* d_level0, int stride_bytes,
                                            size_t image_pitch_bytes, int rounding) {
  CTX_CHECK(c);
  if (n <= 0 || !d_level0) return fail(c, PLSVO_E_INVALID, "build_pyramids_dev: bad arguments");
  int rc = check_slot(c, first_slot); if (rc) return rc;
  rc = check_slot(c, first_slot + n - 1); if (rc) return rc;
  if (stride_bytes < c->pyr.w[0]) return fail(c, PLSVO_E_INVALID, "build_pyramids_dev: stride smaller than width");
  HIP_TRY(c, hipSetDevice(c->device));
  uint8_t* base = c->pyr_slab.as<uint8_t>() + (size_t)first_slot * c->pyr.slot_bytes;
  HIP_TRY(c, launch_copy_level0(reinterpret_cast<const uint8_t*>(d_level0), image_pitch_bytes, c->pyr.w[0], c->pyr.h[0], stride_bytes,
                                base + c->pyr.off[0], c->pyr.slot_bytes, n, c->stream));
  return build_levels(c, first_slot, n, rounding);
}

// "cur becomes ref" for a block of streams without crossing PCIe: device-to-device copy of whole slots, row-major slab and tiled
// mirror alike (src/frame_handler_mono.cpp:272-274: the frame aligned against in the next call is the one just tracked)
extern "C" int plsvo_hip_copy_slots(plsvo_ctx* c, int dst_first, int src_first, int n) {
  CTX_CHECK(c);
  if (n <= 0) return fail(c, PLSVO_E_INVALID, "copy_slots: bad arguments");
  int rc = check_slot(c, dst_first); if (rc) return rc;
  rc = check_slot(c, dst_first + n - 1); if (rc) return rc;
  rc = check_slot(c, src_first); if (rc) return rc;
  rc = check_slot(c, src_first + n - 1); if (rc) return rc;
  if (dst_first < src_first + n && src_first < dst_first + n) return fail(c, PLSVO_E_INVALID, "copy_slots: the two slot ranges overlap");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(c->pyr_slab.as<uint8_t>() + (size_t)dst_first * c->pyr.slot_bytes, c->pyr_slab.as<uint8_t>() + (size_t)src_first * c->pyr.slot_bytes,
                            (size_t)n * c->pyr.slot_bytes, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->pyr_tiled.as<uint8_t>() + (size_t)dst_first * c->pyr.tslot_bytes, c->pyr_tiled.as<uint8_t>() + (size_t)src_first * c->pyr.tslot_bytes,
                            (size_t)n * c->pyr.tslot_bytes, hipMemcpyDeviceToDevice, c->stream));
  for (int k = 0; k < n; ++k) {   // a stale mirror stays stale in its copy (and a fresh one replaces a stale one)
    const uint8_t st = c->tiled_stale[(size_t)(src_first + k)];
    uint8_t& dt = c->tiled_stale[(size_t)(dst_first + k)];
    if (st != dt) { c->tiled_stale_count += st ? 1 : -1; dt = st; }
  }
  return PLSVO_OK;
}

extern "C" int plsvo_hip_download_level(plsvo_ctx* c, int slot, int level, uint8_t* out) {
  CTX_CHECK(c);
  int rc = check_slot(c, slot); if (rc) return rc;
  if (level < 0 || level >= c->pyr.n_levels || !out) return fail(c, PLSVO_E_INVALID, "download_level: bad arguments");
  HIP_TRY(c, hipSetDevice(c->device));
  const uint8_t* src = c->pyr_slab.as<uint8_t>() + (size_t)slot * c->pyr.slot_bytes + c->pyr.off[level];
  HIP_TRY(c, hipMemcpyAsync(out, src, (size_t)c->pyr.w[level] * c->pyr.h[level], hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PLSVO_OK;
}

// ---- rectification of raw distorted frames ------------------------------------------------------
// vk::PinholeCamera::undistortImage ([ext] vikit): cv::remap(raw, out, map1, map2, INTER_LINEAR) through the map the camera's
// constructor builds with cv::initUndistortRectifyMap(K, D, I, K, size, CV_16SC2); K and D are cv::Mat_<float>.  OpenCV 3.x, scalar
// path, restated operation for operation (DESIGN.md "Rectification"); tests/np_rectify.py is the independent NumPy restatement.
static int cv_round(double v) {   // cvRound = _mm_cvtsd_si32: half to even, 0x80000000 when the result does not fit
  if (!(v >= -2147483648.5 && v < 2147483647.5)) return INT32_MIN;
  return (int)std::nearbyint(v);
}

static bool rectify_cam_ok(const plsvo_pinhole_radtan* cam) {
  if (!cam || cam->cam.width < 1 || cam->cam.height < 1 || cam->cam.width > 2046 || cam->cam.height > 2046) return false;   // 11-bit x0 + 1, y0 + 1
  const double p[4] = { cam->cam.fx, cam->cam.fy, cam->cam.cx, cam->cam.cy };
  for (double v : p) if (!std::isfinite(v) || !std::isfinite((float)v)) return false;
  for (double v : cam->d) if (!std::isfinite(v) || !std::isfinite((float)v)) return false;
  return (float)cam->cam.fx != 0.f && (float)cam->cam.fy != 0.f;   // (a singular K: OpenCV's invert fails)
}

static void rectify_map_build(const plsvo_pinhole_radtan* cam, int16_t* xy, uint16_t* frac) {
#pragma clang fp contract(off)
  const int W = cam->cam.width, H = cam->cam.height;
  // cameraMatrix = newCameraMatrix = K (float -> double), R = I: iR = (K * I).inv(DECOMP_LU) -- for 3x3 the closed form of
  // cv::invert (adjugate times 1/det3)
  double A[9] = { (double)(float)cam->cam.fx, 0., (double)(float)cam->cam.cx, 0., (double)(float)cam->cam.fy, (double)(float)cam->cam.cy, 0., 0., 1. };
  double Ar[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Ar[i * 3 + j] = A[i * 3 + 0] * (j == 0 ? 1. : 0.) + A[i * 3 + 1] * (j == 1 ? 1. : 0.) + A[i * 3 + 2] * (j == 2 ? 1. : 0.);
#define M(i, j) Ar[(i) * 3 + (j)]
  double d = M(0, 0) * (M(1, 1) * M(2, 2) - M(1, 2) * M(2, 1)) - M(0, 1) * (M(1, 0) * M(2, 2) - M(1, 2) * M(2, 0)) +
             M(0, 2) * (M(1, 0) * M(2, 1) - M(1, 1) * M(2, 0));
  d = 1. / d;
  double ir[9];
  ir[0] = (M(1, 1) * M(2, 2) - M(1, 2) * M(2, 1)) * d;
  ir[1] = (M(0, 2) * M(2, 1) - M(0, 1) * M(2, 2)) * d;
  ir[2] = (M(0, 1) * M(1, 2) - M(0, 2) * M(1, 1)) * d;
  ir[3] = (M(1, 2) * M(2, 0) - M(1, 0) * M(2, 2)) * d;
  ir[4] = (M(0, 0) * M(2, 2) - M(0, 2) * M(2, 0)) * d;
  ir[5] = (M(0, 2) * M(1, 0) - M(0, 0) * M(1, 2)) * d;
  ir[6] = (M(1, 0) * M(2, 1) - M(1, 1) * M(2, 0)) * d;
  ir[7] = (M(0, 1) * M(2, 0) - M(0, 0) * M(2, 1)) * d;
  ir[8] = (M(0, 0) * M(1, 1) - M(0, 1) * M(1, 0)) * d;
#undef M
  const double u0 = A[2], v0 = A[5], fx = A[0], fy = A[4];
  const double k1 = (double)(float)cam->d[0], k2 = (double)(float)cam->d[1], p1 = (double)(float)cam->d[2], p2 = (double)(float)cam->d[3],
               k3 = (double)(float)cam->d[4], k4 = 0., k5 = 0., k6 = 0.;
  for (int i = 0; i < H; ++i) {
    int16_t* m1 = xy + (size_t)i * W * 2;
    uint16_t* m2 = frac + (size_t)i * W;
    double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
    for (int j = 0; j < W; ++j, _x += ir[0], _y += ir[3], _w += ir[6]) {
      const double w = 1. / _w, x = _x * w, y = _y * w;
      const double x2 = x * x, y2 = y * y;
      const double r2 = x2 + y2, _2xy = 2 * x * y;
      const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
      const double xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2);
      const double yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy;
      const double u = fx * xd + u0, v = fy * yd + v0;   // (tilt matrix = I, invProj = 1)
      const int iu = cv_round(u * 32), iv = cv_round(v * 32);
      m1[j * 2] = (int16_t)(iu >> 5);
      m1[j * 2 + 1] = (int16_t)(iv >> 5);
      m2[j] = (uint16_t)((iv & 31) * 32 + (iu & 31));
    }
  }
}

extern "C" int plsvo_rectify_map(const plsvo_pinhole_radtan* cam, int16_t* xy, uint16_t* frac) {
  if (!rectify_cam_ok(cam) || !xy || !frac) return PLSVO_E_INVALID;
  rectify_map_build(cam, xy, frac);
  return PLSVO_OK;
}

extern "C" int plsvo_hip_config_rectify(plsvo_ctx* c, const plsvo_pinhole_radtan* cam, int flip_vertical, int* map_id) {
  CTX_CHECK(c);
  if (!map_id || !rectify_cam_ok(cam)) return fail(c, PLSVO_E_INVALID, "config_rectify: bad camera (non-finite or zero focal length, size outside 1..2046)");
  if (!c->pyr.base) return fail(c, PLSVO_E_STATE, "config_rectify: pyramids not configured");
  if (cam->cam.width != c->pyr.w[0] || cam->cam.height != c->pyr.h[0]) return fail(c, PLSVO_E_INVALID, "config_rectify: camera size does not match the configured pyramid");
  if (c->rect_n >= PLSVO_MAX_RECTIFY_MAPS) return fail(c, PLSVO_E_CAPACITY, "config_rectify: every rectification map of the context is in use");
  const int W = cam->cam.width, H = cam->cam.height, qw = (W + 3) >> 2;
  const bool identity = !(std::fabs(cam->d[0]) > 0.0000001);   // vikit: distortion_ = fabs(d0) > 0.0000001
  std::vector<int16_t> xy((size_t)W * H * 2);
  std::vector<uint16_t> fr((size_t)W * H);
  if (identity) {   // undistortImage copies; only the flipped copy goes through the remap kernel (an identity map: a copy, bit for bit)
    for (int i = 0; i < H; ++i)
      for (int j = 0; j < W; ++j) { xy[((size_t)i * W + j) * 2] = (int16_t)j; xy[((size_t)i * W + j) * 2 + 1] = (int16_t)i; fr[(size_t)i * W + j] = 0; }
  } else {
    rectify_map_build(cam, xy.data(), fr.data());
  }
  // pack: rows padded to 4 words (padding = a pixel whose taps are all outside)
  std::vector<uint32_t> packed((size_t)qw * 4 * H, (uint32_t)(W + 1) << 10);
  for (int i = 0; i < H; ++i)
    for (int j = 0; j < W; ++j) {
      const size_t k = (size_t)i * W + j;
      const int x0 = xy[k * 2], y0 = xy[k * 2 + 1];
      uint32_t word = (uint32_t)(W + 1) << 10;   // every tap outside the raw frame: 0
      if (x0 >= -1 && x0 < W && y0 >= -1 && y0 < H) word = (uint32_t)fr[k] | ((uint32_t)(x0 + 1) << 10) | ((uint32_t)(y0 + 1) << 21);
      packed[(size_t)i * qw * 4 + j] = word;
    }
  HIP_TRY(c, hipSetDevice(c->device));
  plsvo_ctx::RectifyMap& r = c->rect[c->rect_n];
  HIP_TRY(c, r.map.ensure(packed.size() * sizeof(uint32_t)));
  HIP_TRY(c, hipMemcpyAsync(r.map.p, packed.data(), packed.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the packed words live on this call's stack)
  r.w = W; r.h = H; r.identity = identity; r.flip = flip_vertical != 0;
  *map_id = c->rect_n++;
  return PLSVO_OK;
}

// checks shared by the two rectifying builders: every failure is PLSVO_E_INVALID and nothing has been enqueued
static int rectify_check(plsvo_ctx* c, int map_id, int first_slot, int n, int stride_bytes, const char* what) {
  if (!c->pyr.base) return fail(c, PLSVO_E_STATE, std::string(what) + ": pyramids not configured");
  if (map_id < 0 || map_id >= c->rect_n) return fail(c, PLSVO_E_INVALID, std::string(what) + ": unknown rectification map");
  const plsvo_ctx::RectifyMap& r = c->rect[map_id];
  if (r.w != c->pyr.w[0] || r.h != c->pyr.h[0]) return fail(c, PLSVO_E_INVALID, std::string(what) + ": camera size does not match the configured pyramid");
  if (n <= 0 || first_slot < 0 || first_slot > c->pyr.n_slots - n) return fail(c, PLSVO_E_INVALID, std::string(what) + ": slot range out of bounds");
  if (stride_bytes < r.w || (long long)stride_bytes * r.h > INT32_MAX) return fail(c, PLSVO_E_INVALID, std::string(what) + ": bad row stride");
  return PLSVO_OK;
}

// raw frames (device) -> level 0 of slots [first_slot, first_slot + n), then levels 1.. and the tiled mirror
static int rectify_levels(plsvo_ctx* c, int map_id, int first_slot, int n, const uint8_t* d_raw, int stride_bytes, size_t image_pitch_bytes,
                          int rounding) {
  const plsvo_ctx::RectifyMap& r = c->rect[map_id];
  uint8_t* base = c->pyr_slab.as<uint8_t>() + (size_t)first_slot * c->pyr.slot_bytes;
  if (r.identity && !r.flip) {   // vikit's identity branch: the existing level-0 copy
    HIP_TRY(c, launch_copy_level0(d_raw, image_pitch_bytes, r.w, r.h, stride_bytes, base + c->pyr.off[0], c->pyr.slot_bytes, n, c->stream));
  } else {
    HIP_TRY(c, launch_rectify(d_raw, image_pitch_bytes, stride_bytes, r.flip ? 1 : 0, r.map.as<uint32_t>(), r.w, r.h, base + c->pyr.off[0],
                              c->pyr.slot_bytes, n, c->stream));
  }
  return build_levels(c, first_slot, n, rounding);
}

extern "C" int plsvo_hip_rectify_build_pyramid(plsvo_ctx* c, int map_id, int slot, const uint8_t* raw, int stride_bytes, int rounding) {
  CTX_CHECK(c);
  if (!raw) return fail(c, PLSVO_E_INVALID, "rectify_build_pyramid: bad arguments");
  int rc = rectify_check(c, map_id, slot, 1, stride_bytes, "rectify_build_pyramid"); if (rc) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  const int W = c->pyr.w[0], H = c->pyr.h[0];
  HIP_TRY(c, c->pyr_upload.ensure((size_t)W * H));
  HIP_TRY(c, hipMemcpy2DAsync(c->pyr_upload.p, (size_t)W, raw, (size_t)stride_bytes, (size_t)W, (size_t)H, hipMemcpyHostToDevice, c->stream));
  rc = rectify_levels(c, map_id, slot, 1, c->pyr_upload.as<uint8_t>(), W, (size_t)W * H, rounding); if (rc) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PLSVO_OK;
}

extern "C" int plsvo_hip_rectify_build_pyramids_dev(plsvo_ctx* c, int map_id, int first_slot, int n, const void* d_raw, int stride_bytes,
                                                    size_t image_pitch_bytes, int rounding) {
  CTX_CHECK(c);
  if (!d_raw) return fail(c, PLSVO_E_INVALID, "rectify_build_pyramids_dev: bad arguments");
  int rc = rectify_check(c, map_id, first_slot, n, stride_bytes, "rectify_build_pyramids_dev"); if (rc) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  return rectify_levels(c, map_id, first_slot, n, reinterpret_cast<const uint8_t*>(d_raw), stride_bytes, image_pitch_bytes, rounding);
}

// ---- FAST corners per grid cell ------------------------------------------------------------------
// feature_detection::FastDetector::detect (src/feature_detection.cpp:53-104); kernels and key format: detect_device.hpp
extern "C" int plsvo_detect_grid(int width, int height, int cell_size, int* cols, int* rows) {
  if (width < 1 || height < 1 || cell_size < 1 || !cols || !rows) return PLSVO_E_INVALID;
  *cols = (int)(((long long)width + cell_size - 1) / cell_size);    // ceil(static_cast<double>(img_width) / cell_size), feature_detection.h:110-111
  *rows = (int)(((long long)height + cell_size - 1) / cell_size);
  return PLSVO_OK;
}

extern "C" int plsvo_detect_cell(int cols, int cell_size, double px_x, double px_y) {
  if (cols < 1 || cell_size < 1 || !std::isfinite(px_x) || !std::isfinite(px_y) || px_x < 0.0 || px_y < 0.0) return PLSVO_E_INVALID;
  const double cx = px_x / cell_size, cy = px_y / cell_size;
  if (cx >= 2147483647.0 || cy * cols + cx >= 2147483647.0) return PLSVO_E_INVALID;
  return static_cast<int>(cy) * cols + static_cast<int>(cx);
}

// the levels [level_lo, level_hi] of the configured pyramid as one launch
static void detect_fill_levels(const plsvo_ctx* c, int level_lo, int level_hi, DetectLaunch* a) {
  a->n_lv = 0; a->tile_begin[0] = 0;
  for (int l = level_lo; l <= level_hi; ++l) {
    const int e = a->n_lv++;
    a->level[e] = l; a->w[e] = c->pyr.w[l]; a->h[e] = c->pyr.h[l]; a->off[e] = c->pyr.off[l];
    a->tile_begin[e + 1] = a->tile_begin[e] + detect_tiles(a->w[e], a->h[e], &a->tiles_x[e]);
  }
}

// checks shared by the detect entry points: nothing has been enqueued or written when one fails
static int detect_check(plsvo_ctx* c, int first_slot, int n, const plsvo_detect_params* p, const void* corners, const void* counts, const char* what,
                        int* cols, int* rows) {
  if (!c->pyr.base) return fail(c, PLSVO_E_STATE, std::string(what) + ": pyramids not configured");
  if (!p || !corners || !counts) return fail(c, PLSVO_E_INVALID, std::string(what) + ": NULL params, corners or counts");
  if (n <= 0 || first_slot < 0 || first_slot > c->pyr.n_slots - n) return fail(c, PLSVO_E_INVALID, std::string(what) + ": slot range out of bounds");
  if (p->n_levels < 1 || p->n_levels > c->pyr.n_levels) return fail(c, PLSVO_E_INVALID, std::string(what) + ": n_levels outside the configured pyramid");
  if (p->cell_size < 1) return fail(c, PLSVO_E_INVALID, std::string(what) + ": cell_size < 1");
  if (c->pyr.w[0] > 8191 || c->pyr.h[0] > 8191) return fail(c, PLSVO_E_INVALID, std::string(what) + ": image wider or higher than 8191 (13 bits per coordinate of a cell key)");
  if (c->pyr.w[p->n_levels - 1] < 7 || c->pyr.h[p->n_levels - 1] < 7) return fail(c, PLSVO_E_INVALID, std::string(what) + ": a level smaller than 7 x 7");
  if (p->fast_threshold < 1 || p->fast_threshold > 254) return fail(c, PLSVO_E_INVALID, std::string(what) + ": fast_threshold outside 1..254");
  const double t = p->detection_threshold;
  if (!std::isfinite(t) || t < 0.0 || (double)(float)t != t) return fail(c, PLSVO_E_INVALID, std::string(what) + ": detection_threshold negative, not finite or not a float");
  if (plsvo_detect_grid(c->pyr.w[0], c->pyr.h[0], p->cell_size, cols, rows) != PLSVO_OK || (long long)*cols * *rows * n > INT32_MAX)
    return fail(c, PLSVO_E_INVALID, std::string(what) + ": grid too large");
  return PLSVO_OK;
}

static int detect_enqueue(plsvo_ctx* c, int first_slot, int n, const plsvo_detect_params* p, int cells, int cols, const uint8_t* d_occ,
                          plsvo_corner* d_corners, int32_t* d_counts) {
  const size_t key_bytes = (size_t)n * cells * sizeof(unsigned long long);
  if (key_bytes > c->det_keys.cap) {   // a new buffer starts armed; every compaction leaves it armed
    HIP_TRY(c, c->det_keys.ensure(key_bytes));
    HIP_TRY(c, hipMemsetAsync(c->det_keys.p, 0, c->det_keys.cap, c->stream));
  }
  DetectLaunch a{};
  a.pyr = c->pyr_slab.as<uint8_t>() + (size_t)first_slot * c->pyr.slot_bytes;
  a.slot_bytes = c->pyr.slot_bytes;
  detect_fill_levels(c, 0, p->n_levels - 1, &a);
  a.fast_b = p->fast_threshold; a.thr = (float)p->detection_threshold;
  a.cell = p->cell_size; a.cols = cols; a.n_cells = cells;
  a.occupancy = d_occ; a.keys = c->det_keys.as<unsigned long long>();
  HIP_TRY(c, launch_detect_fast(a, n, c->stream));
  HIP_TRY(c, launch_detect_compact(a.keys, cells, d_corners, d_counts, n, c->stream));
  return PLSVO_OK;
}

extern "C" int plsvo_hip_detect_fast_dev(plsvo_ctx* c, int first_slot, int n, const plsvo_detect_params* params, const uint8_t* d_occupancy,
                                         plsvo_corner* d_corners, int32_t* d_counts) {
  CTX_CHECK(c);
  int cols = 0, rows = 0;
  int rc = detect_check(c, first_slot, n, params, d_corners, d_counts, "detect_fast_dev", &cols, &rows); if (rc) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  return detect_enqueue(c, first_slot, n, params, cols * rows, cols, d_occupancy, d_corners, d_counts);
}

extern "C" int plsvo_hip_detect_fast(plsvo_ctx* c, int first_slot, int n, const plsvo_detect_params* params, const uint8_t* occupancy,
                                     plsvo_corner* corners, int32_t* counts) {
  CTX_CHECK(c);
  int cols = 0, rows = 0;
  int rc = detect_check(c, first_slot, n, params, corners, counts, "detect_fast", &cols, &rows); if (rc) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  const int cells = cols * rows;
  const size_t total = (size_t)n * cells;
  HIP_TRY(c, c->det_corners.ensure(total * sizeof(plsvo_corner)));
  HIP_TRY(c, c->det_counts.ensure((size_t)n * sizeof(int32_t)));
  if (occupancy) {
    HIP_TRY(c, c->det_occ.ensure(total));
    HIP_TRY(c, hipMemcpyAsync(c->det_occ.p, occupancy, total, hipMemcpyHostToDevice, c->stream));
  }
  rc = detect_enqueue(c, first_slot, n, params, cells, cols, occupancy ? c->det_occ.as<uint8_t>() : nullptr, c->det_corners.as<plsvo_corner>(),
                      c->det_counts.as<int32_t>());
  if (rc) return rc;
  // the records come back through a host copy of the device buffer: only the valid ones of every slot reach the caller's array
  std::vector<int32_t> cnt((size_t)n);
  HIP_TRY(c, hipMemcpyAsync(cnt.data(), c->det_counts.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < n; ++i) {
    if (cnt[(size_t)i] < 0 || cnt[(size_t)i] > cells) return fail(c, PLSVO_E_HIP, "detect_fast: corrupt count");
    if (cnt[(size_t)i] > 0)
      HIP_TRY(c, hipMemcpyAsync(corners + (size_t)i * cells, c->det_corners.as<plsvo_corner>() + (size_t)i * cells, (size_t)cnt[(size_t)i] * sizeof(plsvo_corner),
                                hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  memcpy(counts, cnt.data(), (size_t)n * sizeof(int32_t));
  return PLSVO_OK;
}

extern "C" int plsvo_hip_detect_stages(plsvo_ctx* c, int slot, int level, int fast_threshold, uint8_t* score, uint8_t* survives) {
  CTX_CHECK(c);
  if (!c->pyr.base) return fail(c, PLSVO_E_STATE, "detect_stages: pyramids not configured");
  if (!score || !survives || slot < 0 || slot >= c->pyr.n_slots || level < 0 || level >= c->pyr.n_levels || fast_threshold < 1 || fast_threshold > 254 ||
      c->pyr.w[0] > 8191 || c->pyr.h[0] > 8191)
    return fail(c, PLSVO_E_INVALID, "detect_stages: bad arguments");
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t px = (size_t)c->pyr.w[level] * c->pyr.h[level];
  HIP_TRY(c, c->det_stage.ensure(2 * px));
  DetectLaunch a{};
  a.pyr = c->pyr_slab.as<uint8_t>() + (size_t)slot * c->pyr.slot_bytes;
  a.slot_bytes = c->pyr.slot_bytes;
  detect_fill_levels(c, level, level, &a);
  a.fast_b = fast_threshold; a.cell = 1; a.cols = 1; a.n_cells = 1;
  a.stage_score = c->det_stage.as<uint8_t>(); a.stage_survives = a.stage_score + px;
  HIP_TRY(c, launch_detect_stages(a, c->stream));
  HIP_TRY(c, hipMemcpyAsync(score, a.stage_score, px, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(survives, a.stage_survives, px, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PLSVO_OK;
}

// ---- alignment -----------------------------------------------------------------------------------
template <typename T>
static int upload(plsvo_ctx* c, DevBuf& buf, const std::vector<T>& v) {
  HIP_TRY(c, buf.ensure(std::max(v.size(), (size_t)1) * sizeof(T)));
  if (!v.empty()) HIP_TRY(c, hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
  return PLSVO_OK;
}

// Static patch-slot layout of one job at one level (align_kernels.hip header).  Points own slots [0, n_pts).  The kernel works through the
// slots in WAVE-ROUNDS of 64 (slots [64 r, 64 r + 64) go to the 64 lanes of one wave) and weights a line from the residual sums its samples
// left in LDS behind a wave-level fence, so all samples of a segment with N <= 64 must sit inside ONE round; longer segments make the
// level a two-pass level (workgroup barrier between the passes).  Every round costs the same whether its lanes hold patches or holes, so
// the segments are PACKED into the rounds: first-fit in decreasing N (ties in feature order), starting in the round the points leave
// partly empty.  (Rounds 1-5 placed the segments in feature order from the next multiple of 32 behind the points and kept them from
// straddling multiples of 32 -- a left-over of the lane-pair kernel: 6.0 / 6.7 / 8.75 rounds per pass at levels 3 / 2 / 1 of BASELINE
// configs[1] where the patches fill 5 / 6 / 8.)  Segments without a landmark on entry, or whose end points fail the 3-pixel border test of
// the level (src/sparse_img_align.cpp:299-301), get no slots (code -1).  Host-only arithmetic; no result depends on where a segment sits.
// seg_align: 64 = small batches, whose point and segment slots may go to two workgroups (the segments start at a multiple of 64);
//            otherwise the segments start right behind the points.
static int slot_layout(const plsvo_align_in* in, int level, int seg_align, int32_t* seg_code, int32_t* n_slots, int32_t* long_lines, long long* n_patches) {
  if (!in || level < 0 || level >= PLSVO_MAX_LEVELS || in->n_pts < 0 || in->n_seg < 0 || (in->n_seg > 0 && !seg_code)) return PLSVO_E_INVALID;
  const plsvo_align_in& a = *in;
  constexpr int kRound = 64;
  long long n_real = a.n_pts;
  int any_long = 0;
  const double scale = 1.0 / (double)(1 << level);
  const int cw = a.cam.width / (1 << level), ch = a.cam.height / (1 << level);
  std::vector<int> shorts, longs;     // segments with slots: N <= 64 / longer
  for (int s = 0; s < a.n_seg; ++s) {
    seg_code[s] = -1;
    const bool alive_on_entry = a.seg_alive_in ? (a.seg_alive_in[s] != 0) : true;
    const double sx = a.seg_spx[2 * s], sy = a.seg_spx[2 * s + 1], ex = a.seg_epx[2 * s], ey = a.seg_epx[2 * s + 1];
    const int isx = (int)(sx * scale), isy = (int)(sy * scale), iex = (int)(ex * scale), iey = (int)(ey * scale);
    const bool vis = isx >= 3 && isx < cw - 3 && isy >= 3 && isy < ch - 3 && iex >= 3 && iex < cw - 3 && iey >= 3 && iey < ch - 3;
    if (alive_on_entry && vis) {
      const int N = seg_num_samples(sx, sy, ex, ey, a.seg_len[s], level);
      if (N > 2047) return PLSVO_E_CAPACITY;
      seg_code[s] = N << 20;             // (the first slot is filled in below)
      (N <= kRound ? shorts : longs).push_back(s);
      n_real += N;
    }
  }
  const long long seg0 = (seg_align == 64 && a.n_seg > 0) ? (((long long)a.n_pts + 63) & ~63LL) : (long long)a.n_pts;   // first slot a segment may take
  long long used = a.n_pts;
  if (!shorts.empty() || !longs.empty()) {
    std::stable_sort(shorts.begin(), shorts.end(), [&](int x, int y) { return (seg_code[x] >> 20) > (seg_code[y] >> 20); });
    const long long r0 = seg0 / kRound;                                      // the round the first segment may share with the last points
    std::vector<int> fill(1, (int)(seg0 - r0 * kRound));                     // slots taken in round r0 + k
    for (int s : shorts) {
      const int N = seg_code[s] >> 20;
      size_t k = 0;
      while (k < fill.size() && fill[k] + N > kRound) ++k;
      if (k == fill.size()) fill.push_back(0);
      const long long first = (r0 + (long long)k) * kRound + fill[k];
      if (first + N > (1 << 20) - 8) return PLSVO_E_CAPACITY;
      seg_code[s] |= (int)first;
      fill[k] += N;
      used = std::max(used, first + N);
    }
    long long cur = shorts.empty() ? ((seg0 + kRound - 1) / kRound) * kRound : (r0 + (long long)fill.size()) * kRound;   // behind the packed rounds
    for (int s : longs) {                                                    // two-pass level: any contiguous run of slots will do
      const int N = seg_code[s] >> 20;
      if (cur + N > (1 << 20) - 8) return PLSVO_E_CAPACITY;
      seg_code[s] |= (int)cur;
      cur += N; used = cur;
      any_long = 1;
    }
  }
  if (n_slots) *n_slots = (int32_t)used;
  if (long_lines) *long_lines = any_long;
  if (n_patches) *n_patches = n_real;
  return PLSVO_OK;
}
extern "C" int plsvo_align_slot_layout(const plsvo_align_in* in, int level, int32_t* seg_code, int32_t* n_slots, int32_t* long_lines,
                                       long long* n_patches) {
  return slot_layout(in, level, 32, seg_code, n_slots, long_lines, n_patches);
}

// Up to three device ranges to the host with ONE wait: through the context's pinned download buffer when they fit (a per-frame caller's
// results: a few hundred bytes of state + the flags), straight into the caller's (pageable) buffers otherwise.  On return h[k] points at
// range k's bytes: inside the pinned buffer (valid until the next fetch) or inside `fallback`.
// (`fallback` is sized HERE whenever the pinned path is not taken -- too large, or no pinned memory to be had -- so the decision and the
//  storage can never disagree: ADVICE r05)
static int download_ranges(plsvo_ctx* c, int n_ranges, const void* const* src, const size_t* bytes, std::vector<uint8_t>& fallback, const uint8_t** h) {
  size_t total = 0, off[3] = { 0, 0, 0 };
  for (int k = 0; k < n_ranges; ++k) { off[k] = total; total += (bytes[k] + 63) & ~(size_t)63; }
  bool pinned = total <= ((size_t)4 << 20);
  if (pinned && c->dl_pinned_cap < total) {
    if (c->dl_pinned) (void)hipHostFree(c->dl_pinned);
    c->dl_pinned = nullptr; c->dl_pinned_cap = 0;
    const size_t want = std::max(total * 2, (size_t)64 << 10);
    if (hipHostMalloc(&c->dl_pinned, want, hipHostMallocDefault) == hipSuccess) c->dl_pinned_cap = want; else { c->dl_pinned = nullptr; pinned = false; }
  }
  if (!pinned) fallback.resize(std::max(total, (size_t)64));
  uint8_t* const base = pinned ? static_cast<uint8_t*>(c->dl_pinned) : fallback.data();
  for (int k = 0; k < n_ranges; ++k) {
    void* to = static_cast<void*>(base + off[k]);
    h[k] = static_cast<const uint8_t*>(to);
    if (bytes[k]) HIP_TRY(c, hipMemcpyAsync(to, src[k], bytes[k], hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PLSVO_OK;
}

static const size_t kPinnedMax = (size_t)8 << 20;   // blobs up to 8 MB (hundreds of frames) bounce through pinned memory
static int upload_blob(plsvo_ctx* c, DevBuf& buf, const Blob& blob) {
  const size_t bytes = std::max(blob.host.size(), (size_t)256);
  HIP_TRY(c, buf.ensure(bytes));
  if (blob.host.empty()) return PLSVO_OK;
  // Small blobs (a frame, a few hundred frames) bounce through one of two pinned buffers: the DMA of a stage call is awaited only when
  // ITS buffer comes up for reuse two stage calls later (an event recorded behind the copy), so a per-frame caller's stage -> run -> fetch
  // makes ONE synchronisation, the fetch's.  (Round 3 waited for the stream inside every stage call.)
  if (blob.host.size() <= kPinnedMax) {
    const int k = c->pinned_next;
    if (!c->pinned_done[k] && hipEventCreate(&c->pinned_done[k]) != hipSuccess) c->pinned_done[k] = nullptr;
    if (c->pinned_done[k]) {
      HIP_TRY(c, hipEventSynchronize(c->pinned_done[k]));        // the copy that last read this buffer has landed (no-op when never recorded)
      if (c->pinned_cap[k] < blob.host.size()) {
        if (c->pinned[k]) (void)hipHostFree(c->pinned[k]);
        c->pinned[k] = nullptr; c->pinned_cap[k] = 0;
        const size_t want = std::max(blob.host.size() * 2, (size_t)1 << 20);
        if (hipHostMalloc(&c->pinned[k], want, hipHostMallocDefault) == hipSuccess) c->pinned_cap[k] = want; else c->pinned[k] = nullptr;
      }
      if (c->pinned[k]) {
        memcpy(c->pinned[k], blob.host.data(), blob.host.size());
        HIP_TRY(c, hipMemcpyAsync(buf.p, c->pinned[k], blob.host.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipEventRecord(c->pinned_done[k], c->stream));
        c->pinned_next = k ^ 1;
        return PLSVO_OK;
      }
    }
  }
  // large blobs (or no pinned memory): straight from the caller's Blob, which must not be touched while the DMA is in flight -- wait here
  HIP_TRY(c, hipMemcpyAsync(buf.p, blob.host.data(), blob.host.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PLSVO_OK;
}

extern "C" int plsvo_align_stage(plsvo_ctx* c, int n, const plsvo_align_in* in) {
  CTX_CHECK(c);
  if (n <= 0 || !in) return fail(c, PLSVO_E_INVALID, "align_stage: bad arguments");
  if (!c->pyr.base) return fail(c, PLSVO_E_STATE, "align_stage: pyramids not configured");
  HIP_TRY(c, hipSetDevice(c->device));
  c->a_staged = false;
  c->ch_staged = false;   // a resident frame step is built on the staged alignment batch: staging another one invalidates it
  std::vector<AlignJobDev> jobs((size_t)n);
  std::vector<double> T0((size_t)n * 7), ptpx, ptxyz, spx, epx, len, sp, sq;
  std::vector<uint8_t> alive;
  int gmax = -1, gmin = 99;
  // small batches may run two workgroups per frame (points | segments: plsvo_align_run decides from the launch shape): their segments start
  // at a multiple of 64 slots
  const int cus_stage = c->cu_count > 0 ? c->cu_count : 256;
  const int seg_align = (2 * n <= cus_stage) ? 64 : 32;
  int caps[PLSVO_MAX_LEVELS] = { 0 };
  std::vector<long long> work((size_t)n, 0);   // patches summed over the levels, per job: the launch-order key
  std::vector<int> seg_slot[PLSVO_MAX_LEVELS];   // per level, one entry per segment of the batch
  size_t patch_total = 0;
  for (int j = 0; j < n; ++j) {
    const plsvo_align_in& a = in[j];
    if (a.n_pts < 0 || a.n_seg < 0 || a.max_level < a.min_level || a.min_level < 0 || a.max_level >= c->pyr.n_levels || a.n_iter < 0)
      return fail(c, PLSVO_E_INVALID, "align_stage: bad job parameters (levels must exist in the configured pyramid)");
    if (a.ref_slot < 0 || a.ref_slot >= c->pyr.n_slots || a.cur_slot < 0 || a.cur_slot >= c->pyr.n_slots)
      return fail(c, PLSVO_E_CAPACITY, "align_stage: pyramid slot out of range");
    if (a.cam.width != c->pyr.w[0] || a.cam.height != c->pyr.h[0])
      return fail(c, PLSVO_E_INVALID, "align_stage: camera size does not match the configured pyramid");
    if ((a.n_pts > 0 && (!a.pt_px || !a.pt_xyz_ref)) || (a.n_seg > 0 && (!a.seg_spx || !a.seg_epx || !a.seg_len || !a.seg_p_ref || !a.seg_q_ref)))
      return fail(c, PLSVO_E_INVALID, "align_stage: null feature array");
    AlignJobDev& J = jobs[(size_t)j];
    J.ref_slot = a.ref_slot; J.cur_slot = a.cur_slot;
    J.fx = a.cam.fx; J.fy = a.cam.fy; J.cx = a.cam.cx; J.cy = a.cam.cy; J.width = a.cam.width; J.height = a.cam.height;
    J.max_level = a.max_level; J.min_level = a.min_level; J.n_iter = a.n_iter; J.eps = a.eps;
    J.skip = (a.n_pts == 0 && a.n_seg == 0) ? 1 : 0;
    J.pt_off = (int)(ptpx.size() / 2); J.n_pts = a.n_pts; J.seg_off = (int)len.size(); J.n_seg = a.n_seg;
    for (int k = 0; k < 7; ++k) T0[(size_t)j * 7 + k] = a.T_cur_from_ref[k];
    ptpx.insert(ptpx.end(), a.pt_px, a.pt_px + 2 * (size_t)a.n_pts);
    ptxyz.insert(ptxyz.end(), a.pt_xyz_ref, a.pt_xyz_ref + 3 * (size_t)a.n_pts);
    spx.insert(spx.end(), a.seg_spx, a.seg_spx + 2 * (size_t)a.n_seg);
    epx.insert(epx.end(), a.seg_epx, a.seg_epx + 2 * (size_t)a.n_seg);
    len.insert(len.end(), a.seg_len, a.seg_len + (size_t)a.n_seg);
    sp.insert(sp.end(), a.seg_p_ref, a.seg_p_ref + 3 * (size_t)a.n_seg);
    sq.insert(sq.end(), a.seg_q_ref, a.seg_q_ref + 3 * (size_t)a.n_seg);
    for (int s = 0; s < a.n_seg; ++s) alive.push_back(a.seg_alive_in ? (a.seg_alive_in[s] ? 1 : 0) : 1);
    // static patch-slot layout, per level (slot_layout above): points own slots [0, n_pts), the segments are packed behind them into
    // the kernel's wave-rounds of 64 slots; segments without a landmark on entry, or whose end points fail the 3-pixel border test of
    // the level (src/sparse_img_align.cpp:299-301), get no slots.
    int ub_max = 0;
    long long ub_sum = 0;
    J.long_mask = 0; J.ldlt_flavour = c->ldlt_flavour;
    for (int l = 0; l < PLSVO_MAX_LEVELS; ++l) J.n_slots[l] = 0;
    std::vector<int> codes((size_t)std::max(a.n_seg, 1));
    for (int l = a.max_level; l >= a.min_level; --l) {
      int n_slots = 0, long_lines = 0; long long n_real = 0;
      const int lrc = slot_layout(&a, l, seg_align, codes.data(), &n_slots, &long_lines, &n_real);
      if (lrc == PLSVO_E_CAPACITY) return fail(c, PLSVO_E_CAPACITY, "align_stage: a segment with more than 2047 samples or more than 2^20 patch slots in one job");
      if (lrc != PLSVO_OK) return fail(c, lrc, "align_stage: slot layout failed");
      seg_slot[(size_t)l].insert(seg_slot[(size_t)l].end(), codes.begin(), codes.begin() + a.n_seg);
      if (long_lines) J.long_mask |= 1 << l;
      const int slots4 = (n_slots + 3) & ~3;
      J.n_slots[l] = n_slots;
      ub_sum += n_real;
      if (!J.skip) caps[l] = std::max(caps[l], slots4);
      ub_max = std::max(ub_max, slots4);
    }
    J.patch_off = (int)patch_total; J.patch_cap = ub_max;
    work[(size_t)j] = J.skip ? 0 : ub_sum;
    patch_total += (size_t)ub_max;
    if (patch_total > (size_t)0x7fffffff / 16) return fail(c, PLSVO_E_CAPACITY, "align_stage: batch too large (patch index overflow)");
    if (!J.skip) { gmax = std::max(gmax, a.max_level); gmin = std::min(gmin, a.min_level); }
    // levels this job does not run still need an entry per segment: the table is indexed [level][segment of the batch]
    for (int l = 0; l < PLSVO_MAX_LEVELS; ++l)
      if (l > a.max_level || l < a.min_level) seg_slot[(size_t)l].insert(seg_slot[(size_t)l].end(), (size_t)a.n_seg, -1);
  }
  // launch order: most patches (summed over the levels) first; stable, so equal jobs keep their batch order
  std::vector<int> order((size_t)n);
  for (int j = 0; j < n; ++j) order[(size_t)j] = j;
  if (!c->env_align_no_lpt) std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return work[(size_t)x] > work[(size_t)y]; });
  int rc;
  const int slot_level0 = (gmax >= gmin && gmax >= 0) ? gmin : 0;
  const size_t total_seg = len.size();
  std::vector<int> slot_table;
  for (int l = slot_level0; l <= std::max(gmax, slot_level0); ++l) slot_table.insert(slot_table.end(), seg_slot[(size_t)l].begin(), seg_slot[(size_t)l].end());
  if (slot_table.empty()) slot_table.push_back(-1);
  Blob blob;
  const size_t o_slot = blob.add(slot_table), o_order = blob.add(order), o_jobs = blob.add(jobs), o_T0 = blob.add(T0), o_ptpx = blob.add(ptpx),
               o_ptxyz = blob.add(ptxyz), o_spx = blob.add(spx), o_epx = blob.add(epx), o_len = blob.add(len), o_sp = blob.add(sp),
               o_sq = blob.add(sq), o_alive = blob.add(alive);
  if ((rc = upload_blob(c, c->a_d_blob, blob))) return rc;
  HIP_TRY(c, c->a_d_alive.ensure(std::max(alive.size(), (size_t)1)));
  HIP_TRY(c, c->a_d_state.ensure((size_t)n * sizeof(AlignStateDev)));
  HIP_TRY(c, c->a_d_poses.ensure((size_t)n * 7 * sizeof(double)));
  const size_t pt = std::max(patch_total, (size_t)4);
  HIP_TRY(c, c->a_d_pxyz.ensure(pt * 3 * sizeof(double)));
  HIP_TRY(c, c->a_d_puv.ensure(pt * 2 * sizeof(float)));
  HIP_TRY(c, c->a_d_cref.ensure(pt * 64));   // one 64-byte record per patch slot (latency shapes: 192 B of float rows, sized in plsvo_align_run)
  c->a_patch_total = pt;
  const size_t npt_total = ptpx.size() / 2 + 32;
  HIP_TRY(c, c->a_d_chi.ensure(2 * npt_total * 16 * sizeof(float)));   // two planes of the points' per-pixel chi2 terms
  if (c->a_trace_cap > 0) HIP_TRY(c, c->a_d_log.ensure((size_t)n * c->a_trace_cap * sizeof(plsvo_align_iterlog)));

  AlignBatchDev& b = c->a_b;
  uint8_t* const base = c->a_d_blob.as<uint8_t>();
  b.jobs = reinterpret_cast<const AlignJobDev*>(base + o_jobs); b.state = c->a_d_state.as<AlignStateDev>();
  b.T0 = reinterpret_cast<const double*>(base + o_T0);
  b.pt_px = reinterpret_cast<const double*>(base + o_ptpx); b.pt_xyz = reinterpret_cast<const double*>(base + o_ptxyz);
  b.seg_spx = reinterpret_cast<const double*>(base + o_spx); b.seg_epx = reinterpret_cast<const double*>(base + o_epx);
  b.seg_len = reinterpret_cast<const double*>(base + o_len);
  b.seg_p = reinterpret_cast<const double*>(base + o_sp); b.seg_q = reinterpret_cast<const double*>(base + o_sq);
  b.seg_alive_in = base + o_alive; b.seg_alive = c->a_d_alive.as<uint8_t>();
  b.patch_xyz = c->a_d_pxyz.as<double>(); b.patch_uvref = c->a_d_puv.as<float>();
  b.cache_ref = c->a_d_cref.as<float>();
  b.chi_terms = c->a_d_chi.as<float>(); b.chi_plane = (unsigned long long)npt_total * 16;
  b.seg_slot = reinterpret_cast<const int*>(base + o_slot); b.slot_level0 = slot_level0; b.slot_stride = (int)total_seg;
  b.poses = c->a_d_poses.as<double>();
  b.pyr = c->pyr;
  b.log = c->a_trace_cap > 0 ? c->a_d_log.as<plsvo_align_iterlog>() : nullptr;
  b.log_cap = c->a_trace_cap;
  b.n_jobs = n;
  b.pair = 0; b.xseq0 = 0; b.xbuf = nullptr; b.work_key = nullptr; b.tail_n = 0; b.reserved_tail = 0; b.tail_flag = nullptr; b.seg_alive_tail = nullptr;   // (plsvo_align_run decides)
  b.order = reinterpret_cast<const int*>(base + o_order);
  c->a_stage_order = b.order;
  c->a_jobs.swap(jobs);
  c->a_n = n; c->a_total_seg = (int)alive.size(); c->a_gmax = gmax; c->a_gmin = gmin;
  for (int l = 0; l < PLSVO_MAX_LEVELS; ++l) c->a_cap[l] = caps[l];
  c->a_scap = 4;
  for (int j = 0; j < n; ++j) c->a_scap = std::max(c->a_scap, in[j].n_seg);
  c->a_seg_align = seg_align;
  c->a_staged = true; c->a_run_seq = 0;
  return PLSVO_OK;
}

// Launch configuration of the fused alignment kernel (measured on MI355X).  A frame pair is one workgroup (two for the
// smallest batches, plsvo_align_run); how many threads it gets depends on how many frames there are to fill the chip with:
//   >= 64 frames per CU (throughput): 64 threads -- one wave per frame, eight frames per CU hide each other's serial solve / update tails;
//   > 4 / > 1 frames per CU:          128 / 256 threads;
//   at most one frame per CU (latency): 512 threads, the whole CU works on one frame (its points; a second CU on its segments).
// Environment overrides (experiments only, read once at plsvo_hip_create): PLSVO_ALIGN_THREADS, PLSVO_ALIGN_PER_LEVEL, PLSVO_ALIGN_LDS_PAD,
// PLSVO_ALIGN_NO_PAIR, PLSVO_ALIGN_NO_REORDER / PLSVO_POSEOPT_NO_REORDER (launch order of a re-run staged batch), PLSVO_ALIGN_REORDER_MIN /
// PLSVO_POSEOPT_REORDER_MIN (its threshold, tests).  A switch set to "0" is off.
// Threads per frame of a pose-optimiser launch over n frames with `feats` features in all (the crossover is measured below, in
// plsvo_poseopt_run): shared by plsvo_poseopt_run, plsvo_chain_run and plsvo_candidates_pose_optimize
static int pose_opt_threads(const plsvo_ctx* c, int n, long feats) {
  const int cus = c->cu_count > 0 ? c->cu_count : 256;
  const int threads = n <= 2 * cus ? 256 : (feats <= 580l * n ? 16 : 64);
  return c->env_poseopt_threads ? c->env_poseopt_threads : threads;
}

static void pick_align_config(const plsvo_ctx* c, int n_jobs, int cap, int scap, int max_pts, int* threads, size_t* lds, int* chi_lds_pts) {
  const int cus = c->cu_count > 0 ? c->cu_count : 256;
  int t = 64;                            // >= 64 frames per CU: one wave per frame, no workgroup barrier at all
  if (n_jobs <= cus) t = 512;
  else if (n_jobs <= 4 * cus) t = 256;
  else if (n_jobs < 64 * cus) t = 128;
  if (c->env_align_threads) t = c->env_align_threads;
  // chi2 terms: in LDS when a workgroup owns (most of) a CU -- a global store is acknowledged from the memory side (~1 us) and a
  // lone frame has no other wave to hide that behind -- in HBM planes when eight frames share the CU's LDS
  int pts = t >= 256 ? ((max_pts + 3) & ~3) : 0;
  if (pts > 0 && align_level_lds_bytes(t, cap, scap, pts) > c->lds_per_block) pts = 0;
  *chi_lds_pts = pts;
  *threads = t; *lds = align_level_lds_bytes(t, cap, scap, pts);
  *lds += (size_t)c->env_align_lds_pad;   // occupancy experiments: unused LDS bytes per workgroup
}

// roctx range around the host side of an ABI call (rocprofv3 --marker-trace shows it).  The marker library is looked up at run
// time, once: the product library neither links against the profiler SDK nor fails to load without it.
namespace {
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_LAZY | RTLD_GLOBAL);
    if (!h) h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_LAZY | RTLD_GLOBAL);
    if (!h) return;
    push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
    pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
    if (!push || !pop) { push = nullptr; pop = nullptr; }
  }
};
const Roctx& roctx() { static const Roctx r; return r; }
struct RoctxRange {
  explicit RoctxRange(const char* name) { if (roctx().push) roctx().push(name); }
  ~RoctxRange() { if (roctx().pop) roctx().pop(); }
};
}  // namespace

constexpr int kAlignTailRounds = 2;   // tail set of the split, in rounds of resident workgroups (measured: DESIGN.md 3.1)
extern "C" int plsvo_align_run(plsvo_ctx* c) {
  CTX_CHECK(c);
  RoctxRange range("sparse_img_align");
  if (!c->a_staged) return fail(c, PLSVO_E_STATE, "align_run: no staged batch");
  HIP_TRY(c, hipSetDevice(c->device));
  // one launch: the workgroup of a job resets its solver state, runs its levels and writes its pose
  // (jobs without features, src/sparse_img_align.cpp:58-62, only do the first and the last)
  int cap = 4;
  const bool have_levels = c->a_gmax >= c->a_gmin && c->a_gmax >= 0;
  if (have_levels) for (int l = c->a_gmin; l <= c->a_gmax; ++l) cap = std::max(cap, c->a_cap[l]);
  int threads; size_t lds;
  const int scap = (c->a_scap + 3) & ~3;
  int max_pts = 0, chi_lds_pts = 0;
  for (const AlignJobDev& J : c->a_jobs) max_pts = std::max(max_pts, J.n_pts);
  pick_align_config(c, c->a_n, cap, scap, max_pts, &threads, &lds, &chi_lds_pts);
  c->a_b.chi_lds_pts = chi_lds_pts;
  if (lds > c->lds_per_block) return fail(c, PLSVO_E_CAPACITY, "align_run: slot tables do not fit in LDS (too many features in one job)");
  if (threads <= 64 && c->tiled_stale_count > 0) {   // the one-wave-per-frame shape reads the tiled mirror: bring the uploaded slots' tiles up to date first
    std::vector<int> slots;
    slots.reserve(2 * c->a_jobs.size());
    for (const AlignJobDev& J : c->a_jobs) { slots.push_back(J.ref_slot); slots.push_back(J.cur_slot); }
    const int rc_t = retile_stale(c, slots); if (rc_t) return rc_t;
  }
  // TWO WORKGROUPS PER FRAME: a frame that has a CU to itself is bound by that CU's instruction issue (two 64-slot wave-rounds per SIMD per
  // pass at 380 slots); with at most cu_count / 2 frames a second CU takes the segment slots, the two exchange 32 partial sums per
  // iteration through L2 (~1 us) and both run the identical solver.  Needs the latency shape, the chi2 planes in LDS (no deferred
  // decisions) and the layout staged for it; the per-level debug launches keep one workgroup.
  const int cus_run = c->cu_count > 0 ? c->cu_count : 256;
  // (exchange tags are launch << 10 | exchange, at most two exchanges per Gauss-Newton iteration -- the totals and a near tie's float sums:
  //  a launch that could need more than 1023 of them keeps one workgroup per frame, so a tag never runs into the next launch's range)
  int max_iter = 0;
  for (const AlignJobDev& J : c->a_jobs) max_iter = std::max(max_iter, J.n_iter);
  const long long max_exchanges = have_levels ? (long long)(c->a_gmax - c->a_gmin + 1) * (long long)max_iter * 2 : 0;
  const bool pair = threads >= kQuadMinThreads && chi_lds_pts > 0 && c->a_seg_align == 64 && 2 * c->a_n <= cus_run && !c->env_align_no_pair &&
                    !c->env_align_per_level && have_levels && max_exchanges < 1024;
  c->a_b.pair = pair ? 1 : 0;
  if (pair) {
    const size_t xbytes = (size_t)c->a_n * 256 * sizeof(unsigned long long);
    if (c->a_d_xbuf.cap < xbytes) {
      HIP_TRY(c, c->a_d_xbuf.ensure(std::max(xbytes, (size_t)128 * 2048)));
      HIP_TRY(c, hipMemsetAsync(c->a_d_xbuf.p, 0, c->a_d_xbuf.cap, c->stream));   // tag 0 is never used
    }
    c->a_b.xbuf = c->a_d_xbuf.as<unsigned long long>();
    c->x_launch = (c->x_launch + 1u) & 0x3fffffu;
    if (c->x_launch == 0) {   // the 22-bit launch counter wrapped: old tags could repeat -- zero the granules again (stream-ordered behind the last launch)
      HIP_TRY(c, hipMemsetAsync(c->a_d_xbuf.p, 0, c->a_d_xbuf.cap, c->stream));
      c->x_launch = 1;
    }
    c->a_b.xseq0 = c->x_launch << 10;
  }
  if (threads >= kQuadMinThreads) {   // latency shapes keep the reference patches as float rows: 192 B per slot (small batches only: <= 4 frames per CU)
    HIP_TRY(c, c->a_d_cref.ensure(c->a_patch_total * 192));
    c->a_b.cache_ref = c->a_d_cref.as<float>();
  }
  const bool per_level = c->env_align_per_level;
  // (a one-shot call -- plsvo_sparse_align_batch -- never re-runs its batch: no key, no sort)
  const bool reorder = have_levels && !per_level && c->a_n > (c->env_align_reorder_min > 0 ? c->env_align_reorder_min - 1 : cus_run * 512 / threads) &&   // more frames than resident workgroups (eight waves per CU)
                       !c->env_align_no_reorder && !c->env_align_no_lpt && !c->a_one_shot;
  c->a_b.work_key = nullptr;
  if (reorder) {
    if (c->a_d_workkey.cap < (size_t)c->a_n * sizeof(int)) {   // a fresh key buffer starts at zero work: jobs that leave the kernel early never write theirs
      HIP_TRY(c, c->a_d_workkey.ensure((size_t)c->a_n * sizeof(int)));
      HIP_TRY(c, hipMemsetAsync(c->a_d_workkey.p, 0, c->a_d_workkey.cap, c->stream));
    }
    c->a_b.work_key = c->a_d_workkey.as<int>();
  }
  // TAIL SPLIT: a launch of many rounds of resident workgroups ends on whichever long frames started last (~5 % of it: nothing known
  // before a frame runs predicts its cost).  The frames at the end of the launch order -- two rounds' worth -- therefore run as two
  // workgroups of the same launch, their coarse levels first and their finest level last (align_kernels.hip), so that the launch ends on
  // single levels.  Scheduling only: every result is bit-identical.  One wave per frame, at least two levels, at least four rounds; a
  // traced batch (plsvo_align_set_trace: its records count up in the frame's state iteration by iteration) keeps one workgroup per frame.
  c->a_b.tail_n = 0; c->a_b.tail_flag = nullptr; c->a_b.seg_alive_tail = nullptr;
  if (c->opt_align_tail_split && threads == 64 && have_levels && c->a_gmax > c->a_gmin && !pair && !per_level && c->a_trace_cap == 0) {
    const int resident = cus_run * 512 / threads;
    const int min_n = c->env_align_tail_min > 0 ? c->env_align_tail_min : 4 * resident;
    const int want = c->env_align_tail_frames > 0 ? c->env_align_tail_frames : (c->env_align_tail_k > 0 ? c->env_align_tail_k : kAlignTailRounds) * resident;
    if (c->a_n >= min_n) {
      const int tail_n = std::min(c->a_n, want);
      // flags are re-armed by a memset ahead of every launch (a 16-byte multiple from the allocation's start): no tag to keep in step
      // with the launch count, and a launch that was cut short leaves nothing behind
      const size_t fbytes = (((size_t)tail_n * sizeof(unsigned int)) + 15) & ~(size_t)15;
      HIP_TRY(c, c->a_d_tailflag.ensure(fbytes));
      HIP_TRY(c, hipMemsetAsync(c->a_d_tailflag.p, 0, fbytes, c->stream));
      HIP_TRY(c, c->a_d_alive_tail.ensure((size_t)std::max(c->a_total_seg, 1)));
      c->a_b.tail_n = tail_n; c->a_b.tail_flag = c->a_d_tailflag.as<unsigned int>(); c->a_b.seg_alive_tail = c->a_d_alive_tail.as<uint8_t>();
    }
  }
  if (!per_level || !have_levels) {
    EventPair ep{}; prof_begin(c, PLSVO_K_ALIGN_LEVEL, &ep);
    HIP_TRY(c, launch_align_levels(c->a_b, cap, scap, have_levels ? c->a_gmax : 0, have_levels ? c->a_gmin : 0, 1, threads, lds, c->stream));
    prof_end(c, PLSVO_K_ALIGN_LEVEL, &ep);
    // a batch with more frames than resident slots: the NEXT launch of this staged batch starts its frames longest-first by what they cost in
    // this one (one small kernel behind the launch; the order buffers alternate, the running launch's is never written)
    if (reorder) {
      DevBuf& ob = c->a_d_order[c->a_order_next];
      HIP_TRY(c, ob.ensure((size_t)c->a_n * sizeof(int)));
      HIP_TRY(c, launch_align_reorder(c->a_b.work_key, c->a_n, ob.as<int>(), 7, c->stream));
      c->a_b.order = ob.as<int>();
      c->a_order_next ^= 1;
    }
  } else {
    for (int level = c->a_gmax; level >= c->a_gmin; --level) {   // debug: one launch per level, state carried in HBM
      EventPair ep{}; prof_begin(c, PLSVO_K_ALIGN_LEVEL, &ep);
      HIP_TRY(c, launch_align_levels(c->a_b, cap, scap, level, level, level == c->a_gmax ? 1 : 0, threads, lds, c->stream));
      prof_end(c, PLSVO_K_ALIGN_LEVEL, &ep);
    }
  }
  c->a_run_seq = ++c->run_seq;
  return PLSVO_OK;
}

extern "C" int plsvo_align_fetch(plsvo_ctx* c, int n, plsvo_align_out* out) {
  CTX_CHECK(c);
  if (!c->a_staged) return fail(c, PLSVO_E_STATE, "align_fetch: no staged batch");
  if (n != c->a_n || !out) return fail(c, PLSVO_E_INVALID, "align_fetch: n does not match the staged batch");
  HIP_TRY(c, hipSetDevice(c->device));
  std::vector<uint8_t> big;   // (large batches, or no pinned memory: download_ranges sizes it)
  const size_t rb[2] = { (size_t)n * sizeof(AlignStateDev), (size_t)std::max(c->a_total_seg, 0) };
  const void* const rs[2] = { c->a_d_state.p, c->a_d_alive.p };
  const uint8_t* rh[2] = { nullptr, nullptr };
  { const int rc_d = download_ranges(c, 2, rs, rb, big, rh); if (rc_d) return rc_d; }
  const AlignStateDev* const st = reinterpret_cast<const AlignStateDev*>(rh[0]);
  const uint8_t* const alive = rh[1];
  int dev_err = 0;
  for (int j = 0; j < n; ++j) {
    const AlignStateDev& s = st[(size_t)j];
    plsvo_align_out& o = out[j];
    uint8_t* alive_out = o.seg_alive_out;
    memset(&o, 0, sizeof(o));
    o.seg_alive_out = alive_out;
    for (int k = 0; k < 7; ++k) o.T_cur_from_ref[k] = s.T[k];
    o.n_meas = s.n_meas; o.n_tracked = s.n_meas / PLSVO_PATCH_AREA;
    for (int k = 0; k < 36; ++k) o.H[k] = s.H[k];
    o.chi2 = s.chi2;
    for (int l = 0; l < PLSVO_MAX_LEVELS; ++l) o.iters_per_level[l] = s.iters[l];
    o.status = s.stop ? 1 : 0;
    if (alive_out && c->a_jobs[(size_t)j].n_seg > 0)
      memcpy(alive_out, alive + c->a_jobs[(size_t)j].seg_off, (size_t)c->a_jobs[(size_t)j].n_seg);
    if (s.error) dev_err = s.error;
  }
  // 1: a job's slot layout does not fit the launch; 2: a workgroup waited in vain for another one's data (the partner of a two-workgroup
  // frame, or the coarse part of a split frame) -- nothing a capacity would have prevented
  if (dev_err == 2) return fail(c, PLSVO_E_HIP, "align: a workgroup timed out waiting for the workgroup it shares a frame with (device-side hand-off, code 2)");
  if (dev_err) return fail(c, PLSVO_E_CAPACITY, "align: device-side capacity check failed (code " + std::to_string(dev_err) + ")");
  return PLSVO_OK;
}

extern "C" int plsvo_sparse_align_batch(plsvo_ctx* c, int n, const plsvo_align_in* in, plsvo_align_out* out) {
  const bool host_timing = c && c->env_host_timing;   // debug: wall time of the three steps on stderr
  const auto t0 = std::chrono::steady_clock::now();
  int rc = plsvo_align_stage(c, n, in); if (rc) return rc;
  const auto t1 = std::chrono::steady_clock::now();
  c->a_one_shot = true;
  rc = plsvo_align_run(c);
  c->a_one_shot = false;
  if (rc) return rc;
  const auto t2 = std::chrono::steady_clock::now();
  rc = plsvo_align_fetch(c, n, out);
  if (host_timing) {
    const auto t3 = std::chrono::steady_clock::now();
    fprintf(stderr, "[plsvo_hip] sparse_align_batch n=%d: stage %.1f us, run (enqueue) %.1f us, fetch (incl. wait) %.1f us\n", n,
            std::chrono::duration<double, std::micro>(t1 - t0).count(), std::chrono::duration<double, std::micro>(t2 - t1).count(),
            std::chrono::duration<double, std::micro>(t3 - t2).count());
  }
  return rc;
}
extern "C" int plsvo_sparse_align(plsvo_ctx* c, const plsvo_align_in* in, plsvo_align_out* out) {
  return plsvo_sparse_align_batch(c, 1, in, out);
}

extern "C" int plsvo_align_set_trace(plsvo_ctx* c, int max_records_per_job) {
  CTX_CHECK(c);
  if (max_records_per_job < 0) return fail(c, PLSVO_E_INVALID, "set_trace: negative capacity");
  c->a_trace_cap = max_records_per_job;
  c->a_staged = false;  // the trace buffer is sized at stage time
  return PLSVO_OK;
}

extern "C" int plsvo_align_fetch_trace(plsvo_ctx* c, int job, plsvo_align_iterlog* out, int max_records, int* n_records) {
  CTX_CHECK(c);
  if (!c->a_staged || c->a_trace_cap <= 0) return fail(c, PLSVO_E_STATE, "fetch_trace: tracing not enabled for the staged batch");
  if (job < 0 || job >= c->a_n || !out || !n_records) return fail(c, PLSVO_E_INVALID, "fetch_trace: bad arguments");
  HIP_TRY(c, hipSetDevice(c->device));
  AlignStateDev s;
  HIP_TRY(c, hipMemcpyAsync(&s, c->a_d_state.as<AlignStateDev>() + job, sizeof(s), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const int have = std::min(s.log_count, c->a_trace_cap);
  const int nrec = std::min(have, max_records);
  if (nrec > 0) {
    HIP_TRY(c, hipMemcpyAsync(out, c->a_d_log.as<plsvo_align_iterlog>() + (size_t)job * c->a_trace_cap, (size_t)nrec * sizeof(plsvo_align_iterlog),
                              hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  *n_records = nrec;
  return PLSVO_OK;
}

extern "C" const double* plsvo_align_poses_dev(plsvo_ctx* c) { return (c && c->a_staged) ? c->a_d_poses.as<double>() : nullptr; }

// debug: per-phase s_memtime ticks summed over the batch (all zero unless built with -DPLSVO_TIMING); not in the public header
extern "C" int plsvo_align_phase_ticks(plsvo_ctx* c, unsigned long long* out8) {
  CTX_CHECK(c);
  if (!c->a_staged || !out8) return fail(c, PLSVO_E_STATE, "phase_ticks: no staged batch");
  std::vector<AlignStateDev> st((size_t)c->a_n);
  HIP_TRY(c, hipMemcpyAsync(st.data(), c->a_d_state.p, (size_t)c->a_n * sizeof(AlignStateDev), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < 8; ++k) { out8[k] = 0; for (auto& s : st) out8[k] += s.phase_ticks[k]; }
  return PLSVO_OK;
}

extern "C" int plsvo_poseopt_phase_ticks(plsvo_ctx* c, unsigned long long* out8) {
  CTX_CHECK(c);
  if (!c->p_staged || !out8) return fail(c, PLSVO_E_STATE, "phase_ticks: no staged batch");
  std::vector<PoseStateDev> st((size_t)c->p_n);
  HIP_TRY(c, hipMemcpyAsync(st.data(), c->p_d_state.p, (size_t)c->p_n * sizeof(PoseStateDev), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < 8; ++k) { out8[k] = 0; for (auto& s : st) out8[k] += s.phase_ticks[k]; }
  return PLSVO_OK;
}

extern "C" int plsvo_align_copy_poses(plsvo_ctx* c, double* d_dst) {
  CTX_CHECK(c);
  if (!c->a_staged || !d_dst) return fail(c, PLSVO_E_STATE, "align_copy_poses: no staged batch / null destination");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(d_dst, c->a_d_poses.p, (size_t)c->a_n * 7 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  return PLSVO_OK;
}

extern "C" int plsvo_align_work(plsvo_ctx* c, uint64_t* patch_levels, uint64_t* patch_iters) {
  CTX_CHECK(c);
  if (!c->a_staged) return fail(c, PLSVO_E_STATE, "align_work: no staged batch");
  HIP_TRY(c, hipSetDevice(c->device));
  std::vector<AlignStateDev> st((size_t)c->a_n);
  HIP_TRY(c, hipMemcpyAsync(st.data(), c->a_d_state.p, (size_t)c->a_n * sizeof(AlignStateDev), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  uint64_t pl = 0, pi = 0;
  for (auto& s : st) { pl += s.patch_levels; pi += s.patch_iters; }
  if (patch_levels) *patch_levels = pl;
  if (patch_iters) *patch_iters = pi;
  return PLSVO_OK;
}

extern "C" int plsvo_align_work_points(plsvo_ctx* c, uint64_t* point_patch_iters) {
  CTX_CHECK(c);
  if (!c->a_staged) return fail(c, PLSVO_E_STATE, "align_work_points: no staged batch");
  HIP_TRY(c, hipSetDevice(c->device));
  std::vector<AlignStateDev> st((size_t)c->a_n);
  HIP_TRY(c, hipMemcpyAsync(st.data(), c->a_d_state.p, (size_t)c->a_n * sizeof(AlignStateDev), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  uint64_t n = 0;
  for (auto& s : st) n += s.patch_iters_pt;
  if (point_patch_iters) *point_patch_iters = n;
  return PLSVO_OK;
}

extern "C" int plsvo_align_launch_order(plsvo_ctx* c, int n, int32_t* order) {
  CTX_CHECK(c);
  if (!c->a_staged) return fail(c, PLSVO_E_STATE, "align_launch_order: no staged batch");
  if (n != c->a_n || !order) return fail(c, PLSVO_E_INVALID, "align_launch_order: n does not match the staged batch");
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->a_b.order) { for (int j = 0; j < n; ++j) order[j] = j; return PLSVO_OK; }
  HIP_TRY(c, hipMemcpyAsync(order, c->a_b.order, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PLSVO_OK;
}

extern "C" int plsvo_align_tail_frames(plsvo_ctx* c, int* tail_frames) {
  CTX_CHECK(c);
  if (!c->a_staged) return fail(c, PLSVO_E_STATE, "align_tail_frames: no staged batch");
  if (!tail_frames) return fail(c, PLSVO_E_INVALID, "align_tail_frames: NULL output");
  *tail_frames = c->a_b.tail_n;
  return PLSVO_OK;
}

extern "C" int plsvo_align_chi2_ties(plsvo_ctx* c, uint64_t* iterations, uint64_t* ties, uint64_t* near_ties_without_terms) {
  CTX_CHECK(c);
  if (!c->a_staged) return fail(c, PLSVO_E_STATE, "align_chi2_ties: no staged batch");
  HIP_TRY(c, hipSetDevice(c->device));
  std::vector<AlignStateDev> st((size_t)c->a_n);
  HIP_TRY(c, hipMemcpyAsync(st.data(), c->a_d_state.p, (size_t)c->a_n * sizeof(AlignStateDev), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  uint64_t it = 0, t = 0, un = 0;
  for (auto& s : st) { t += (uint64_t)s.chi2_ties; un += (uint64_t)s.chi2_unarmed; for (int l = 0; l < PLSVO_MAX_LEVELS; ++l) it += (uint64_t)s.iters[l]; }
  if (iterations) *iterations = it;
  if (ties) *ties = t;
  if (near_ties_without_terms) *near_ties_without_terms = un;
  return PLSVO_OK;
}

// ---- pose optimisation ---------------------------------------------------------------------------
extern "C" int plsvo_poseopt_stage(plsvo_ctx* c, int n, const plsvo_poseopt_in* in) {
  CTX_CHECK(c);
  if (n <= 0 || !in) return fail(c, PLSVO_E_INVALID, "poseopt_stage: bad arguments");
  HIP_TRY(c, hipSetDevice(c->device));
  c->p_staged = false;
  std::vector<PoseJobDev> jobs((size_t)n);
  std::vector<double> f, pos, line, spos, epos;
  std::vector<int> plev, slev;
  for (int j = 0; j < n; ++j) {
    const plsvo_poseopt_in& a = in[j];
    if (a.n_pts < 0 || a.n_seg < 0 || a.n_iter < 0) return fail(c, PLSVO_E_INVALID, "poseopt_stage: bad job parameters");
    if ((a.n_pts > 0 && (!a.pt_f || !a.pt_pos || !a.pt_level)) || (a.n_seg > 0 && (!a.seg_line || !a.seg_spos || !a.seg_epos || !a.seg_level)))
      return fail(c, PLSVO_E_INVALID, "poseopt_stage: null feature array");
    PoseJobDev& J = jobs[(size_t)j];
    for (int k = 0; k < 7; ++k) J.T0[k] = a.T_f_w[k];
    J.fx = a.fx; J.reproj_thresh = a.reproj_thresh; J.n_iter = a.n_iter; J.n_iter_ref = a.n_iter_ref; J.ldlt_flavour = c->ldlt_flavour; J.reserved0 = 0;
    J.pt_off = (int)plev.size(); J.n_pts = a.n_pts; J.seg_off = (int)slev.size(); J.n_seg = a.n_seg;
    f.insert(f.end(), a.pt_f, a.pt_f + 3 * (size_t)a.n_pts);
    pos.insert(pos.end(), a.pt_pos, a.pt_pos + 3 * (size_t)a.n_pts);
    plev.insert(plev.end(), a.pt_level, a.pt_level + (size_t)a.n_pts);
    line.insert(line.end(), a.seg_line, a.seg_line + 3 * (size_t)a.n_seg);
    spos.insert(spos.end(), a.seg_spos, a.seg_spos + 3 * (size_t)a.n_seg);
    epos.insert(epos.end(), a.seg_epos, a.seg_epos + 3 * (size_t)a.n_seg);
    slev.insert(slev.end(), a.seg_level, a.seg_level + (size_t)a.n_seg);
    for (int i = 0; i < a.n_pts; ++i) if (a.pt_level[i] < 0 || a.pt_level[i] > 30) return fail(c, PLSVO_E_INVALID, "poseopt_stage: feature level out of range");
    for (int i = 0; i < a.n_seg; ++i) if (a.seg_level[i] < 0 || a.seg_level[i] > 30) return fail(c, PLSVO_E_INVALID, "poseopt_stage: feature level out of range");
  }
  int rc;
  Blob blob;
  const size_t o_jobs = blob.add(jobs), o_f = blob.add(f), o_pos = blob.add(pos), o_plev = blob.add(plev), o_line = blob.add(line),
               o_spos = blob.add(spos), o_epos = blob.add(epos), o_slev = blob.add(slev);
  if ((rc = upload_blob(c, c->p_d_blob, blob))) return rc;
  const size_t npt = plev.size(), nsg = slev.size(), nft = std::max(npt + nsg, (size_t)1);
  HIP_TRY(c, c->p_d_ptkeep.ensure(std::max(npt, (size_t)1)));
  HIP_TRY(c, c->p_d_segkeep.ensure(std::max(nsg, (size_t)1)));
  HIP_TRY(c, c->p_d_s32.ensure(nft * sizeof(float)));
  HIP_TRY(c, c->p_d_s64.ensure(nft * 5 * sizeof(double)));
  HIP_TRY(c, c->p_d_state.ensure((size_t)n * sizeof(PoseStateDev)));
  HIP_TRY(c, c->p_d_poses.ensure((size_t)n * 7 * sizeof(double)));
  if (c->p_trace_cap > 0) HIP_TRY(c, c->p_d_log.ensure((size_t)n * c->p_trace_cap * sizeof(plsvo_poseopt_iterlog)));
  PoseBatchDev& b = c->p_b;
  uint8_t* const base = c->p_d_blob.as<uint8_t>();
  b.jobs = reinterpret_cast<const PoseJobDev*>(base + o_jobs); b.state = c->p_d_state.as<PoseStateDev>();
  b.pt_f = reinterpret_cast<const double*>(base + o_f); b.pt_pos = reinterpret_cast<const double*>(base + o_pos);
  b.pt_level = reinterpret_cast<const int*>(base + o_plev);
  b.seg_line = reinterpret_cast<const double*>(base + o_line); b.seg_spos = reinterpret_cast<const double*>(base + o_spos);
  b.seg_epos = reinterpret_cast<const double*>(base + o_epos); b.seg_level = reinterpret_cast<const int*>(base + o_slev);
  b.pt_keep = c->p_d_ptkeep.as<uint8_t>(); b.seg_keep = c->p_d_segkeep.as<uint8_t>();
  b.scratch_f32 = c->p_d_s32.as<float>(); b.scratch_f64 = c->p_d_s64.as<double>();
  b.log = c->p_trace_cap > 0 ? c->p_d_log.as<plsvo_poseopt_iterlog>() : nullptr;
  b.log_cap = c->p_trace_cap; b.n_jobs = n;
  b.order = nullptr; b.work_key = nullptr;   // a new batch: no measured work yet (plsvo_poseopt_run)
  {   // sort-key resolution: the most feature-iterations a frame of this batch can evaluate, in 1024 bins
    long key_max = 1;
    for (int j = 0; j < n; ++j) key_max = std::max(key_max, (long)(jobs[j].n_pts + jobs[j].n_seg) * (long)(std::max(jobs[j].n_iter, 0) + std::max(jobs[j].n_iter_ref, 0)));
    c->p_key_shift = 0;
    while ((key_max >> c->p_key_shift) > 1023) ++c->p_key_shift;
  }
  c->p_any_ref = false;
  for (int j = 0; j < n; ++j) c->p_any_ref = c->p_any_ref || jobs[j].n_iter_ref > 0;
  c->p_jobs.swap(jobs);
  c->p_n = n; c->p_total_pt = (int)npt; c->p_total_seg = (int)nsg;
  c->p_staged = true; c->p_run_seq = 0;
  return PLSVO_OK;
}

extern "C" int plsvo_poseopt_run(plsvo_ctx* c) {
  CTX_CHECK(c);
  RoctxRange range("pose_optimizer");
  if (!c->p_staged) return fail(c, PLSVO_E_STATE, "poseopt_run: no staged batch");
  HIP_TRY(c, hipSetDevice(c->device));
  // Large batches: a 16-lane row per frame, four frames per wave (the serial solve + update of four frames share one instruction stream:
  // poseopt_kernels.hip) while a frame has a few hundred features -- measured on MI355X, 32768 frames: 200 + 80 features 1.86 ms against
  // 2.03 ms for a wave per frame, 500 + 200 features 4.55 against 3.77 (a row then needs 44 dependent feature rounds per pass).  The
  // crossover, measured in round 5 (tools/poseopt_crossover.py, 16384 frames): 420 features 1.31 vs 1.47 ms, 550 features 1.72 vs 1.79,
  // 620 features 1.91 vs 1.80, 700 features 2.19 vs 1.95 -- frames above 580 features keep the wave-per-frame shape.  Too few frames to fill the chip: four waves per frame (the Gauss-Newton loop of
  // one frame is then ~2x shorter).  PLSVO_POSEOPT_THREADS / PLSVO_OPT_POSEOPT_THREADS override (tests and measurements).
  const int cus = c->cu_count > 0 ? c->cu_count : 256;
  const long feats = (long)c->p_total_pt + (long)c->p_total_seg;
  const int threads = pose_opt_threads(c, c->p_n, feats);
  // batches larger than the resident waves: this launch records what every frame cost, the next one takes them most-expensive first (see
  // plsvo_align_run; for the rows kernel the sort also puts frames that stop together into the same wave)
  const bool reorder = threads != 256 && !c->env_poseopt_no_reorder && !c->p_one_shot &&
                       c->p_n > (c->env_poseopt_reorder_min > 0 ? c->env_poseopt_reorder_min - 1 : (threads == 16 ? 4 : 8) * cus);   // (rows: the grouping pays before the launch has a tail)
  c->p_b.work_key = nullptr;
  if (reorder) {
    if (c->p_d_workkey.cap < (size_t)c->p_n * sizeof(int)) {
      HIP_TRY(c, c->p_d_workkey.ensure((size_t)c->p_n * sizeof(int)));
      HIP_TRY(c, hipMemsetAsync(c->p_d_workkey.p, 0, c->p_d_workkey.cap, c->stream));
    }
    c->p_b.work_key = c->p_d_workkey.as<int>();
  } else c->p_b.order = nullptr;
  // ROW REFILL: the four frames of a row-shape wave iterate until the last of them stops, and iteration counts are bimodal -- in the
  // stage order almost every wave runs all ten.  With more than two frames per resident row the launch is cut at the Gauss-Newton
  // loop's borders and the rows of a persistent kernel take their next frame from a queue (poseopt_kernels.hip).  Scheduling only: every
  // result is bit-identical.  At two frames per row the launch still ends on a ten-iteration frame that started second.  The crossover,
  // measured on MI355X (8192 resident rows, 200 + 80 features, one launch -> three; profiles/poseopt_refill_ab.md): 16384 frames 0.890 ->
  // 0.887 ms, 24576 frames 1.325 -> 1.271, 32768 frames 1.751 -> 1.575, 65536 frames 3.385 -> 2.914; 550 features x 16384 frames 1.684 -> 1.712.
  // A batch with a refinement loop or an iteration trace keeps pose_opt_rows_kernel.
  const int resident_wgs = cus * 512 / 64;
  const int refill_min = c->env_poseopt_refill_min > 0 ? c->env_poseopt_refill_min : 2 * 4 * resident_wgs + 1;
  const bool refill = c->opt_poseopt_refill && threads == 16 && !c->p_b.log && !c->p_any_ref && pose_opt_refill_built() && c->p_n >= refill_min;
  c->p_refill_frames = 0;
  EventPair ep{}; prof_begin(c, PLSVO_K_POSEOPT, &ep);
  if (refill) {
    const int wgs = (c->p_n + 3) / 4;
    const int gn_grid = std::max(1, std::min(wgs, c->env_poseopt_refill_waves > 0 ? c->env_poseopt_refill_waves : resident_wgs));
    HIP_TRY(c, c->p_d_carry.ensure((size_t)c->p_n * sizeof(PoseRefillCarry)));
    HIP_TRY(c, c->p_d_refill_next.ensure(16));
    HIP_TRY(c, hipMemsetAsync(c->p_d_refill_next.p, 0, 16, c->stream));   // the queue is re-armed ahead of every launch
    const PoseRefillDev q{ c->p_d_carry.as<PoseRefillCarry>(), c->p_d_refill_next.as<int>() };
    HIP_TRY(c, launch_pose_opt_refill(c->p_b, q, c->p_d_poses.as<double>(), gn_grid, c->opt_poseopt_select ? 1 : 0, c->stream));
    c->p_refill_frames = c->p_n;
  } else {
    HIP_TRY(c, launch_pose_opt(c->p_b, c->p_d_poses.as<double>(), threads, c->opt_poseopt_select ? 1 : 0, c->stream));
  }
  c->p_run_seq = ++c->run_seq;
  prof_end(c, PLSVO_K_POSEOPT, &ep);
  if (reorder) {
    DevBuf& ob = c->p_d_order[c->p_order_next];
    HIP_TRY(c, ob.ensure((size_t)c->p_n * sizeof(int)));
    HIP_TRY(c, launch_align_reorder(c->p_b.work_key, c->p_n, ob.as<int>(), c->p_key_shift, c->stream));
    c->p_b.order = ob.as<int>();
    c->p_order_next ^= 1;
  }
  return PLSVO_OK;
}

extern "C" int plsvo_poseopt_fetch(plsvo_ctx* c, int n, plsvo_poseopt_out* out) {
  CTX_CHECK(c);
  if (!c->p_staged) return fail(c, PLSVO_E_STATE, "poseopt_fetch: no staged batch");
  if (n != c->p_n || !out) return fail(c, PLSVO_E_INVALID, "poseopt_fetch: n does not match the staged batch");
  HIP_TRY(c, hipSetDevice(c->device));
  std::vector<uint8_t> big;   // (large batches, or no pinned memory: download_ranges sizes it)
  const size_t rb[3] = { (size_t)n * sizeof(PoseStateDev), (size_t)std::max(c->p_total_pt, 0), (size_t)std::max(c->p_total_seg, 0) };
  const void* const rs[3] = { c->p_d_state.p, c->p_d_ptkeep.p, c->p_d_segkeep.p };
  const uint8_t* rh[3] = { nullptr, nullptr, nullptr };
  { const int rc_d = download_ranges(c, 3, rs, rb, big, rh); if (rc_d) return rc_d; }
  const PoseStateDev* const st = reinterpret_cast<const PoseStateDev*>(rh[0]);
  const uint8_t* const pk = rh[1]; const uint8_t* const sk = rh[2];
  for (int j = 0; j < n; ++j) {
    const PoseStateDev& s = st[(size_t)j];
    const PoseJobDev& J = c->p_jobs[(size_t)j];
    plsvo_poseopt_out& o = out[j];
    uint8_t* pko = o.pt_keep; uint8_t* sko = o.seg_keep;
    memset(&o, 0, sizeof(o));
    o.pt_keep = pko; o.seg_keep = sko;
    for (int k = 0; k < 7; ++k) o.T_f_w[k] = s.T[k];
    for (int k = 0; k < 36; ++k) o.cov[k] = s.cov[k];
    o.estimated_scale = s.estimated_scale; o.error_init = s.error_init; o.error_final = s.error_final;
    o.num_obs_pt = s.num_obs_pt; o.num_obs_ls = s.num_obs_ls;
    o.iters = s.iters; o.iters_ref = s.iters_ref; o.status = s.status;
    if (pko && J.n_pts > 0) memcpy(pko, pk + J.pt_off, (size_t)J.n_pts);
    if (sko && J.n_seg > 0) memcpy(sko, sk + J.seg_off, (size_t)J.n_seg);
  }
  return PLSVO_OK;
}

extern "C" int plsvo_poseopt_refill_frames(plsvo_ctx* c, int* refill_frames) {
  CTX_CHECK(c);
  if (!refill_frames) return fail(c, PLSVO_E_INVALID, "poseopt_refill_frames: NULL output");
  *refill_frames = c->p_refill_frames;
  return PLSVO_OK;
}

// the row kernels' select on rows of patterns (tests): staged in one blob, one launch, read back
extern "C" int plsvo_poseopt_row_select(plsvo_ctx* c, const plsvo_row_select_in* in, void* selected, int32_t* path) {
  CTX_CHECK(c);
  if (!in || !selected || !path || in->n_rows < 0 || in->n_patterns < 0 || (in->bits != 32 && in->bits != 64))
    return fail(c, PLSVO_E_INVALID, "poseopt_row_select: bad arguments");
  const int nr = in->n_rows;
  if (nr == 0) return PLSVO_OK;
  if (!in->row_off || !in->row_n || !in->row_k || !in->row_active || (in->n_patterns > 0 && !in->patterns))
    return fail(c, PLSVO_E_INVALID, "poseopt_row_select: null input array");
  for (int r = 0; r < nr; ++r) {
    const long long o = in->row_off[r]; const int n = in->row_n[r];
    if (n < 0 || o < 0 || o + (long long)n > in->n_patterns) return fail(c, PLSVO_E_INVALID, "poseopt_row_select: a row lies outside the patterns");
    if (in->row_active[r] && n > 0 && (in->row_k[r] < 0 || in->row_k[r] >= n)) return fail(c, PLSVO_E_INVALID, "poseopt_row_select: k outside [0, n)");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t width = (size_t)in->bits / 8;
  auto up16 = [](size_t v) { return (v + 15) / 16 * 16; };
  const size_t o_off = up16((size_t)in->n_patterns * width), o_n = o_off + up16((size_t)nr * sizeof(long long)), o_k = o_n + up16((size_t)nr * sizeof(int));
  const size_t o_act = o_k + up16((size_t)nr * sizeof(int)), in_bytes = o_act + up16((size_t)nr);
  std::vector<uint8_t> h(in_bytes, 0);
  if (in->n_patterns > 0) memcpy(h.data(), in->patterns, (size_t)in->n_patterns * width);
  memcpy(h.data() + o_off, in->row_off, (size_t)nr * sizeof(long long));
  memcpy(h.data() + o_n, in->row_n, (size_t)nr * sizeof(int));
  memcpy(h.data() + o_k, in->row_k, (size_t)nr * sizeof(int));
  memcpy(h.data() + o_act, in->row_active, (size_t)nr);
  const size_t o_path = up16((size_t)nr * width), out_bytes = o_path + (size_t)nr * sizeof(int);
  HIP_TRY(c, c->s_d_in.ensure(in_bytes + 16));
  HIP_TRY(c, c->s_d_out.ensure(out_bytes + 16));
  char* din = reinterpret_cast<char*>(c->s_d_in.p); char* dout = reinterpret_cast<char*>(c->s_d_out.p);
  HIP_TRY(c, hipMemcpyAsync(din, h.data(), in_bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemsetAsync(dout, 0, out_bytes, c->stream));
  RowSelectDev t{};
  t.patterns = din; t.row_off = reinterpret_cast<const long long*>(din + o_off); t.row_n = reinterpret_cast<const int*>(din + o_n);
  t.row_k = reinterpret_cast<const int*>(din + o_k); t.row_active = reinterpret_cast<const uint8_t*>(din + o_act);
  t.selected = dout; t.path = reinterpret_cast<int*>(dout + o_path);
  t.n_rows = nr; t.bits = in->bits; t.select = c->opt_poseopt_select ? 1 : 0;
  HIP_TRY(c, launch_pose_row_select(t, c->stream));
  std::vector<uint8_t> ho(out_bytes);
  HIP_TRY(c, hipMemcpyAsync(ho.data(), dout, out_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  memcpy(selected, ho.data(), (size_t)nr * width);
  memcpy(path, ho.data() + o_path, (size_t)nr * sizeof(int));
  return PLSVO_OK;
}

extern "C" int plsvo_pose_optimize_batch(plsvo_ctx* c, int n, const plsvo_poseopt_in* in, plsvo_poseopt_out* out) {
  int rc = plsvo_poseopt_stage(c, n, in); if (rc) return rc;
  c->p_one_shot = true;
  rc = plsvo_poseopt_run(c);
  c->p_one_shot = false;
  if (rc) return rc;
  return plsvo_poseopt_fetch(c, n, out);
}
extern "C" int plsvo_pose_optimize(plsvo_ctx* c, const plsvo_poseopt_in* in, plsvo_poseopt_out* out) {
  return plsvo_pose_optimize_batch(c, 1, in, out);
}

extern "C" int plsvo_poseopt_set_trace(plsvo_ctx* c, int max_records_per_job) {
  CTX_CHECK(c);
  if (max_records_per_job < 0) return fail(c, PLSVO_E_INVALID, "set_trace: negative capacity");
  c->p_trace_cap = max_records_per_job;
  c->p_staged = false;
  return PLSVO_OK;
}

extern "C" int plsvo_poseopt_fetch_trace(plsvo_ctx* c, int job, plsvo_poseopt_iterlog* out, int max_records, int* n_records) {
  CTX_CHECK(c);
  if (!c->p_staged || c->p_trace_cap <= 0) return fail(c, PLSVO_E_STATE, "fetch_trace: tracing not enabled for the staged batch");
  if (job < 0 || job >= c->p_n || !out || !n_records) return fail(c, PLSVO_E_INVALID, "fetch_trace: bad arguments");
  HIP_TRY(c, hipSetDevice(c->device));
  PoseStateDev s;
  HIP_TRY(c, hipMemcpyAsync(&s, c->p_d_state.as<PoseStateDev>() + job, sizeof(s), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const int nrec = std::min(std::min(s.log_count, c->p_trace_cap), max_records);
  if (nrec > 0) {
    HIP_TRY(c, hipMemcpyAsync(out, c->p_d_log.as<plsvo_poseopt_iterlog>() + (size_t)job * c->p_trace_cap, (size_t)nrec * sizeof(plsvo_poseopt_iterlog),
                              hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  *n_records = nrec;
  return PLSVO_OK;
}

extern "C" const double* plsvo_poseopt_poses_dev(plsvo_ctx* c) { return (c && c->p_staged) ? c->p_d_poses.as<double>() : nullptr; }

extern "C" int plsvo_poseopt_copy_poses(plsvo_ctx* c, double* d_dst) {
  CTX_CHECK(c);
  if (!c->p_staged || !d_dst) return fail(c, PLSVO_E_STATE, "poseopt_copy_poses: no staged batch / null destination");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(d_dst, c->p_d_poses.p, (size_t)c->p_n * 7 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  return PLSVO_OK;
}

extern "C" int plsvo_poseopt_work(plsvo_ctx* c, uint64_t* pt_iters, uint64_t* seg_iters) {
  CTX_CHECK(c);
  if (!c->p_staged) return fail(c, PLSVO_E_STATE, "poseopt_work: no staged batch");
  HIP_TRY(c, hipSetDevice(c->device));
  std::vector<PoseStateDev> st((size_t)c->p_n);
  HIP_TRY(c, hipMemcpyAsync(st.data(), c->p_d_state.p, (size_t)c->p_n * sizeof(PoseStateDev), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  uint64_t a = 0, b2 = 0;
  for (auto& s : st) { a += s.pt_iters; b2 += s.seg_iters; }
  if (pt_iters) *pt_iters = a;
  if (seg_iters) *seg_iters = b2;
  return PLSVO_OK;
}

// ---- structure optimisation ------------------------------------------------------------------------
extern "C" int plsvo_structure_optimize(plsvo_ctx* c, const plsvo_structopt_in* in, plsvo_structopt_out* out) {
  CTX_CHECK(c);
  if (!in || !out || in->n_pts < 0 || in->n_seg < 0 || in->n_frames < 0 || in->n_iter_pts < 0 || in->n_iter_segs < 0)
    return fail(c, PLSVO_E_INVALID, "structure_optimize: bad arguments");
  if ((in->n_pts > 0 && (!in->pt_pos || !in->pt_obs_off)) || (in->n_seg > 0 && (!in->seg_spos || !in->seg_epos || !in->seg_obs_off)))
    return fail(c, PLSVO_E_INVALID, "structure_optimize: null landmark array");
  if (in->n_pts + in->n_seg == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const int np = in->n_pts, ns = in->n_seg;
  const int npo = np > 0 ? in->pt_obs_off[np] : 0, nso = ns > 0 ? in->seg_obs_off[ns] : 0;
  if (npo < 0 || nso < 0 || (npo > 0 && (!in->pt_obs_frame || !in->pt_obs_f)) || (nso > 0 && (!in->seg_obs_frame || !in->seg_obs_sf || !in->seg_obs_ef)) ||
      ((npo > 0 || nso > 0) && (!in->frame_T || in->n_frames <= 0)))
    return fail(c, PLSVO_E_INVALID, "structure_optimize: bad observation tables");
  for (int i = 0; i < npo; ++i) if (in->pt_obs_frame[i] < 0 || in->pt_obs_frame[i] >= in->n_frames) return fail(c, PLSVO_E_INVALID, "structure_optimize: frame index out of range");
  for (int i = 0; i < nso; ++i) if (in->seg_obs_frame[i] < 0 || in->seg_obs_frame[i] >= in->n_frames) return fail(c, PLSVO_E_INVALID, "structure_optimize: frame index out of range");
  // one packed upload: doubles first, then ints
  std::vector<double> d;
  auto putd = [&](const double* p, size_t n) { const size_t o = d.size(); if (n) d.insert(d.end(), p, p + n); return o; };
  const size_t o_T = putd(in->frame_T, (size_t)in->n_frames * 7), o_pp = putd(in->pt_pos, (size_t)np * 3), o_pf = putd(in->pt_obs_f, (size_t)npo * 3);
  const size_t o_ss = putd(in->seg_spos, (size_t)ns * 3), o_se = putd(in->seg_epos, (size_t)ns * 3);
  const size_t o_sf = putd(in->seg_obs_sf, (size_t)nso * 3), o_ef = putd(in->seg_obs_ef, (size_t)nso * 3);
  std::vector<int> iv;
  auto puti = [&](const int32_t* p, size_t n) { const size_t o = iv.size(); if (n) iv.insert(iv.end(), p, p + n); return o; };
  const size_t o_po = puti(in->pt_obs_off, np > 0 ? (size_t)np + 1 : 0), o_pfr = puti(in->pt_obs_frame, (size_t)npo);
  const size_t o_so = puti(in->seg_obs_off, ns > 0 ? (size_t)ns + 1 : 0), o_sfr = puti(in->seg_obs_frame, (size_t)nso);
  const size_t dbytes = (d.size() + 1) * sizeof(double), ibytes = (iv.size() + 1) * sizeof(int);
  HIP_TRY(c, c->s_d_in.ensure(dbytes + ibytes));
  HIP_TRY(c, hipMemcpyAsync(c->s_d_in.p, d.data(), d.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (!iv.empty()) HIP_TRY(c, hipMemcpyAsync(reinterpret_cast<char*>(c->s_d_in.p) + dbytes, iv.data(), iv.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  const size_t out_d = (size_t)(np + 2 * ns) * 3, out_i = (size_t)(np + ns);
  HIP_TRY(c, c->s_d_out.ensure((out_d + 1) * sizeof(double) + (out_i + 1) * sizeof(int)));
  const double* dd = c->s_d_in.as<double>();
  const int* di = reinterpret_cast<const int*>(reinterpret_cast<const char*>(c->s_d_in.p) + dbytes);
  double* od = c->s_d_out.as<double>();
  int* oi = reinterpret_cast<int*>(reinterpret_cast<char*>(c->s_d_out.p) + (out_d + 1) * sizeof(double));
  StructBatchDev s{};
  s.frame_T = dd + o_T; s.pt_pos = dd + o_pp; s.pt_obs_f = dd + o_pf; s.seg_spos = dd + o_ss; s.seg_epos = dd + o_se;
  s.seg_obs_sf = dd + o_sf; s.seg_obs_ef = dd + o_ef;
  s.pt_obs_off = di + o_po; s.pt_obs_frame = di + o_pfr; s.seg_obs_off = di + o_so; s.seg_obs_frame = di + o_sfr;
  s.pt_pos_out = od; s.seg_spos_out = od + (size_t)np * 3; s.seg_epos_out = od + (size_t)(np + ns) * 3;
  s.pt_iters = oi; s.seg_iters = oi + np;
  s.n_pts = np; s.n_seg = ns; s.n_iter_pts = in->n_iter_pts; s.n_iter_segs = in->n_iter_segs;
  {
    EventPair ep{}; prof_begin(c, PLSVO_K_STRUCTOPT, &ep);
    HIP_TRY(c, launch_structopt(s, c->stream));
    prof_end(c, PLSVO_K_STRUCTOPT, &ep);
  }
  std::vector<double> hd(out_d + 1);
  std::vector<int> hi(out_i + 1);
  HIP_TRY(c, hipMemcpyAsync(hd.data(), od, out_d * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(hi.data(), oi, out_i * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (out->pt_pos && np) memcpy(out->pt_pos, hd.data(), (size_t)np * 3 * sizeof(double));
  if (out->seg_spos && ns) memcpy(out->seg_spos, hd.data() + (size_t)np * 3, (size_t)ns * 3 * sizeof(double));
  if (out->seg_epos && ns) memcpy(out->seg_epos, hd.data() + (size_t)(np + ns) * 3, (size_t)ns * 3 * sizeof(double));
  if (out->pt_iters && np) memcpy(out->pt_iters, hi.data(), (size_t)np * sizeof(int));
  if (out->seg_iters && ns) memcpy(out->seg_iters, hi.data() + np, (size_t)ns * sizeof(int));
  return PLSVO_OK;
}

// ---- direct feature matching -------------------------------------------------------------------------
constexpr size_t kWarpPatchBytes = 100;   // patch_with_border_: 10 x 10 (match_device.hpp PB_ROWS x PB_STEP)
// one staging, launch and read-back path for plsvo_match_direct (wout == nullptr) and its diagnostic view plsvo_match_warp_patches (out == nullptr)
static int match_run(plsvo_ctx* c, const plsvo_match_in* in, plsvo_match_out* out, plsvo_match_warp_out* wout) {
  CTX_CHECK(c);
  if (!in || (!out && !wout) || in->n < 0 || in->n_frames < 0 || in->n_pyr_levels < 1 || in->align_max_iter < 0)
    return fail(c, PLSVO_E_INVALID, "match_direct: bad arguments");
  const int n = in->n, nf = in->n_frames;
  if (n == 0) return PLSVO_OK;
  if (!c->pyr.base) return fail(c, PLSVO_E_STATE, "match_direct: pyramids not configured");
  if (nf <= 0 || !in->frame_T || !in->frame_slot || !in->cur_frame || !in->ref_frame || !in->ref_px || !in->ref_f || !in->ref_level ||
      !in->ref_type || !in->pos || !in->px_cur)
    return fail(c, PLSVO_E_INVALID, "match_direct: null input array");
  if (in->n_pyr_levels > c->pyr.n_levels) return fail(c, PLSVO_E_INVALID, "match_direct: n_pyr_levels exceeds the configured pyramid");
  if (in->cam.width != c->pyr.w[0] || in->cam.height != c->pyr.h[0]) return fail(c, PLSVO_E_INVALID, "match_direct: camera size does not match the configured pyramid");
  for (int k = 0; k < nf; ++k) if (in->frame_slot[k] < 0 || in->frame_slot[k] >= c->pyr.n_slots) return fail(c, PLSVO_E_CAPACITY, "match_direct: pyramid slot out of range");
  bool any_edgelet = false;
  for (int i = 0; i < n; ++i) {
    if (in->cur_frame[i] < 0 || in->cur_frame[i] >= nf || in->ref_frame[i] < 0 || in->ref_frame[i] >= nf) return fail(c, PLSVO_E_INVALID, "match_direct: frame index out of range");
    if (in->ref_level[i] < 0 || in->ref_level[i] >= c->pyr.n_levels) return fail(c, PLSVO_E_INVALID, "match_direct: ref_level outside the configured pyramid");
    if (in->ref_type[i] == PLSVO_FTR_EDGELET) any_edgelet = true;
    else if (in->ref_type[i] != PLSVO_FTR_CORNER) return fail(c, PLSVO_E_INVALID, "match_direct: unknown feature type");
  }
  if (any_edgelet && !in->ref_grad) return fail(c, PLSVO_E_INVALID, "match_direct: edgelets without ref_grad");
  HIP_TRY(c, hipSetDevice(c->device));
  // one packed upload: doubles, then ints, then bytes
  std::vector<double> d;
  auto putd = [&](const double* p, size_t k) { const size_t o = d.size(); if (p) d.insert(d.end(), p, p + k); else d.resize(d.size() + k, 0.0); return o; };
  const size_t o_T = putd(in->frame_T, (size_t)nf * 7), o_px = putd(in->ref_px, (size_t)n * 2), o_f = putd(in->ref_f, (size_t)n * 3);
  const size_t o_g = putd(in->ref_grad, (size_t)n * 2), o_pos = putd(in->pos, (size_t)n * 3), o_pc = putd(in->px_cur, (size_t)n * 2);
  std::vector<int> iv;
  auto puti = [&](const int32_t* p, size_t k) { const size_t o = iv.size(); iv.insert(iv.end(), p, p + k); return o; };
  const size_t o_slot = puti(in->frame_slot, (size_t)nf), o_cf = puti(in->cur_frame, (size_t)n), o_rf = puti(in->ref_frame, (size_t)n), o_lv = puti(in->ref_level, (size_t)n);
  const size_t dbytes = d.size() * sizeof(double), ibytes = ((iv.size() * sizeof(int) + 15) / 16) * 16, bbytes = (size_t)n;
  HIP_TRY(c, c->s_d_in.ensure(dbytes + ibytes + bbytes + 16));
  char* din = reinterpret_cast<char*>(c->s_d_in.p);
  HIP_TRY(c, hipMemcpyAsync(din, d.data(), dbytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(din + dbytes, iv.data(), iv.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(din + dbytes + ibytes, in->ref_type, bbytes, hipMemcpyHostToDevice, c->stream));
  const size_t out_d = (size_t)n * 2 * sizeof(double), out_i = (size_t)n * 2 * sizeof(int), out_b = (size_t)n;
  // the diagnostic view appends: A (4 doubles), then warped, staged, patch (100 bytes) per candidate
  const size_t o_dA = (out_d + out_i + out_b + 15) / 16 * 16, diag_A = (size_t)n * 4 * sizeof(double), diag_b = (size_t)n * (2 + kWarpPatchBytes);
  HIP_TRY(c, c->s_d_out.ensure((wout ? o_dA + diag_A + diag_b : out_d + out_i + out_b) + 16));
  char* dout = reinterpret_cast<char*>(c->s_d_out.p);
  const double* dd = reinterpret_cast<const double*>(din);
  const int* di = reinterpret_cast<const int*>(din + dbytes);
  MatchBatchDev b{};
  b.pyr_base = c->pyr.base; b.slot_bytes = c->pyr.slot_bytes; b.width = c->pyr.w[0]; b.height = c->pyr.h[0];
  b.fx = in->cam.fx; b.fy = in->cam.fy; b.cx = in->cam.cx; b.cy = in->cam.cy; b.cam_width = in->cam.width; b.cam_height = in->cam.height;
  b.n = n; b.n_pyr_levels = in->n_pyr_levels; b.align_max_iter = in->align_max_iter;
  b.frame_T = dd + o_T; b.ref_px = dd + o_px; b.ref_f = dd + o_f; b.ref_grad = dd + o_g; b.pos = dd + o_pos; b.px_cur = dd + o_pc;
  b.frame_slot = di + o_slot; b.cur_frame = di + o_cf; b.ref_frame = di + o_rf; b.ref_level = di + o_lv;
  b.ref_type = reinterpret_cast<const uint8_t*>(din + dbytes + ibytes);
  b.px_out = reinterpret_cast<double*>(dout);
  b.search_level = reinterpret_cast<int*>(dout + out_d); b.n_iter = b.search_level + n;
  b.found = reinterpret_cast<uint8_t*>(dout + out_d + out_i);
  if (wout) {
    HIP_TRY(c, hipMemsetAsync(dout + o_dA, 0, diag_A + diag_b, c->stream));
    b.diag_A = reinterpret_cast<double*>(dout + o_dA);
    b.diag_warped = reinterpret_cast<uint8_t*>(dout + o_dA + diag_A); b.diag_staged = b.diag_warped + n; b.diag_patch = b.diag_staged + n;
    HIP_TRY(c, launch_match_warp_patches(b, c->stream));
    std::vector<char> h(o_dA + diag_A + diag_b);
    HIP_TRY(c, hipMemcpyAsync(h.data(), dout, h.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const char* hb = h.data() + o_dA + diag_A;
    if (wout->A) memcpy(wout->A, h.data() + o_dA, diag_A);
    if (wout->search_level) memcpy(wout->search_level, h.data() + out_d, (size_t)n * sizeof(int));
    if (wout->warped) memcpy(wout->warped, hb, (size_t)n);
    if (wout->staged) memcpy(wout->staged, hb + n, (size_t)n);
    if (wout->patch) memcpy(wout->patch, hb + 2 * (size_t)n, (size_t)n * kWarpPatchBytes);
    return PLSVO_OK;
  }
  {
    EventPair ep{}; prof_begin(c, PLSVO_K_MATCH, &ep);
    HIP_TRY(c, launch_match_direct(b, c->stream));
    prof_end(c, PLSVO_K_MATCH, &ep);
  }
  std::vector<char> h(out_d + out_i + out_b);
  HIP_TRY(c, hipMemcpyAsync(h.data(), dout, h.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (out->px_cur) memcpy(out->px_cur, h.data(), out_d);
  if (out->search_level) memcpy(out->search_level, h.data() + out_d, (size_t)n * sizeof(int));
  if (out->n_iter) memcpy(out->n_iter, h.data() + out_d + (size_t)n * sizeof(int), (size_t)n * sizeof(int));
  if (out->found) memcpy(out->found, h.data() + out_d + out_i, out_b);
  return PLSVO_OK;
}

extern "C" int plsvo_match_direct(plsvo_ctx* c, const plsvo_match_in* in, plsvo_match_out* out) {
  CTX_CHECK(c);
  if (!out) return fail(c, PLSVO_E_INVALID, "match_direct: bad arguments");
  return match_run(c, in, out, nullptr);
}

extern "C" int plsvo_match_warp_patches(plsvo_ctx* c, const plsvo_match_in* in, plsvo_match_warp_out* out) {
  CTX_CHECK(c);
  if (!out) return fail(c, PLSVO_E_INVALID, "match_warp_patches: bad arguments");
  return match_run(c, in, nullptr, out);
}

// ---- reprojection of landmarks (candidates for the direct matcher) ------------------------------------
extern "C" int plsvo_reproject(plsvo_ctx* c, const plsvo_reproject_in* in, plsvo_reproject_out* out) {
  CTX_CHECK(c);
  if (!in || !out || in->n < 0 || in->n_frames < 0 || in->cell_size <= 0 || in->grid_n_cols <= 0 || in->boundary < 0)
    return fail(c, PLSVO_E_INVALID, "reproject: bad arguments");
  const int n = in->n, nf = in->n_frames;
  if (n == 0) return PLSVO_OK;
  if (nf <= 0 || !in->frame_T || !in->frame || !in->pos) return fail(c, PLSVO_E_INVALID, "reproject: null input array");
  for (int i = 0; i < n; ++i) if (in->frame[i] < 0 || in->frame[i] >= nf) return fail(c, PLSVO_E_INVALID, "reproject: frame index out of range");
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t dT = (size_t)nf * 7, dP = (size_t)n * 3;
  const size_t dbytes = (dT + dP) * sizeof(double), ibytes = (size_t)n * sizeof(int);
  HIP_TRY(c, c->s_d_in.ensure(dbytes + ibytes + 16));
  char* din = reinterpret_cast<char*>(c->s_d_in.p);
  HIP_TRY(c, hipMemcpyAsync(din, in->frame_T, dT * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(din + dT * sizeof(double), in->pos, dP * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(din + dbytes, in->frame, ibytes, hipMemcpyHostToDevice, c->stream));
  const size_t out_d = (size_t)n * 2 * sizeof(double), out_i = (size_t)n * sizeof(int);
  HIP_TRY(c, c->s_d_out.ensure(out_d + out_i + 16));
  char* dout = reinterpret_cast<char*>(c->s_d_out.p);
  ReprojBatchDev b{};
  b.fx = in->cam.fx; b.fy = in->cam.fy; b.cx = in->cam.cx; b.cy = in->cam.cy; b.cam_width = in->cam.width; b.cam_height = in->cam.height;
  b.n = n; b.cell_size = in->cell_size; b.grid_n_cols = in->grid_n_cols; b.boundary = in->boundary;
  b.frame_T = reinterpret_cast<const double*>(din); b.pos = b.frame_T + dT; b.frame = reinterpret_cast<const int*>(din + dbytes);
  b.px = reinterpret_cast<double*>(dout); b.cell = reinterpret_cast<int*>(dout + out_d);
  {
    EventPair ep{}; prof_begin(c, PLSVO_K_MATCH, &ep);
    HIP_TRY(c, launch_reproject(b, c->stream));
    prof_end(c, PLSVO_K_MATCH, &ep);
  }
  std::vector<char> h(out_d + out_i);
  HIP_TRY(c, hipMemcpyAsync(h.data(), dout, h.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (out->px) memcpy(out->px, h.data(), out_d);
  if (out->cell) memcpy(out->cell, h.data() + out_d, out_i);
  return PLSVO_OK;
}

// ---- resident frame step ------------------------------------------------------------------------------
namespace {
// carve typed arrays out of one device allocation (256-byte aligned sections)
struct Carver {
  size_t off = 0;
  template <typename T> size_t take(size_t n) { const size_t o = (off + 255) & ~(size_t)255; off = o + std::max(n, (size_t)1) * sizeof(T); return o; }
};
}  // namespace

// ---- keyframe stage: close keyframes, scene depth, new-keyframe test, key points (keyframe_device.hpp) --------------------
extern "C" int plsvo_close_keyframes(plsvo_ctx* c, int n, const plsvo_close_kf_in* in, plsvo_close_kf_out* out) {
  CTX_CHECK(c);
  if (n < 0 || (n > 0 && (!in || !out))) return fail(c, PLSVO_E_INVALID, "close_keyframes: bad arguments");
  if (n == 0) return PLSVO_OK;
  size_t total = 0;
  for (int i = 0; i < n; ++i) {
    if (in[i].n_kf < 0 || in[i].max_n_kfs < 0) return fail(c, PLSVO_E_INVALID, "close_keyframes: negative count");
    if (in[i].n_kf > 0 && (!in[i].kf_T || !in[i].keypt_pos || !in[i].keypt_valid)) return fail(c, PLSVO_E_INVALID, "close_keyframes: null table array");
    total += (size_t)in[i].n_kf;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  // the streams' tables are packed straight into the blob that travels (one pass over the caller's arrays)
  Blob blob;
  blob.host.reserve((size_t)n * sizeof(CloseKfJobDev) + total * (22 * sizeof(double) + 5) + 4 * 512);
  const size_t o_jobs = blob.reserve<CloseKfJobDev>((size_t)n), o_T = blob.reserve<double>(total * 7), o_kp = blob.reserve<double>(total * 15),
               o_kv = blob.reserve<uint8_t>(total * 5);
  CloseKfJobDev* jobs = blob.at<CloseKfJobDev>(o_jobs);
  double* kf_T = blob.at<double>(o_T); double* kp = blob.at<double>(o_kp); uint8_t* kv = blob.at<uint8_t>(o_kv);
  size_t off = 0;
  for (int i = 0; i < n; ++i) {
    CloseKfJobDev& J = jobs[(size_t)i];
    memcpy(J.T, in[i].T_f_w, sizeof(J.T));
    J.fx = in[i].cam.fx; J.fy = in[i].cam.fy; J.cx = in[i].cam.cx; J.cy = in[i].cam.cy; J.width = in[i].cam.width; J.height = in[i].cam.height;
    J.n_kf = in[i].n_kf; J.max_n_kfs = in[i].max_n_kfs; J.kf_off = (long long)off;
    const size_t k = (size_t)in[i].n_kf;
    if (k) {
      memcpy(kf_T + off * 7, in[i].kf_T, k * 7 * sizeof(double));
      memcpy(kp + off * 15, in[i].keypt_pos, k * 15 * sizeof(double));
      memcpy(kv + off * 5, in[i].keypt_valid, k * 5);
    }
    off += k;
  }
  int rc;
  if ((rc = upload_blob(c, c->s_d_in, blob))) return rc;
  Carver cv;
  const size_t o_tmp = cv.take<double>(total), o_idx = cv.take<int>(total), o_dist = cv.take<double>(total), o_cnt = cv.take<int>((size_t)n * 2);
  HIP_TRY(c, c->s_d_out.ensure(cv.off + 256));
  char* din = reinterpret_cast<char*>(c->s_d_in.p); char* dout = reinterpret_cast<char*>(c->s_d_out.p);
  CloseKfBatchDev b{};
  b.jobs = reinterpret_cast<const CloseKfJobDev*>(din + o_jobs); b.n_jobs = n;
  b.kf_T = reinterpret_cast<const double*>(din + o_T); b.keypt_pos = reinterpret_cast<const double*>(din + o_kp);
  b.keypt_valid = reinterpret_cast<const uint8_t*>(din + o_kv);
  b.tmp_dist = reinterpret_cast<double*>(dout + o_tmp); b.close_idx = reinterpret_cast<int*>(dout + o_idx);
  b.close_dist = reinterpret_cast<double*>(dout + o_dist); b.counts = reinterpret_cast<int*>(dout + o_cnt);
  {
    EventPair ep{}; prof_begin(c, PLSVO_K_KEYFRAME, &ep);
    HIP_TRY(c, launch_close_keyframes(b, c->stream));
    prof_end(c, PLSVO_K_KEYFRAME, &ep);
  }
  std::vector<char> h(cv.off);
  HIP_TRY(c, hipMemcpyAsync(h.data(), dout, h.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const int* h_idx = reinterpret_cast<const int*>(h.data() + o_idx); const double* h_dist = reinterpret_cast<const double*>(h.data() + o_dist);
  const int* h_cnt = reinterpret_cast<const int*>(h.data() + o_cnt);
  for (int i = 0; i < n; ++i) {
    const size_t at = (size_t)blob.at<CloseKfJobDev>(o_jobs)[(size_t)i].kf_off;
    const int nc = h_cnt[2 * i];
    out[i].n_close = nc; out[i].n_overlap = h_cnt[2 * i + 1];
    if (out[i].close_idx && nc > 0) memcpy(out[i].close_idx, h_idx + at, (size_t)nc * sizeof(int));
    if (out[i].close_dist && nc > 0) memcpy(out[i].close_dist, h_dist + at, (size_t)nc * sizeof(double));
  }
  return PLSVO_OK;
}

extern "C" int plsvo_keyframe_decide(plsvo_ctx* c, int n, const plsvo_kf_decide_in* in, plsvo_kf_decide_out* out) {
  CTX_CHECK(c);
  if (n < 0 || (n > 0 && (!in || !out))) return fail(c, PLSVO_E_INVALID, "keyframe_decide: bad arguments");
  if (n == 0) return PLSVO_OK;
  size_t t_pt = 0, t_seg = 0, t_kf = 0, t_ov = 0;
  for (int i = 0; i < n; ++i) {
    const plsvo_kf_decide_in& I = in[i];
    if (I.n_pt < 0 || I.n_seg < 0 || I.n_kf < 0 || I.n_overlap < 0) return fail(c, PLSVO_E_INVALID, "keyframe_decide: negative count");
    if ((I.n_pt > 0 && (!I.pt_px || !I.pt_pos)) || (I.n_seg > 0 && (!I.seg_spos || !I.seg_epos)) || (I.n_kf > 0 && !I.kf_T) ||
        (I.n_overlap > 0 && !I.overlap_idx))
      return fail(c, PLSVO_E_INVALID, "keyframe_decide: null array with a non-zero count");
    for (int k = 0; k < I.n_overlap; ++k)
      if (I.overlap_idx[k] < 0 || I.overlap_idx[k] >= I.n_kf) return fail(c, PLSVO_E_INVALID, "keyframe_decide: overlap index outside the keyframe table");
    for (int k = 0; k < 5; ++k)
      if (I.key_pts_prev[k] < -1 || I.key_pts_prev[k] >= I.n_pt) return fail(c, PLSVO_E_INVALID, "keyframe_decide: key_pts_prev outside the points");
    t_pt += (size_t)I.n_pt; t_seg += (size_t)I.n_seg; t_kf += (size_t)I.n_kf; t_ov += (size_t)I.n_overlap;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  // the streams' lists are packed straight into the blob that travels (one pass over the caller's arrays)
  Blob blob;
  blob.host.reserve((size_t)n * sizeof(KfDecideJobDev) + t_pt * (5 * sizeof(double) + 1) + t_seg * (6 * sizeof(double) + 1) + t_kf * 7 * sizeof(double) +
                    t_ov * sizeof(int) + 9 * 512);
  const size_t b_jobs = blob.reserve<KfDecideJobDev>((size_t)n), b_px = blob.reserve<double>(t_pt * 2), b_pos = blob.reserve<double>(t_pt * 3),
               b_pa = blob.reserve<uint8_t>(t_pt), b_sp = blob.reserve<double>(t_seg * 3), b_ep = blob.reserve<double>(t_seg * 3),
               b_sa = blob.reserve<uint8_t>(t_seg), b_kf = blob.reserve<double>(t_kf * 7), b_ov = blob.reserve<int>(t_ov);
  KfDecideJobDev* jobs = blob.at<KfDecideJobDev>(b_jobs);
  double* pt_px = blob.at<double>(b_px); double* pt_pos = blob.at<double>(b_pos); uint8_t* pa = blob.at<uint8_t>(b_pa);
  double* sp = blob.at<double>(b_sp); double* ep = blob.at<double>(b_ep); uint8_t* sa = blob.at<uint8_t>(b_sa);
  double* kf_T = blob.at<double>(b_kf); int* ov = blob.at<int>(b_ov);
  size_t o_pt = 0, o_seg = 0, o_kf = 0, o_ov = 0, o_depth = 0;
  for (int i = 0; i < n; ++i) {
    const plsvo_kf_decide_in& I = in[i];
    KfDecideJobDev& J = jobs[(size_t)i];
    memcpy(J.T_new, I.T_new_w, sizeof(J.T_new)); memcpy(J.T_last, I.T_last_w, sizeof(J.T_last));
    J.d_T_new = I.d_T_new; J.min_t = I.kfselect_mindist_t; J.min_r = I.kfselect_mindist_r;
    J.width = I.cam.width; J.height = I.cam.height;
    J.n_pt = I.n_pt; J.n_seg = I.n_seg; J.n_kf = I.n_kf; J.n_ov = I.n_overlap;
    J.pt_off = (long long)o_pt; J.seg_off = (long long)o_seg; J.kf_off = (long long)o_kf; J.ov_off = (long long)o_ov; J.depth_off = (long long)o_depth;
    for (int k = 0; k < 5; ++k) J.key_prev[k] = I.key_pts_prev[k];
    J.reserved0 = 0;
    const size_t np = (size_t)I.n_pt, ns = (size_t)I.n_seg, nk = (size_t)I.n_kf, no = (size_t)I.n_overlap;
    if (np) {
      memcpy(pt_px + o_pt * 2, I.pt_px, np * 2 * sizeof(double)); memcpy(pt_pos + o_pt * 3, I.pt_pos, np * 3 * sizeof(double));
      if (I.pt_alive) for (size_t k = 0; k < np; ++k) pa[o_pt + k] = I.pt_alive[k] ? 1 : 0;
      else memset(pa + o_pt, 1, np);
    }
    if (ns) {
      memcpy(sp + o_seg * 3, I.seg_spos, ns * 3 * sizeof(double)); memcpy(ep + o_seg * 3, I.seg_epos, ns * 3 * sizeof(double));
      if (I.seg_alive) for (size_t k = 0; k < ns; ++k) sa[o_seg + k] = I.seg_alive[k] ? 1 : 0;
      else memset(sa + o_seg, 1, ns);
    }
    if (nk) memcpy(kf_T + o_kf * 7, I.kf_T, nk * 7 * sizeof(double));
    if (no) memcpy(ov + o_ov, I.overlap_idx, no * sizeof(int));
    o_pt += np; o_seg += ns; o_kf += nk; o_ov += no; o_depth += np + 2 * ns;
  }
  int rc;
  if ((rc = upload_blob(c, c->s_d_in, blob))) return rc;
  Carver cv;   // results first (what travels back), the depth rows behind them
  const size_t r_out = cv.take<KfDecideOutDev>((size_t)n), r_dt = cv.take<double>(t_ov), r_dr = cv.take<double>(t_ov);
  const size_t fetch_bytes = cv.off;
  const size_t r_keys = cv.take<unsigned long long>(o_depth);
  HIP_TRY(c, c->s_d_out.ensure(cv.off + 256));
  char* din = reinterpret_cast<char*>(c->s_d_in.p); char* dout = reinterpret_cast<char*>(c->s_d_out.p);
  KfDecideBatchDev b{};
  b.jobs = reinterpret_cast<const KfDecideJobDev*>(din + b_jobs); b.out = reinterpret_cast<KfDecideOutDev*>(dout + r_out); b.n_jobs = n;
  b.pt_px = reinterpret_cast<const double*>(din + b_px); b.pt_pos = reinterpret_cast<const double*>(din + b_pos);
  b.pt_alive = reinterpret_cast<const uint8_t*>(din + b_pa);
  b.seg_spos = reinterpret_cast<const double*>(din + b_sp); b.seg_epos = reinterpret_cast<const double*>(din + b_ep);
  b.seg_alive = reinterpret_cast<const uint8_t*>(din + b_sa);
  b.kf_T = reinterpret_cast<const double*>(din + b_kf); b.overlap_idx = reinterpret_cast<const int*>(din + b_ov);
  b.depth_keys = reinterpret_cast<unsigned long long*>(dout + r_keys);
  b.delta_t = reinterpret_cast<double*>(dout + r_dt); b.delta_r = reinterpret_cast<double*>(dout + r_dr);
  {
    EventPair ep{}; prof_begin(c, PLSVO_K_KEYFRAME, &ep);
    HIP_TRY(c, launch_keyframe_decide(b, c->stream));
    prof_end(c, PLSVO_K_KEYFRAME, &ep);
  }
  std::vector<char> h(fetch_bytes);
  HIP_TRY(c, hipMemcpyAsync(h.data(), dout, h.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const KfDecideOutDev* ho = reinterpret_cast<const KfDecideOutDev*>(h.data() + r_out);
  const double* h_dt = reinterpret_cast<const double*>(h.data() + r_dt); const double* h_dr = reinterpret_cast<const double*>(h.data() + r_dr);
  for (int i = 0; i < n; ++i) {
    const KfDecideOutDev& o = ho[i];
    plsvo_kf_decide_out& O = out[i];
    O.depth_mean = o.depth_mean; O.depth_min = o.depth_min; O.has_depth = o.has_depth; O.n_depth = o.n_depth;
    O.need_new_kf = o.need_new_kf; O.blocking = o.blocking; O.furthest_kf = o.furthest_kf;
    for (int k = 0; k < 5; ++k) O.key_pts[k] = o.key_pts[k];
    const size_t at = (size_t)blob.at<KfDecideJobDev>(b_jobs)[(size_t)i].ov_off, no = (size_t)in[i].n_overlap;
    if (O.delta_t && no) memcpy(O.delta_t, h_dt + at, no * sizeof(double));
    if (O.delta_r && no) memcpy(O.delta_r, h_dr + at, no * sizeof(double));
  }
  return PLSVO_OK;
}

extern "C" int plsvo_chain_stage(plsvo_ctx* c, int n, const plsvo_chain_in* in, const plsvo_chain_params* pr) {
  CTX_CHECK(c);
  if (n <= 0 || !in || !pr) return fail(c, PLSVO_E_INVALID, "chain_stage: bad arguments");
  if (pr->cell_size <= 0 || pr->n_pyr_levels < 1 || pr->align_max_iter < 0 || pr->poseopt_n_iter < 0 || pr->max_fts < 0)
    return fail(c, PLSVO_E_INVALID, "chain_stage: bad parameters");
  if (!c->pyr.base) return fail(c, PLSVO_E_STATE, "chain_stage: pyramids not configured");
  if (pr->n_pyr_levels > c->pyr.n_levels) return fail(c, PLSVO_E_INVALID, "chain_stage: n_pyr_levels exceeds the configured pyramid");
  if (pr->cam.width != c->pyr.w[0] || pr->cam.height != c->pyr.h[0]) return fail(c, PLSVO_E_INVALID, "chain_stage: camera size does not match the configured pyramid");
  c->ch_staged = false;
  // the alignment part is an ordinary staged alignment batch
  std::vector<plsvo_align_in> ain((size_t)n);
  for (int j = 0; j < n; ++j) ain[(size_t)j] = in[j].align;
  int rc = plsvo_align_stage(c, n, ain.data()); if (rc) return rc;
  const int grid_n_cols = (pr->cam.width + pr->cell_size - 1) / pr->cell_size, grid_n_rows = (pr->cam.height + pr->cell_size - 1) / pr->cell_size;
  const int n_cells = grid_n_cols * grid_n_rows;
  const bool seg_grid = pr->cell_rule && pr->seg_cell_size > 0;
  if (pr->seg_cell_size < 0 || (seg_grid && pr->max_fts_segs < 0)) return fail(c, PLSVO_E_INVALID, "chain_stage: bad segment-grid parameters");
  const int seg_n_cols = seg_grid ? (pr->cam.width + pr->seg_cell_size - 1) / pr->seg_cell_size : 0;
  const int seg_n_cells = seg_grid ? seg_n_cols * ((pr->cam.height + pr->seg_cell_size - 1) / pr->seg_cell_size) : 0;
  if (pr->cell_rule && ((size_t)n_cells + (size_t)seg_n_cells) * sizeof(int) > 60000) return fail(c, PLSVO_E_CAPACITY, "chain_stage: reprojection grid too fine for the selection kernel");
  if (seg_grid && pr->seg_cell_order)
    for (int k = 0; k < seg_n_cells; ++k) if (pr->seg_cell_order[k] < 0 || pr->seg_cell_order[k] >= seg_n_cells) return fail(c, PLSVO_E_INVALID, "chain_stage: seg_cell_order entry out of range");
  if (pr->cell_rule && pr->cell_order)
    for (int k = 0; k < n_cells; ++k) if (pr->cell_order[k] < 0 || pr->cell_order[k] >= n_cells) return fail(c, PLSVO_E_INVALID, "chain_stage: cell_order entry out of range");
  std::vector<ChainJobDev> jobs((size_t)n);
  std::vector<double> pos, rpx, rf, rgrad;
  std::vector<int> rlevel, cand_job, frame_cur, frame_ref, order, seg_order;
  std::vector<uint8_t> rtype, active;
  bool any_active = false, any_edgelet = false;
  int npt_total = 0, nseg_total = 0;
  for (int j = 0; j < n; ++j) {
    const plsvo_chain_in& a = in[j];
    const int nc = a.n_cand_pt + 2 * a.n_cand_seg;
    if (a.n_cand_pt < 0 || a.n_cand_seg < 0) return fail(c, PLSVO_E_INVALID, "chain_stage: negative candidate count");
    if (nc > 0 && (!a.pos || !a.ref_px || !a.ref_f || !a.ref_level)) return fail(c, PLSVO_E_INVALID, "chain_stage: null candidate array");
    if (a.kf_slot < 0 || a.kf_slot >= c->pyr.n_slots) return fail(c, PLSVO_E_CAPACITY, "chain_stage: keyframe slot out of range");
    ChainJobDev& J = jobs[(size_t)j];
    for (int k = 0; k < 7; ++k) { J.T_prev[k] = a.T_prev_w[k]; J.T_kf[k] = a.T_kf_w[k]; }
    J.kf_slot = a.kf_slot; J.cur_slot = a.align.cur_slot;
    J.cand_off = (int)cand_job.size(); J.n_pt = a.n_cand_pt; J.n_seg = a.n_cand_seg;
    J.po_pt_off = npt_total; J.po_seg_off = nseg_total; J.reserved0 = 0;
    npt_total += a.n_cand_pt; nseg_total += (seg_grid ? 2 : 1) * a.n_cand_seg;   // (a segment that wins both of its cells is a feature twice)
    pos.insert(pos.end(), a.pos, a.pos + 3 * (size_t)nc);
    rpx.insert(rpx.end(), a.ref_px, a.ref_px + 2 * (size_t)nc);
    rf.insert(rf.end(), a.ref_f, a.ref_f + 3 * (size_t)nc);
    for (int k = 0; k < nc; ++k) {
      if (a.ref_level[k] < 0 || a.ref_level[k] >= c->pyr.n_levels) return fail(c, PLSVO_E_INVALID, "chain_stage: ref_level outside the configured pyramid");
      const uint8_t ty = (a.ref_type && k < a.n_cand_pt) ? a.ref_type[k] : (uint8_t)PLSVO_FTR_CORNER;
      if (ty == PLSVO_FTR_EDGELET) any_edgelet = true; else if (ty != PLSVO_FTR_CORNER) return fail(c, PLSVO_E_INVALID, "chain_stage: unknown feature type");
      if (ty == PLSVO_FTR_EDGELET && !a.ref_grad) return fail(c, PLSVO_E_INVALID, "chain_stage: edgelets without ref_grad");
      rtype.push_back(ty);
      const bool has_grad = a.ref_grad && k < a.n_cand_pt;   // ref_type / ref_grad are sized by the POINT candidates (header); end points: 0
      rgrad.push_back(has_grad ? a.ref_grad[2 * k] : 0.0); rgrad.push_back(has_grad ? a.ref_grad[2 * k + 1] : 0.0);
      rlevel.push_back(a.ref_level[k]);
      active.push_back(a.active ? (a.active[k] ? 1 : 0) : 1);
      if (a.active) any_active = true;
      cand_job.push_back(j); frame_ref.push_back(2 * j); frame_cur.push_back(2 * j + 1);
    }
  }
  (void)any_edgelet;
  const size_t NC = cand_job.size();
  if (pr->cell_rule) { order.resize((size_t)n_cells); for (int k = 0; k < n_cells; ++k) order[(size_t)k] = pr->cell_order ? pr->cell_order[k] : k; }
  if (seg_grid) { seg_order.resize((size_t)seg_n_cells); for (int k = 0; k < seg_n_cells; ++k) seg_order[(size_t)k] = pr->seg_cell_order ? pr->seg_cell_order[k] : k; }
  Blob blob;
  const size_t o_jobs = blob.add(jobs), o_pos = blob.add(pos), o_rpx = blob.add(rpx), o_rf = blob.add(rf), o_rgrad = blob.add(rgrad), o_rlevel = blob.add(rlevel),
               o_cjob = blob.add(cand_job), o_fcur = blob.add(frame_cur), o_fref = blob.add(frame_ref), o_rtype = blob.add(rtype), o_active = blob.add(active),
               o_order = blob.add(order), o_sorder = blob.add(seg_order);
  if ((rc = upload_blob(c, c->ch_d_blob, blob))) return rc;
  // work arrays
  Carver w;
  const size_t w_frameT = w.take<double>((size_t)n * 14), w_fslot = w.take<int>((size_t)n * 2), w_px = w.take<double>(NC * 2), w_cell = w.take<int>(NC),
               w_act = w.take<uint8_t>(NC), w_mpx = w.take<double>(NC * 2), w_found = w.take<uint8_t>(NC), w_slevel = w.take<int>(NC), w_niter = w.take<int>(NC),
               w_selpt = w.take<int>((size_t)npt_total), w_selseg = w.take<int>((size_t)nseg_total), w_nsel = w.take<int>((size_t)n * 2);
  HIP_TRY(c, c->ch_d_work.ensure(w.off + 256));
  Carver p;
  const size_t p_jobs = p.take<PoseJobDev>((size_t)n), p_ptf = p.take<double>((size_t)npt_total * 3), p_ptpos = p.take<double>((size_t)npt_total * 3),
               p_ptlev = p.take<int>((size_t)npt_total), p_line = p.take<double>((size_t)nseg_total * 3), p_spos = p.take<double>((size_t)nseg_total * 3),
               p_epos = p.take<double>((size_t)nseg_total * 3), p_slev = p.take<int>((size_t)nseg_total);
  HIP_TRY(c, c->ch_d_po.ensure(p.off + 256));
  const size_t nft = std::max((size_t)npt_total + (size_t)nseg_total, (size_t)1);
  HIP_TRY(c, c->ch_d_ptkeep.ensure(std::max((size_t)npt_total, (size_t)1)));
  HIP_TRY(c, c->ch_d_segkeep.ensure(std::max((size_t)nseg_total, (size_t)1)));
  HIP_TRY(c, c->ch_d_s32.ensure(nft * sizeof(float)));
  HIP_TRY(c, c->ch_d_s64.ensure(nft * 5 * sizeof(double)));
  HIP_TRY(c, c->ch_d_state.ensure((size_t)n * sizeof(PoseStateDev)));
  HIP_TRY(c, c->ch_d_poses.ensure((size_t)n * 7 * sizeof(double)));
  uint8_t* const B = c->ch_d_blob.as<uint8_t>();
  uint8_t* const Wk = c->ch_d_work.as<uint8_t>();
  uint8_t* const Po = c->ch_d_po.as<uint8_t>();
  ChainBatchDev& b = c->ch_b;
  b = ChainBatchDev{};
  b.jobs = reinterpret_cast<const ChainJobDev*>(B + o_jobs); b.n_jobs = n; b.n_cand = (int)NC;
  b.align_poses = c->a_d_poses.as<double>();
  b.frame_T = reinterpret_cast<double*>(Wk + w_frameT); b.frame_slot = reinterpret_cast<int*>(Wk + w_fslot);
  b.cand_job = reinterpret_cast<const int*>(B + o_cjob); b.pos = reinterpret_cast<const double*>(B + o_pos);
  b.active_in = any_active ? B + o_active : nullptr;
  b.cell = reinterpret_cast<const int*>(Wk + w_cell); b.active = Wk + w_act;
  b.m_px = reinterpret_cast<const double*>(Wk + w_mpx); b.found = Wk + w_found; b.search_level = reinterpret_cast<const int*>(Wk + w_slevel);
  b.fx = pr->cam.fx; b.fy = pr->cam.fy; b.cx = pr->cam.cx; b.cy = pr->cam.cy;
  b.n_cells = n_cells; b.cell_rule = pr->cell_rule ? 1 : 0; b.max_fts = pr->max_fts;
  b.cell_order = pr->cell_rule ? reinterpret_cast<const int*>(B + o_order) : nullptr;
  b.proj_px = reinterpret_cast<const double*>(Wk + w_px);
  b.seg_cell_size = seg_grid ? pr->seg_cell_size : 0; b.seg_n_cols = seg_n_cols; b.seg_n_cells = seg_n_cells; b.max_fts_segs = pr->max_fts_segs;
  b.seg_cell_order = seg_grid ? reinterpret_cast<const int*>(B + o_sorder) : nullptr;
  b.po_jobs = reinterpret_cast<PoseJobDev*>(Po + p_jobs);
  b.pt_f = reinterpret_cast<double*>(Po + p_ptf); b.pt_pos = reinterpret_cast<double*>(Po + p_ptpos); b.pt_level = reinterpret_cast<int*>(Po + p_ptlev);
  b.seg_line = reinterpret_cast<double*>(Po + p_line); b.seg_spos = reinterpret_cast<double*>(Po + p_spos); b.seg_epos = reinterpret_cast<double*>(Po + p_epos);
  b.seg_level = reinterpret_cast<int*>(Po + p_slev);
  b.sel_pt = reinterpret_cast<int*>(Wk + w_selpt); b.sel_seg = reinterpret_cast<int*>(Wk + w_selseg); b.n_sel = reinterpret_cast<int*>(Wk + w_nsel);
  b.reproj_thresh = pr->reproj_thresh; b.po_n_iter = pr->poseopt_n_iter; b.ldlt_flavour = c->ldlt_flavour;
  ReprojBatchDev& r = c->ch_reproj;
  r = ReprojBatchDev{};
  r.fx = pr->cam.fx; r.fy = pr->cam.fy; r.cx = pr->cam.cx; r.cy = pr->cam.cy; r.cam_width = pr->cam.width; r.cam_height = pr->cam.height;
  r.n = (int)NC; r.cell_size = pr->cell_size; r.grid_n_cols = grid_n_cols; r.boundary = 8;
  r.frame_T = b.frame_T; r.frame = reinterpret_cast<const int*>(B + o_fcur); r.pos = b.pos;
  r.px = reinterpret_cast<double*>(Wk + w_px); r.cell = reinterpret_cast<int*>(Wk + w_cell);
  MatchBatchDev& m = c->ch_match;
  m = MatchBatchDev{};
  m.pyr_base = c->pyr.base; m.slot_bytes = c->pyr.slot_bytes; m.width = c->pyr.w[0]; m.height = c->pyr.h[0];
  m.fx = pr->cam.fx; m.fy = pr->cam.fy; m.cx = pr->cam.cx; m.cy = pr->cam.cy; m.cam_width = pr->cam.width; m.cam_height = pr->cam.height;
  m.n = (int)NC; m.n_pyr_levels = pr->n_pyr_levels; m.align_max_iter = pr->align_max_iter;
  m.frame_T = b.frame_T; m.frame_slot = b.frame_slot; m.cur_frame = r.frame; m.ref_frame = reinterpret_cast<const int*>(B + o_fref);
  m.ref_px = reinterpret_cast<const double*>(B + o_rpx); m.ref_f = reinterpret_cast<const double*>(B + o_rf); m.ref_level = reinterpret_cast<const int*>(B + o_rlevel);
  m.ref_type = B + o_rtype; m.ref_grad = reinterpret_cast<const double*>(B + o_rgrad); m.pos = b.pos; m.px_cur = r.px;
  m.px_out = reinterpret_cast<double*>(Wk + w_mpx); m.found = Wk + w_found; m.search_level = reinterpret_cast<int*>(Wk + w_slevel); m.n_iter = reinterpret_cast<int*>(Wk + w_niter);
  m.active = b.active;
  PoseBatchDev& q = c->ch_pose;
  q = PoseBatchDev{};
  q.jobs = b.po_jobs; q.state = c->ch_d_state.as<PoseStateDev>();
  q.pt_f = b.pt_f; q.pt_pos = b.pt_pos; q.pt_level = b.pt_level; q.seg_line = b.seg_line; q.seg_spos = b.seg_spos; q.seg_epos = b.seg_epos; q.seg_level = b.seg_level;
  q.pt_keep = c->ch_d_ptkeep.as<uint8_t>(); q.seg_keep = c->ch_d_segkeep.as<uint8_t>();
  q.scratch_f32 = c->ch_d_s32.as<float>(); q.scratch_f64 = c->ch_d_s64.as<double>();
  q.log = nullptr; q.log_cap = 0; q.n_jobs = n;
  c->ch_jobs.swap(jobs);
  c->ch_n = n; c->ch_ncand = (int)NC; c->ch_npt_cap = npt_total; c->ch_nseg_cap = nseg_total;
  c->ch_staged = true; c->ch_run_seq = 0;
  return PLSVO_OK;
}

extern "C" int plsvo_chain_run(plsvo_ctx* c) {
  CTX_CHECK(c);
  RoctxRange range("frame_step");
  if (!c->ch_staged || !c->a_staged || c->a_n != c->ch_n) return fail(c, PLSVO_E_STATE, "chain_run: no staged frame step (or the alignment batch was re-staged since)");
  int rc = plsvo_align_run(c); if (rc) return rc;
  HIP_TRY(c, launch_chain_pose(c->ch_b, c->stream));
  { EventPair ep{}; prof_begin(c, PLSVO_K_MATCH, &ep);
    HIP_TRY(c, launch_reproject(c->ch_reproj, c->stream));
    HIP_TRY(c, launch_chain_active(c->ch_b, c->stream));
    HIP_TRY(c, launch_match_direct(c->ch_match, c->stream));
    HIP_TRY(c, launch_chain_select(c->ch_b, c->stream));
    prof_end(c, PLSVO_K_MATCH, &ep); }
  const int threads = pose_opt_threads(c, c->ch_n, (long)c->ch_b.n_cand);   // (selected features <= candidates)
  c->p_refill_frames = 0;   // (the chain's jobs are written on the device: the host cannot see whether one has a refinement loop -- pose_opt_rows_kernel)
  EventPair ep{}; prof_begin(c, PLSVO_K_POSEOPT, &ep);
  HIP_TRY(c, launch_pose_opt(c->ch_pose, c->ch_d_poses.as<double>(), threads, c->opt_poseopt_select ? 1 : 0, c->stream));
  prof_end(c, PLSVO_K_POSEOPT, &ep);
  c->ch_run_seq = ++c->run_seq;
  return PLSVO_OK;
}

extern "C" const double* plsvo_chain_poses_dev(plsvo_ctx* c) { return (c && c->ch_staged) ? c->ch_d_poses.as<double>() : nullptr; }

extern "C" int plsvo_chain_fetch(plsvo_ctx* c, int n, plsvo_chain_out* out) {
  CTX_CHECK(c);
  if (!c->ch_staged) return fail(c, PLSVO_E_STATE, "chain_fetch: no staged frame step");
  if (n != c->ch_n || !out) return fail(c, PLSVO_E_INVALID, "chain_fetch: n does not match the staged batch");
  // the alignment results through the ordinary fetch (the caller's seg_alive_out buffers are honoured)
  std::vector<plsvo_align_out> ao((size_t)n);
  for (int j = 0; j < n; ++j) ao[(size_t)j].seg_alive_out = out[j].align.seg_alive_out;
  int rc = plsvo_align_fetch(c, n, ao.data()); if (rc) return rc;
  const size_t NC = (size_t)c->ch_ncand, NP = (size_t)c->ch_npt_cap, NS = (size_t)c->ch_nseg_cap;
  std::vector<PoseStateDev> st((size_t)n);
  std::vector<uint8_t> found(std::max(NC, (size_t)1)), pk(std::max(NP, (size_t)1)), sk(std::max(NS, (size_t)1));
  std::vector<double> mpx(std::max(NC * 2, (size_t)1));
  std::vector<int> slev(std::max(NC, (size_t)1)), selp(std::max(NP, (size_t)1)), sels(std::max(NS, (size_t)1)), nsel((size_t)n * 2);
  const ChainBatchDev& b = c->ch_b;
  HIP_TRY(c, hipMemcpyAsync(st.data(), c->ch_d_state.p, (size_t)n * sizeof(PoseStateDev), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(nsel.data(), b.n_sel, (size_t)n * 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (NC) {
    HIP_TRY(c, hipMemcpyAsync(found.data(), b.found, NC, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(mpx.data(), b.m_px, NC * 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(slev.data(), b.search_level, NC * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  }
  if (NP) {
    HIP_TRY(c, hipMemcpyAsync(pk.data(), c->ch_d_ptkeep.p, NP, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(selp.data(), b.sel_pt, NP * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  }
  if (NS) {
    HIP_TRY(c, hipMemcpyAsync(sk.data(), c->ch_d_segkeep.p, NS, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(sels.data(), b.sel_seg, NS * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int j = 0; j < n; ++j) {
    const ChainJobDev& J = c->ch_jobs[(size_t)j];
    const PoseStateDev& s = st[(size_t)j];
    plsvo_chain_out& o = out[j];
    o.align = ao[(size_t)j];
    uint8_t* pko = o.pose.pt_keep; uint8_t* sko = o.pose.seg_keep;
    memset(&o.pose, 0, sizeof(o.pose));
    o.pose.pt_keep = pko; o.pose.seg_keep = sko;
    for (int k = 0; k < 7; ++k) o.pose.T_f_w[k] = s.T[k];
    for (int k = 0; k < 36; ++k) o.pose.cov[k] = s.cov[k];
    o.pose.estimated_scale = s.estimated_scale; o.pose.error_init = s.error_init; o.pose.error_final = s.error_final;
    o.pose.num_obs_pt = s.num_obs_pt; o.pose.num_obs_ls = s.num_obs_ls;
    o.pose.iters = s.iters; o.pose.iters_ref = s.iters_ref; o.pose.status = s.status;
    o.n_sel_pt = nsel[(size_t)j * 2]; o.n_sel_seg = nsel[(size_t)j * 2 + 1];
    const int nc = J.n_pt + 2 * J.n_seg;
    if (pko && o.n_sel_pt > 0) memcpy(pko, pk.data() + J.po_pt_off, (size_t)o.n_sel_pt);
    if (sko && o.n_sel_seg > 0) memcpy(sko, sk.data() + J.po_seg_off, (size_t)o.n_sel_seg);
    if (o.found && nc) memcpy(o.found, found.data() + J.cand_off, (size_t)nc);
    if (o.px && nc) memcpy(o.px, mpx.data() + 2 * (size_t)J.cand_off, (size_t)nc * 2 * sizeof(double));
    if (o.search_level && nc) memcpy(o.search_level, slev.data() + J.cand_off, (size_t)nc * sizeof(int));
    if (o.sel_pt && o.n_sel_pt > 0) memcpy(o.sel_pt, selp.data() + J.po_pt_off, (size_t)o.n_sel_pt * sizeof(int));
    if (o.sel_seg && o.n_sel_seg > 0) memcpy(o.sel_seg, sels.data() + J.po_seg_off, (size_t)o.n_sel_seg * sizeof(int));
  }
  return PLSVO_OK;
}

extern "C" int plsvo_frame_step_batch(plsvo_ctx* c, int n, const plsvo_chain_in* in, const plsvo_chain_params* params, plsvo_chain_out* out) {
  int rc = plsvo_chain_stage(c, n, in, params); if (rc) return rc;
  rc = plsvo_chain_run(c); if (rc) return rc;
  return plsvo_chain_fetch(c, n, out);
}

// ---- map candidates: overlap keyframes' features, first visit, closest view, quality order (candidates_device.hpp) ---------
namespace {
struct CandTotals { size_t kf = 0, kfpt = 0, kfseg = 0, pt = 0, seg = 0, ptobs = 0, segobs = 0, ptc = 0, segc = 0, opt = 0, oseg = 0, m = 0, f = 0, vis = 0; };
// CSR offsets of k lists over `total` entries: start at 0, never decrease; the last one is the length
static bool cand_csr_ok(const int32_t* off, int k) {
  if (off[0] != 0) return false;
  for (int i = 0; i < k; ++i) if (off[i + 1] < off[i]) return false;
  return true;
}
static bool cand_idx_ok(const int32_t* v, size_t n, int lo, int hi) {   // lo <= v < hi
  for (size_t i = 0; i < n; ++i) if (v[i] < lo || v[i] >= hi) return false;
  return true;
}
}  // namespace

extern "C" int plsvo_candidates_stage(plsvo_ctx* c, int n, const plsvo_cand_map* maps, const plsvo_cand_params* pr) {
  CTX_CHECK(c);
  if (n < 0 || !pr || (n > 0 && !maps)) return fail(c, PLSVO_E_INVALID, "candidates_stage: bad arguments");
  if (pr->cell_size <= 0 || pr->seg_cell_size <= 0 || pr->boundary < 0 || pr->n_pyr_levels < 1 || pr->align_max_iter < 0 || pr->cam.width <= 0 || pr->cam.height <= 0)
    return fail(c, PLSVO_E_INVALID, "candidates_stage: bad parameters");
  CandTotals t;
  int max_level = 0;
  std::vector<CandMapDev> md((size_t)n);
  const plsvo_cand_reserve R = c->ci_reserve;       // room beyond the staged sizes: the offsets below are laid out by capacity
  const plsvo_cand_lm_reserve L = c->cn_reserve;    // landmark rows beyond the staged counts: the per-landmark rows, the candidate lists, the filed rows follow
  std::vector<int> cap((size_t)n * 5), used((size_t)n * 4), lmcap((size_t)n * 4), fetch_cand((size_t)n * 2);
  for (int s = 0; s < n; ++s) {
    const plsvo_cand_map& I = maps[s];
    if (I.n_kf < 0 || I.n_pt < 0 || I.n_seg < 0 || I.n_pt_cand < 0 || I.n_seg_cand < 0) return fail(c, PLSVO_E_INVALID, "candidates_stage: negative count");
    if (I.n_kf > 0 && (!I.kf_T || !I.kf_slot || !I.kf_pt_off || !I.kf_seg_off)) return fail(c, PLSVO_E_INVALID, "candidates_stage: null keyframe table");
    if (I.n_pt > 0 && (!I.pt_pos || !I.pt_type || !I.pt_obs_off)) return fail(c, PLSVO_E_INVALID, "candidates_stage: null point table");
    if (I.n_seg > 0 && (!I.seg_spos || !I.seg_epos || !I.seg_type || !I.seg_obs_off)) return fail(c, PLSVO_E_INVALID, "candidates_stage: null segment table");
    if ((I.n_pt_cand > 0 && !I.pt_cand) || (I.n_seg_cand > 0 && !I.seg_cand)) return fail(c, PLSVO_E_INVALID, "candidates_stage: null candidate list");
    if (I.n_kf > 0 && (!cand_csr_ok(I.kf_pt_off, I.n_kf) || !cand_csr_ok(I.kf_seg_off, I.n_kf))) return fail(c, PLSVO_E_INVALID, "candidates_stage: bad feature list offsets");
    if ((I.n_pt > 0 && !cand_csr_ok(I.pt_obs_off, I.n_pt)) || (I.n_seg > 0 && !cand_csr_ok(I.seg_obs_off, I.n_seg)))
      return fail(c, PLSVO_E_INVALID, "candidates_stage: bad observation list offsets");
    const size_t kfpt = I.n_kf ? (size_t)I.kf_pt_off[I.n_kf] : 0, kfseg = I.n_kf ? (size_t)I.kf_seg_off[I.n_kf] : 0;
    const size_t ptobs = I.n_pt ? (size_t)I.pt_obs_off[I.n_pt] : 0, segobs = I.n_seg ? (size_t)I.seg_obs_off[I.n_seg] : 0;
    if ((kfpt && !I.kf_pt_lm) || (kfseg && !I.kf_seg_lm)) return fail(c, PLSVO_E_INVALID, "candidates_stage: null feature list");
    if (ptobs && (!I.pt_obs_kf || !I.pt_obs_px || !I.pt_obs_f || !I.pt_obs_level || !I.pt_obs_type)) return fail(c, PLSVO_E_INVALID, "candidates_stage: null point observations");
    if (segobs && (!I.seg_obs_kf || !I.seg_obs_spx || !I.seg_obs_epx || !I.seg_obs_sf || !I.seg_obs_ef || !I.seg_obs_level))
      return fail(c, PLSVO_E_INVALID, "candidates_stage: null segment observations");
    if (!cand_idx_ok(I.kf_pt_lm, kfpt, -1, I.n_pt) || !cand_idx_ok(I.kf_seg_lm, kfseg, -1, I.n_seg)) return fail(c, PLSVO_E_INVALID, "candidates_stage: landmark index out of range");
    if (!cand_idx_ok(I.pt_cand, (size_t)I.n_pt_cand, 0, I.n_pt) || !cand_idx_ok(I.seg_cand, (size_t)I.n_seg_cand, 0, I.n_seg))
      return fail(c, PLSVO_E_INVALID, "candidates_stage: candidate index out of range");
    if (!cand_idx_ok(I.pt_obs_kf, ptobs, 0, I.n_kf) || !cand_idx_ok(I.seg_obs_kf, segobs, 0, I.n_kf)) return fail(c, PLSVO_E_INVALID, "candidates_stage: observation keyframe out of range");
    if (!cand_idx_ok(I.pt_type, (size_t)I.n_pt, PLSVO_LM_DELETED, PLSVO_LM_GOOD + 1) || !cand_idx_ok(I.seg_type, (size_t)I.n_seg, PLSVO_LM_DELETED, PLSVO_LM_GOOD + 1))
      return fail(c, PLSVO_E_INVALID, "candidates_stage: unknown landmark type");
    if (!cand_idx_ok(I.kf_slot, (size_t)I.n_kf, 0, INT32_MAX)) return fail(c, PLSVO_E_INVALID, "candidates_stage: negative pyramid slot");
    if (!cand_idx_ok(I.pt_obs_level, ptobs, 0, PLSVO_MAX_LEVELS) || !cand_idx_ok(I.seg_obs_level, segobs, 0, PLSVO_MAX_LEVELS))
      return fail(c, PLSVO_E_INVALID, "candidates_stage: observation level out of range");
    bool edgelet = false;
    for (size_t k = 0; k < ptobs; ++k) {
      if (I.pt_obs_type[k] == PLSVO_FTR_EDGELET) edgelet = true;
      else if (I.pt_obs_type[k] != PLSVO_FTR_CORNER) return fail(c, PLSVO_E_INVALID, "candidates_stage: unknown feature type");
      max_level = std::max(max_level, (int)I.pt_obs_level[k]);
    }
    if (edgelet && !I.pt_obs_grad) return fail(c, PLSVO_E_INVALID, "candidates_stage: edgelets without pt_obs_grad");
    for (size_t k = 0; k < segobs; ++k) max_level = std::max(max_level, (int)I.seg_obs_level[k]);
    CandMapDev& M = md[(size_t)s];
    M.n_kf = I.n_kf; M.n_pt = I.n_pt; M.n_seg = I.n_seg; M.n_pt_cand = I.n_pt_cand; M.n_seg_cand = I.n_seg_cand;
    if ((size_t)I.n_pt + (size_t)I.n_pt_cand + 2 * (size_t)L.extra_pt > (size_t)INT32_MAX || (size_t)I.n_seg + (size_t)I.n_seg_cand + 2 * (size_t)L.extra_seg > (size_t)INT32_MAX)
      return fail(c, PLSVO_E_CAPACITY, "candidates_stage: stream too large");
    int* lc = lmcap.data() + 4 * (size_t)s;
    lc[0] = I.n_pt + L.extra_pt; lc[1] = I.n_seg + L.extra_seg; lc[2] = I.n_pt_cand + L.extra_pt; lc[3] = I.n_seg_cand + L.extra_seg;
    fetch_cand[2 * (size_t)s] = I.n_pt_cand; fetch_cand[2 * (size_t)s + 1] = I.n_seg_cand;
    M.cap_pt = lc[0] + lc[2]; M.cap_seg = lc[1] + lc[3]; M.stream = s;   // (what the candidate kernel switches off behind the filed entries: the rows as laid out)
    M.kf_off = (long long)t.kf; M.kfpt_off = (long long)t.kfpt; M.kfseg_off = (long long)t.kfseg; M.pt_off = (long long)t.pt; M.seg_off = (long long)t.seg;
    M.ptobs_off = (long long)t.ptobs; M.segobs_off = (long long)t.segobs; M.ptc_off = (long long)t.ptc; M.segc_off = (long long)t.segc;
    M.opt_off = (long long)t.opt; M.oseg_off = (long long)t.oseg; M.m_off = (long long)t.m; M.f_off = (long long)t.f;
    M.vis_pt_off = (long long)t.vis; t.vis += ((size_t)lc[0] + 63) & ~(size_t)63;
    M.vis_seg_off = (long long)t.vis; t.vis += ((size_t)lc[1] + 63) & ~(size_t)63;
    if (kfpt + (size_t)R.extra_kf_pt > (size_t)INT32_MAX || kfseg + (size_t)R.extra_kf_seg > (size_t)INT32_MAX || ptobs + (size_t)R.extra_pt_obs > (size_t)INT32_MAX ||
        segobs + (size_t)R.extra_seg_obs > (size_t)INT32_MAX || (size_t)I.n_kf + (size_t)R.extra_kf > (size_t)INT32_MAX) return fail(c, PLSVO_E_CAPACITY, "candidates_stage: stream too large");
    int* cp = cap.data() + 5 * (size_t)s; int* us = used.data() + 4 * (size_t)s;
    cp[0] = I.n_kf + R.extra_kf; cp[1] = (int)kfpt + R.extra_kf_pt; cp[2] = (int)kfseg + R.extra_kf_seg; cp[3] = (int)ptobs + R.extra_pt_obs; cp[4] = (int)segobs + R.extra_seg_obs;
    us[0] = (int)kfpt; us[1] = (int)kfseg; us[2] = (int)ptobs; us[3] = (int)segobs;
    t.kf += (size_t)cp[0]; t.kfpt += (size_t)cp[1]; t.kfseg += (size_t)cp[2]; t.pt += (size_t)lc[0]; t.seg += (size_t)lc[1]; t.ptobs += (size_t)cp[3]; t.segobs += (size_t)cp[4];
    t.ptc += (size_t)lc[2]; t.segc += (size_t)lc[3]; t.opt += (size_t)M.cap_pt; t.oseg += (size_t)M.cap_seg;
    t.m += (size_t)M.cap_pt + 2 * (size_t)M.cap_seg; t.f += (size_t)cp[0] + 1;
  }
  if (t.m > (size_t)INT32_MAX || t.f > (size_t)INT32_MAX || t.vis > (size_t)INT32_MAX) return fail(c, PLSVO_E_CAPACITY, "candidates_stage: batch too large");
  c->cd_staged = false; c->cd_ran = false; c->cd_matched = false; c->cs_selected = false; c->cs_posed = false; c->ci_inserted = false; c->ci_have_out = false;
  c->cn_closed = false; c->cn_have_out = false;
  c->ci_cap = std::move(cap); c->ci_used = std::move(used); c->cn_cap = std::move(lmcap); c->cd_fetch_cand = std::move(fetch_cand);
  c->ci_t_kf = t.kf; c->ci_t_kfpt = t.kfpt; c->ci_t_kfseg = t.kfseg; c->ci_t_ptobs = t.ptobs; c->ci_t_segobs = t.segobs;
  if (n == 0) { c->cd_n = 0; c->cd_staged = true; c->cd_maps.clear(); c->cd_m_off.clear(); c->cd_f_off.clear(); c->cd_params = *pr; return PLSVO_OK; }
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t N = (size_t)n;
  Blob blob;
  const size_t b_maps = blob.add(md);
  const size_t b_kfT = blob.reserve<double>(t.kf * 7), b_kfpo = blob.reserve<int>(t.kf + N), b_kfpl = blob.reserve<int>(t.kfpt), b_kfso = blob.reserve<int>(t.kf + N),
               b_kfsl = blob.reserve<int>(t.kfseg);
  const size_t b_ppos = blob.reserve<double>(t.pt * 3), b_ptype = blob.reserve<int>(t.pt), b_pobo = blob.reserve<int>(t.pt + N), b_pokf = blob.reserve<int>(t.ptobs),
               b_popx = blob.reserve<double>(t.ptobs * 2), b_pof = blob.reserve<double>(t.ptobs * 3), b_polv = blob.reserve<int>(t.ptobs),
               b_poty = blob.reserve<uint8_t>(t.ptobs), b_pogr = blob.reserve<double>(t.ptobs * 2);
  const size_t b_sspos = blob.reserve<double>(t.seg * 3), b_sepos = blob.reserve<double>(t.seg * 3), b_stype = blob.reserve<int>(t.seg), b_sobo = blob.reserve<int>(t.seg + N),
               b_sokf = blob.reserve<int>(t.segobs), b_sospx = blob.reserve<double>(t.segobs * 2), b_soepx = blob.reserve<double>(t.segobs * 2),
               b_sosf = blob.reserve<double>(t.segobs * 3), b_soef = blob.reserve<double>(t.segobs * 3), b_solv = blob.reserve<int>(t.segobs);
  const size_t b_ptc = blob.reserve<int>(t.ptc), b_segc = blob.reserve<int>(t.segc), b_fT = blob.reserve<double>(t.f * 7), b_fslot = blob.reserve<int>(t.f);
  auto put = [&](size_t sec, size_t at, const void* src, size_t count, size_t elem) {
    if (count) { if (src) memcpy(blob.host.data() + sec + at * elem, src, count * elem); else memset(blob.host.data() + sec + at * elem, 0, count * elem); }
  };
  c->cd_kf_slot.assign(t.kf, 0);
  c->cd_m_off.resize(N); c->cd_f_off.resize(N);
  for (int s = 0; s < n; ++s) {
    const plsvo_cand_map& I = maps[s];
    const CandMapDev& M = md[(size_t)s];
    const size_t nk = (size_t)I.n_kf, np = (size_t)I.n_pt, ns = (size_t)I.n_seg;
    const size_t kfpt = nk ? (size_t)I.kf_pt_off[nk] : 0, kfseg = nk ? (size_t)I.kf_seg_off[nk] : 0, ptobs = np ? (size_t)I.pt_obs_off[np] : 0, segobs = ns ? (size_t)I.seg_obs_off[ns] : 0;
    const size_t S = (size_t)s;
    put(b_kfT, (size_t)M.kf_off * 7, I.kf_T, nk * 7, sizeof(double));
    put(b_kfpo, (size_t)M.kf_off + S, nk ? I.kf_pt_off : nullptr, nk + 1, sizeof(int));
    put(b_kfso, (size_t)M.kf_off + S, nk ? I.kf_seg_off : nullptr, nk + 1, sizeof(int));
    put(b_kfpl, (size_t)M.kfpt_off, I.kf_pt_lm, kfpt, sizeof(int)); put(b_kfsl, (size_t)M.kfseg_off, I.kf_seg_lm, kfseg, sizeof(int));
    put(b_ppos, (size_t)M.pt_off * 3, I.pt_pos, np * 3, sizeof(double)); put(b_ptype, (size_t)M.pt_off, I.pt_type, np, sizeof(int));
    put(b_pobo, (size_t)M.pt_off + S, np ? I.pt_obs_off : nullptr, np + 1, sizeof(int));
    put(b_pokf, (size_t)M.ptobs_off, I.pt_obs_kf, ptobs, sizeof(int)); put(b_popx, (size_t)M.ptobs_off * 2, I.pt_obs_px, ptobs * 2, sizeof(double));
    put(b_pof, (size_t)M.ptobs_off * 3, I.pt_obs_f, ptobs * 3, sizeof(double)); put(b_polv, (size_t)M.ptobs_off, I.pt_obs_level, ptobs, sizeof(int));
    put(b_poty, (size_t)M.ptobs_off, I.pt_obs_type, ptobs, 1); put(b_pogr, (size_t)M.ptobs_off * 2, I.pt_obs_grad, ptobs * 2, sizeof(double));
    put(b_sspos, (size_t)M.seg_off * 3, I.seg_spos, ns * 3, sizeof(double)); put(b_sepos, (size_t)M.seg_off * 3, I.seg_epos, ns * 3, sizeof(double));
    put(b_stype, (size_t)M.seg_off, I.seg_type, ns, sizeof(int)); put(b_sobo, (size_t)M.seg_off + S, ns ? I.seg_obs_off : nullptr, ns + 1, sizeof(int));
    put(b_sokf, (size_t)M.segobs_off, I.seg_obs_kf, segobs, sizeof(int));
    put(b_sospx, (size_t)M.segobs_off * 2, I.seg_obs_spx, segobs * 2, sizeof(double)); put(b_soepx, (size_t)M.segobs_off * 2, I.seg_obs_epx, segobs * 2, sizeof(double));
    put(b_sosf, (size_t)M.segobs_off * 3, I.seg_obs_sf, segobs * 3, sizeof(double)); put(b_soef, (size_t)M.segobs_off * 3, I.seg_obs_ef, segobs * 3, sizeof(double));
    put(b_solv, (size_t)M.segobs_off, I.seg_obs_level, segobs, sizeof(int));
    put(b_ptc, (size_t)M.ptc_off, I.pt_cand, (size_t)I.n_pt_cand, sizeof(int)); put(b_segc, (size_t)M.segc_off, I.seg_cand, (size_t)I.n_seg_cand, sizeof(int));
    // the matcher's frame table: the keyframes; the new frame's entry (identity until a run writes it)
    put(b_fT, (size_t)M.f_off * 7, I.kf_T, nk * 7, sizeof(double)); put(b_fslot, (size_t)M.f_off, I.kf_slot, nk, sizeof(int));
    const double ident[7] = { 0, 0, 0, 1, 0, 0, 0 };
    put(b_fT, ((size_t)M.f_off + nk) * 7, ident, 7, sizeof(double)); put(b_fslot, (size_t)M.f_off + nk, nullptr, 1, sizeof(int));
    if (nk) memcpy(c->cd_kf_slot.data() + M.kf_off, I.kf_slot, nk * sizeof(int));
    c->cd_m_off[S] = M.m_off; c->cd_f_off[S] = M.f_off;
  }
  int rc;
  if ((rc = upload_blob(c, c->cd_d_blob, blob))) return rc;
  c->cd_blob_bytes = blob.host.size();
  // device work: results first (what a fetch brings back), then scratch, then the matcher's arrays and its results
  Carver cv;
  const size_t w_cnt = cv.take<int>(N * 2), w_plm = cv.take<int>(t.opt), w_ppx = cv.take<double>(t.opt * 2), w_pcell = cv.take<int>(t.opt), w_pobs = cv.take<int>(t.opt),
               w_pview = cv.take<uint8_t>(t.opt), w_pact = cv.take<uint8_t>(t.opt), w_slm = cv.take<int>(t.oseg), w_spx = cv.take<double>(t.oseg * 4),
               w_scell = cv.take<int>(t.oseg * 2), w_sobs = cv.take<int>(t.oseg), w_sview = cv.take<uint8_t>(t.oseg), w_sact = cv.take<uint8_t>(t.oseg),
               w_pfail = cv.take<uint8_t>(t.ptc), w_sfail = cv.take<uint8_t>(t.segc);
  c->cd_fetch_bytes = cv.off;
  const size_t w_vis = cv.take<unsigned int>(t.vis), w_kfpos = cv.take<double>(t.kf * 3), w_tplm = cv.take<int>(t.opt), w_tppx = cv.take<double>(t.opt * 2),
               w_tpcell = cv.take<int>(t.opt), w_tslm = cv.take<int>(t.oseg), w_tspx = cv.take<double>(t.oseg * 4), w_tscell = cv.take<int>(t.oseg * 2);
  const size_t w_mcf = cv.take<int>(t.m), w_mrf = cv.take<int>(t.m), w_mrpx = cv.take<double>(t.m * 2), w_mrf3 = cv.take<double>(t.m * 3), w_mlv = cv.take<int>(t.m),
               w_mty = cv.take<uint8_t>(t.m), w_mgr = cv.take<double>(t.m * 2), w_mpos = cv.take<double>(t.m * 3), w_mpx = cv.take<double>(t.m * 2), w_mact = cv.take<uint8_t>(t.m);
  const size_t w_opx = cv.take<double>(t.m * 2), w_olev = cv.take<int>(t.m), w_oit = cv.take<int>(t.m), w_ofound = cv.take<uint8_t>(t.m);
  HIP_TRY(c, c->cd_d_work.ensure(cv.off + 256));
  char* din = reinterpret_cast<char*>(c->cd_d_blob.p); char* dw = reinterpret_cast<char*>(c->cd_d_work.p);
  auto D = [&](size_t o) { return reinterpret_cast<double*>(din + o); };
  auto Iv = [&](size_t o) { return reinterpret_cast<int*>(din + o); };
  auto WD = [&](size_t o) { return reinterpret_cast<double*>(dw + o); };
  auto WI = [&](size_t o) { return reinterpret_cast<int*>(dw + o); };
  auto WB = [&](size_t o) { return reinterpret_cast<uint8_t*>(dw + o); };
  CandBatchDev b{};
  b.maps = reinterpret_cast<const CandMapDev*>(din + b_maps); b.n_jobs = n;
  b.fx = pr->cam.fx; b.fy = pr->cam.fy; b.cx = pr->cam.cx; b.cy = pr->cam.cy; b.cam_width = pr->cam.width; b.cam_height = pr->cam.height;
  b.cell_size = pr->cell_size; b.grid_n_cols = (pr->cam.width + pr->cell_size - 1) / pr->cell_size;
  b.seg_cell_size = pr->seg_cell_size; b.seg_grid_n_cols = (pr->cam.width + pr->seg_cell_size - 1) / pr->seg_cell_size; b.boundary = pr->boundary;
  b.kf_T = D(b_kfT); b.kf_pt_off = Iv(b_kfpo); b.kf_pt_lm = Iv(b_kfpl); b.kf_seg_off = Iv(b_kfso); b.kf_seg_lm = Iv(b_kfsl);
  b.pt_pos = D(b_ppos); b.pt_type = Iv(b_ptype); b.pt_obs_off = Iv(b_pobo); b.pt_obs_kf = Iv(b_pokf); b.pt_obs_px = D(b_popx); b.pt_obs_f = D(b_pof);
  b.pt_obs_level = Iv(b_polv); b.pt_obs_type = reinterpret_cast<const uint8_t*>(din + b_poty); b.pt_obs_grad = D(b_pogr);
  b.seg_spos = D(b_sspos); b.seg_epos = D(b_sepos); b.seg_type = Iv(b_stype); b.seg_obs_off = Iv(b_sobo); b.seg_obs_kf = Iv(b_sokf);
  b.seg_obs_spx = D(b_sospx); b.seg_obs_epx = D(b_soepx); b.seg_obs_sf = D(b_sosf); b.seg_obs_ef = D(b_soef); b.seg_obs_level = Iv(b_solv);
  b.pt_cand = Iv(b_ptc); b.seg_cand = Iv(b_segc);
  b.visit = reinterpret_cast<unsigned int*>(dw + w_vis); b.kf_pos = WD(w_kfpos);
  b.t_pt_lm = WI(w_tplm); b.t_pt_px = WD(w_tppx); b.t_pt_cell = WI(w_tpcell); b.t_seg_lm = WI(w_tslm); b.t_seg_px = WD(w_tspx); b.t_seg_cell = WI(w_tscell);
  b.counts = WI(w_cnt);
  b.o_pt_lm = WI(w_plm); b.o_pt_px = WD(w_ppx); b.o_pt_cell = WI(w_pcell); b.o_pt_obs = WI(w_pobs); b.o_pt_view = WB(w_pview); b.o_pt_active = WB(w_pact);
  b.o_seg_lm = WI(w_slm); b.o_seg_px = WD(w_spx); b.o_seg_cell = WI(w_scell); b.o_seg_obs = WI(w_sobs); b.o_seg_view = WB(w_sview); b.o_seg_active = WB(w_sact);
  b.pt_cand_failed = WB(w_pfail); b.seg_cand_failed = WB(w_sfail);
  b.frame_T = D(b_fT); b.frame_slot = Iv(b_fslot);
  b.m_cur_frame = WI(w_mcf); b.m_ref_frame = WI(w_mrf); b.m_ref_px = WD(w_mrpx); b.m_ref_f = WD(w_mrf3); b.m_ref_level = WI(w_mlv); b.m_ref_type = WB(w_mty);
  b.m_ref_grad = WD(w_mgr); b.m_pos = WD(w_mpos); b.m_px_cur = WD(w_mpx); b.m_active = WB(w_mact);
  c->cd_b = b;
  MatchBatchDev mb{};
  mb.fx = b.fx; mb.fy = b.fy; mb.cx = b.cx; mb.cy = b.cy; mb.cam_width = b.cam_width; mb.cam_height = b.cam_height;
  mb.n = (int)t.m; mb.n_pyr_levels = pr->n_pyr_levels; mb.align_max_iter = pr->align_max_iter;
  mb.frame_T = b.frame_T; mb.frame_slot = b.frame_slot; mb.cur_frame = b.m_cur_frame; mb.ref_frame = b.m_ref_frame;
  mb.ref_px = b.m_ref_px; mb.ref_f = b.m_ref_f; mb.ref_level = b.m_ref_level; mb.ref_type = b.m_ref_type; mb.ref_grad = b.m_ref_grad;
  mb.pos = b.m_pos; mb.px_cur = b.m_px_cur; mb.active = b.m_active;
  mb.px_out = WD(w_opx); mb.search_level = WI(w_olev); mb.n_iter = WI(w_oit); mb.found = WB(w_ofound);
  c->cd_match = mb;
  c->cd_off = { w_cnt, w_plm, w_ppx, w_pcell, w_pobs, w_pview, w_pact, w_slm, w_spx, w_scell, w_sobs, w_sview, w_sact, w_pfail, w_sfail };
  c->cd_vis_off = w_vis; c->cd_vis_bytes = t.vis * sizeof(unsigned int);
  c->cd_maps = std::move(md); c->cd_params = *pr; c->cd_n = n; c->cd_total_m = t.m; c->cd_total_f = t.f; c->cd_max_level = max_level;
  // the landmark quality the selection maintains: n_failed_reproj_, n_succeeded_reproj_ of points and segments, then their event bytes -- zero
  {
    Carver q;
    q.take<int>(t.pt); q.take<int>(t.pt); q.take<int>(t.seg); q.take<int>(t.seg);
    c->cs_ev_off = q.take<uint8_t>(t.pt); q.take<uint8_t>(t.seg);
    HIP_TRY(c, c->cs_d_q.ensure(q.off + 256));
    HIP_TRY(c, hipMemsetAsync(c->cs_d_q.p, 0, q.off, c->stream));
  }
  c->cd_t_pt = t.pt; c->cd_t_seg = t.seg; c->cd_t_ptc = t.ptc; c->cd_t_segc = t.segc; c->cd_t_opt = t.opt; c->cd_t_oseg = t.oseg;
  c->cd_staged = true;
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_run(plsvo_ctx* c, int n, const plsvo_cand_frame* fr) {
  CTX_CHECK(c);
  if (!c->cd_staged) return fail(c, PLSVO_E_STATE, "candidates_run: no staged map tables");
  if (n != c->cd_n || (n > 0 && !fr)) return fail(c, PLSVO_E_INVALID, "candidates_run: n does not match the staged batch");
  size_t t_ov = 0;
  for (int s = 0; s < n; ++s) {
    if (fr[s].n_overlap < 0 || fr[s].cur_slot < 0) return fail(c, PLSVO_E_INVALID, "candidates_run: negative count or slot");
    if (fr[s].n_overlap > 0 && !fr[s].overlap_idx) return fail(c, PLSVO_E_INVALID, "candidates_run: null overlap list");
    if (!cand_idx_ok(fr[s].overlap_idx, (size_t)fr[s].n_overlap, 0, c->cd_maps[(size_t)s].n_kf)) return fail(c, PLSVO_E_INVALID, "candidates_run: overlap index outside the keyframe table");
    t_ov += (size_t)fr[s].n_overlap;
  }
  c->cd_ran = false; c->cd_matched = false; c->cs_selected = false; c->cs_posed = false; c->ci_inserted = false; c->cn_closed = false;
  for (int s = 0; s < n; ++s) { c->cd_fetch_cand[2 * (size_t)s] = c->cd_maps[(size_t)s].n_pt_cand; c->cd_fetch_cand[2 * (size_t)s + 1] = c->cd_maps[(size_t)s].n_seg_cand; }
  c->cd_ov_off.assign((size_t)n + 1, 0);
  if (n == 0) { c->cd_ran = true; return PLSVO_OK; }
  HIP_TRY(c, hipSetDevice(c->device));
  Blob blob;
  const size_t b_jobs = blob.reserve<CandJobDev>((size_t)n), b_ov = blob.reserve<int>(t_ov);
  CandJobDev* jobs = blob.at<CandJobDev>(b_jobs); int* ov = blob.at<int>(b_ov);
  c->cd_cur_slot.resize((size_t)n);
  size_t o = 0;
  for (int s = 0; s < n; ++s) {
    CandJobDev& J = jobs[s];
    memcpy(J.T, fr[s].T_f_w, sizeof(J.T)); J.d_T = fr[s].d_T_f_w; J.cur_slot = fr[s].cur_slot; J.n_ov = fr[s].n_overlap; J.ov_off = (long long)o;
    if (J.n_ov) memcpy(ov + o, fr[s].overlap_idx, (size_t)J.n_ov * sizeof(int));
    c->cd_cur_slot[(size_t)s] = fr[s].cur_slot; c->cd_ov_off[(size_t)s] = (long long)o;
    o += (size_t)J.n_ov;
  }
  c->cd_ov_off[(size_t)n] = (long long)o;
  int rc;
  if ((rc = upload_blob(c, c->cd_d_run, blob))) return rc;
  HIP_TRY(c, c->cd_d_kfcount.ensure(std::max(t_ov, (size_t)1) * sizeof(int)));
  CandBatchDev b = c->cd_b;
  const char* dr = reinterpret_cast<const char*>(c->cd_d_run.p);
  b.jobs = reinterpret_cast<const CandJobDev*>(dr + b_jobs); b.overlap_idx = reinterpret_cast<const int*>(dr + b_ov); b.kf_count = c->cd_d_kfcount.as<int>();
  {
    EventPair ep{}; prof_begin(c, PLSVO_K_CANDIDATES, &ep);
    // the first-visit words are all ones ahead of EVERY launch: a run must not see the visits of the one before
    hipError_t rearm_then_launch = hipSuccess;
    if (c->cd_vis_bytes) rearm_then_launch = hipMemsetAsync(reinterpret_cast<char*>(c->cd_d_work.p) + c->cd_vis_off, 0xff, c->cd_vis_bytes, c->stream);
    if (rearm_then_launch == hipSuccess) rearm_then_launch = launch_map_candidates(b, c->stream);
    prof_end(c, PLSVO_K_CANDIDATES, &ep);            // ahead of the error return: the event pair goes back to the pool either way
    HIP_TRY(c, rearm_then_launch);
  }
  c->cd_ran = true;
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_fetch(plsvo_ctx* c, int n, plsvo_cand_out* out) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->cd_ran) return fail(c, PLSVO_E_STATE, "candidates_fetch: no run to fetch");
  if (n != c->cd_n || (n > 0 && !out)) return fail(c, PLSVO_E_INVALID, "candidates_fetch: n does not match the staged batch");
  if (n == 0) return PLSVO_OK;
  std::vector<char> h(c->cd_fetch_bytes);
  const size_t t_ov = (size_t)c->cd_ov_off[(size_t)n];
  std::vector<int> kfc(std::max(t_ov, (size_t)1));
  HIP_TRY(c, hipMemcpyAsync(h.data(), c->cd_d_work.p, h.size(), hipMemcpyDeviceToHost, c->stream));
  if (t_ov) HIP_TRY(c, hipMemcpyAsync(kfc.data(), c->cd_d_kfcount.p, t_ov * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const size_t* W = c->cd_off.data();
  const int* cnt = reinterpret_cast<const int*>(h.data() + W[0]);
  auto cp = [&](void* dst, size_t sec, size_t at, size_t count, size_t elem) { if (dst && count) memcpy(dst, h.data() + sec + at * elem, count * elem); };
  for (int s = 0; s < n; ++s) {
    const CandMapDev& M = c->cd_maps[(size_t)s];
    plsvo_cand_out& O = out[s];
    const size_t np = (size_t)cnt[2 * s], ns = (size_t)cnt[2 * s + 1], po = (size_t)M.opt_off, so = (size_t)M.oseg_off;
    O.n_filed_pt = (int32_t)np; O.n_filed_seg = (int32_t)ns;
    cp(O.pt_lm, W[1], po, np, sizeof(int)); cp(O.pt_px, W[2], po * 2, np * 2, sizeof(double)); cp(O.pt_cell, W[3], po, np, sizeof(int));
    cp(O.pt_obs, W[4], po, np, sizeof(int)); cp(O.pt_has_view, W[5], po, np, 1); cp(O.pt_active, W[6], po, np, 1);
    cp(O.seg_lm, W[7], so, ns, sizeof(int)); cp(O.seg_px, W[8], so * 4, ns * 4, sizeof(double)); cp(O.seg_cell, W[9], so * 2, ns * 2, sizeof(int));
    cp(O.seg_obs, W[10], so, ns, sizeof(int)); cp(O.seg_has_view, W[11], so, ns, 1); cp(O.seg_active, W[12], so, ns, 1);
    cp(O.pt_cand_failed, W[13], (size_t)M.ptc_off, (size_t)c->cd_fetch_cand[2 * (size_t)s], 1); cp(O.seg_cand_failed, W[14], (size_t)M.segc_off, (size_t)c->cd_fetch_cand[2 * (size_t)s + 1], 1);
    const size_t a = (size_t)c->cd_ov_off[(size_t)s], e = (size_t)c->cd_ov_off[(size_t)s + 1];
    if (O.kf_count && e > a) memcpy(O.kf_count, kfc.data() + a, (e - a) * sizeof(int));
  }
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_match(plsvo_ctx* c) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->cd_ran) return fail(c, PLSVO_E_STATE, "candidates_match: no candidates on the device");
  if (c->ci_inserted) return fail(c, PLSVO_E_STATE, "candidates_match: this run's frame was inserted (the tables have moved on); run again");
  if (c->cn_closed) return fail(c, PLSVO_E_STATE, "candidates_match: landmarks were added behind this run (the tables have moved on); run again");
  if (c->cd_n == 0 || c->cd_total_m == 0) { c->cd_matched = true; return PLSVO_OK; }
  if (!c->pyr.base) return fail(c, PLSVO_E_STATE, "candidates_match: pyramids not configured");
  const plsvo_cand_params& pr = c->cd_params;
  if (pr.n_pyr_levels > c->pyr.n_levels) return fail(c, PLSVO_E_INVALID, "candidates_match: n_pyr_levels exceeds the configured pyramid");
  if (pr.cam.width != c->pyr.w[0] || pr.cam.height != c->pyr.h[0]) return fail(c, PLSVO_E_INVALID, "candidates_match: camera size does not match the configured pyramid");
  if (c->cd_max_level >= c->pyr.n_levels) return fail(c, PLSVO_E_CAPACITY, "candidates_match: observation level outside the configured pyramid");
  for (int v : c->cd_kf_slot) if (v >= c->pyr.n_slots) return fail(c, PLSVO_E_CAPACITY, "candidates_match: pyramid slot out of range");
  for (int v : c->cd_cur_slot) if (v >= c->pyr.n_slots) return fail(c, PLSVO_E_CAPACITY, "candidates_match: pyramid slot out of range");
  HIP_TRY(c, hipSetDevice(c->device));
  MatchBatchDev mb = c->cd_match;
  mb.pyr_base = c->pyr.base; mb.slot_bytes = c->pyr.slot_bytes; mb.width = c->pyr.w[0]; mb.height = c->pyr.h[0];
  {
    EventPair ep{}; prof_begin(c, PLSVO_K_MATCH, &ep);
    const hipError_t launched = launch_match_direct(mb, c->stream);
    prof_end(c, PLSVO_K_MATCH, &ep);                 // ahead of the error return, as in plsvo_candidates_run
    HIP_TRY(c, launched);
  }
  c->cd_matched = true;
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_match_fetch(plsvo_ctx* c, int n, plsvo_cand_match_out* out) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->cd_ran || !c->cd_matched) return fail(c, PLSVO_E_STATE, "candidates_match_fetch: no match to fetch");
  if (n != c->cd_n || (n > 0 && !out)) return fail(c, PLSVO_E_INVALID, "candidates_match_fetch: n does not match the staged batch");
  if (n == 0 || c->cd_total_m == 0) return PLSVO_OK;
  const size_t NM = c->cd_total_m;
  std::vector<int> cnt((size_t)n * 2), lev(NM);
  std::vector<double> px(NM * 2);
  std::vector<uint8_t> found(NM);
  const MatchBatchDev& mb = c->cd_match;
  HIP_TRY(c, hipMemcpyAsync(cnt.data(), c->cd_b.counts, cnt.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(px.data(), mb.px_out, NM * 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(lev.data(), mb.search_level, NM * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(found.data(), mb.found, NM, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int s = 0; s < n; ++s) {
    const size_t at = (size_t)c->cd_maps[(size_t)s].m_off, k = (size_t)cnt[2 * s] + 2 * (size_t)cnt[2 * s + 1];
    if (!k) continue;
    if (out[s].found) memcpy(out[s].found, found.data() + at, k);
    if (out[s].px) memcpy(out[s].px, px.data() + 2 * at, k * 2 * sizeof(double));
    if (out[s].search_level) memcpy(out[s].search_level, lev.data() + at, k * sizeof(int));
  }
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_dev(plsvo_ctx* c, plsvo_cand_dev* o) {
  CTX_CHECK(c);
  if (!o) return fail(c, PLSVO_E_INVALID, "candidates_dev: bad arguments");
  if (!c->cd_staged || !c->cd_ran || c->cd_n == 0 || c->ci_inserted || c->cn_closed) return fail(c, PLSVO_E_STATE, "candidates_dev: no candidates on the device");
  const CandBatchDev& b = c->cd_b; const MatchBatchDev& mb = c->cd_match;
  o->n_entries = (int64_t)c->cd_total_m; o->n_frames = (int64_t)c->cd_total_f;
  o->m_off = c->cd_m_off.data(); o->f_off = c->cd_f_off.data();
  o->d_counts = b.counts; o->d_frame_T = b.frame_T; o->d_frame_slot = b.frame_slot; o->d_cur_frame = b.m_cur_frame; o->d_ref_frame = b.m_ref_frame;
  o->d_ref_px = b.m_ref_px; o->d_ref_f = b.m_ref_f; o->d_ref_level = b.m_ref_level; o->d_ref_type = b.m_ref_type; o->d_ref_grad = b.m_ref_grad;
  o->d_pos = b.m_pos; o->d_px_cur = b.m_px_cur; o->d_active = b.m_active;
  o->d_found = mb.found; o->d_px_out = mb.px_out; o->d_search_level = mb.search_level;
  return PLSVO_OK;
}

// ---- cell selection of the map candidates: one per cell, landmark quality, features, pose-optimiser input (select_device.hpp) ---------
namespace {
constexpr int kInsJoinedBit = 32;                  // insert_device.hpp's kInsJoined
constexpr int kNewCandBit = 64;                    // newcand_device.hpp's kNewCand
// the sections of cs_d_q, as plsvo_candidates_stage carved them
struct QualitySections { size_t pt_nf, pt_ns, seg_nf, seg_ns, pt_ev, seg_ev, end; };
static QualitySections quality_sections(const plsvo_ctx* c) {
  Carver q; QualitySections s;
  s.pt_nf = q.take<int>(c->cd_t_pt); s.pt_ns = q.take<int>(c->cd_t_pt); s.seg_nf = q.take<int>(c->cd_t_seg); s.seg_ns = q.take<int>(c->cd_t_seg);
  s.pt_ev = q.take<uint8_t>(c->cd_t_pt); s.seg_ev = q.take<uint8_t>(c->cd_t_seg); s.end = q.off;
  return s;
}
// order (visit position -> cell) and its inverse, appended to v; false when `order` is no permutation of 0 .. n-1
static bool append_cell_order(std::vector<int>& v, const int32_t* order, int n) {
  const size_t at = v.size();
  v.resize(at + 2 * (size_t)n, -1);
  for (int k = 0; k < n; ++k) {
    const int cell = order ? order[k] : k;
    if (cell < 0 || cell >= n || v[at + (size_t)n + (size_t)cell] != -1) return false;
    v[at + (size_t)k] = cell; v[at + (size_t)n + (size_t)cell] = k;
  }
  return true;
}
}  // namespace

extern "C" int plsvo_candidates_set_quality(plsvo_ctx* c, int n, const plsvo_cand_quality_in* in) {
  CTX_CHECK(c);
  if (!c->cd_staged) return fail(c, PLSVO_E_STATE, "candidates_set_quality: no staged map tables");
  if (n != c->cd_n || (n > 0 && !in)) return fail(c, PLSVO_E_INVALID, "candidates_set_quality: n does not match the staged batch");
  for (int s = 0; s < n; ++s) {
    const CandMapDev& M = c->cd_maps[(size_t)s];
    const int32_t* arr[4] = { in[s].pt_n_failed, in[s].pt_n_succeeded, in[s].seg_n_failed, in[s].seg_n_succeeded };
    for (int a = 0; a < 4; ++a) if (arr[a] && !cand_idx_ok(arr[a], (size_t)(a < 2 ? M.n_pt : M.n_seg), 0, INT32_MAX)) return fail(c, PLSVO_E_INVALID, "candidates_set_quality: negative counter");
  }
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const QualitySections q = quality_sections(c);
  const size_t sec[4] = { q.pt_nf, q.pt_ns, q.seg_nf, q.seg_ns };
  char* d = reinterpret_cast<char*>(c->cs_d_q.p);
  for (int s = 0; s < n; ++s) {
    const CandMapDev& M = c->cd_maps[(size_t)s];
    const int32_t* arr[4] = { in[s].pt_n_failed, in[s].pt_n_succeeded, in[s].seg_n_failed, in[s].seg_n_succeeded };
    for (int a = 0; a < 4; ++a) {
      const size_t cnt = (size_t)(a < 2 ? M.n_pt : M.n_seg), at = (size_t)(a < 2 ? M.pt_off : M.seg_off);
      if (arr[a] && cnt) HIP_TRY(c, hipMemcpyAsync(d + sec[a] + at * sizeof(int), arr[a], cnt * sizeof(int), hipMemcpyHostToDevice, c->stream));
    }
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // the caller's arrays are free again
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_fetch_quality(plsvo_ctx* c, int n, plsvo_cand_quality_out* out) {
  CTX_CHECK(c);
  if (!c->cd_staged) return fail(c, PLSVO_E_STATE, "candidates_fetch_quality: no staged map tables");
  if (n != c->cd_n || (n > 0 && !out)) return fail(c, PLSVO_E_INVALID, "candidates_fetch_quality: n does not match the staged batch");
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const QualitySections q = quality_sections(c);
  const CandBatchDev& b = c->cd_b;
  std::vector<char> hq(q.end);
  std::vector<CandMapDev> maps((size_t)n);
  std::vector<int> ptype(std::max(c->cd_t_pt, (size_t)1)), stype(std::max(c->cd_t_seg, (size_t)1)), ptc(std::max(c->cd_t_ptc, (size_t)1)), segc(std::max(c->cd_t_segc, (size_t)1));
  HIP_TRY(c, hipMemcpyAsync(hq.data(), c->cs_d_q.p, q.end, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(maps.data(), b.maps, (size_t)n * sizeof(CandMapDev), hipMemcpyDeviceToHost, c->stream));
  if (c->cd_t_pt) HIP_TRY(c, hipMemcpyAsync(ptype.data(), b.pt_type, c->cd_t_pt * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (c->cd_t_seg) HIP_TRY(c, hipMemcpyAsync(stype.data(), b.seg_type, c->cd_t_seg * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (c->cd_t_ptc) HIP_TRY(c, hipMemcpyAsync(ptc.data(), b.pt_cand, c->cd_t_ptc * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (c->cd_t_segc) HIP_TRY(c, hipMemcpyAsync(segc.data(), b.seg_cand, c->cd_t_segc * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  auto cp = [&](void* dst, const void* src, size_t at, size_t count, size_t elem) { if (dst && count) memcpy(dst, reinterpret_cast<const char*>(src) + at * elem, count * elem); };
  for (int s = 0; s < n; ++s) {
    const CandMapDev& M = maps[(size_t)s];
    plsvo_cand_quality_out& O = out[s];
    const size_t np = (size_t)M.n_pt, ns = (size_t)M.n_seg, po = (size_t)M.pt_off, so = (size_t)M.seg_off;
    O.n_pt_cand = M.n_pt_cand; O.n_seg_cand = M.n_seg_cand;
    cp(O.pt_n_failed, hq.data() + q.pt_nf, po, np, sizeof(int)); cp(O.pt_n_succeeded, hq.data() + q.pt_ns, po, np, sizeof(int));
    cp(O.seg_n_failed, hq.data() + q.seg_nf, so, ns, sizeof(int)); cp(O.seg_n_succeeded, hq.data() + q.seg_ns, so, ns, sizeof(int));
    cp(O.pt_type, ptype.data(), po, np, sizeof(int)); cp(O.seg_type, stype.data(), so, ns, sizeof(int));
    // (the insertion's bit sits above the selection's internal ones)
    auto public_event = [](char ev) { return (uint8_t)((ev & (PLSVO_LM_EVENT_PROMOTED | PLSVO_LM_EVENT_DELETED)) | ((ev & kInsJoinedBit) ? PLSVO_LM_EVENT_JOINED : 0) |
                                                    ((ev & kNewCandBit) ? PLSVO_LM_EVENT_NEW : 0)); };
    if (O.pt_event) for (size_t k = 0; k < np; ++k) O.pt_event[k] = public_event(hq[q.pt_ev + po + k]);
    if (O.seg_event) for (size_t k = 0; k < ns; ++k) O.seg_event[k] = public_event(hq[q.seg_ev + so + k]);
    cp(O.pt_cand, ptc.data(), (size_t)M.ptc_off, (size_t)M.n_pt_cand, sizeof(int)); cp(O.seg_cand, segc.data(), (size_t)M.segc_off, (size_t)M.n_seg_cand, sizeof(int));
  }
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_set_match(plsvo_ctx* c, int n, const plsvo_cand_match_out* in) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->cd_ran) return fail(c, PLSVO_E_STATE, "candidates_set_match: no candidates on the device");
  if (c->ci_inserted) return fail(c, PLSVO_E_STATE, "candidates_set_match: this run's frame was inserted (the tables have moved on); run again");
  if (c->cn_closed) return fail(c, PLSVO_E_STATE, "candidates_set_match: landmarks were added behind this run (the tables have moved on); run again");
  if (n != c->cd_n || (n > 0 && !in)) return fail(c, PLSVO_E_INVALID, "candidates_set_match: n does not match the staged batch");
  for (int s = 0; s < n; ++s) if (!in[s].found || !in[s].px || !in[s].search_level) return fail(c, PLSVO_E_INVALID, "candidates_set_match: null array");
  if (n == 0 || c->cd_total_m == 0) { c->cd_matched = true; return PLSVO_OK; }
  HIP_TRY(c, hipSetDevice(c->device));
  std::vector<int> cnt((size_t)n * 2);
  HIP_TRY(c, hipMemcpyAsync(cnt.data(), c->cd_b.counts, cnt.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const MatchBatchDev& mb = c->cd_match;
  for (int s = 0; s < n; ++s) {
    const size_t at = (size_t)c->cd_maps[(size_t)s].m_off, k = (size_t)cnt[2 * s] + 2 * (size_t)cnt[2 * s + 1];
    if (!k) continue;
    HIP_TRY(c, hipMemcpyAsync(mb.found + at, in[s].found, k, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(mb.px_out + 2 * at, in[s].px, k * 2 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(mb.search_level + at, in[s].search_level, k * sizeof(int), hipMemcpyHostToDevice, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->cd_matched = true;
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_select(plsvo_ctx* c, const plsvo_cand_select_params* sp) {
  CTX_CHECK(c);
  if (!sp) return fail(c, PLSVO_E_INVALID, "candidates_select: bad arguments");
  if (!c->cd_staged || !c->cd_ran || !c->cd_matched) return fail(c, PLSVO_E_STATE, "candidates_select: no match on the device");
  if (c->cs_selected) return fail(c, PLSVO_E_STATE, "candidates_select: this run's candidates were selected already (the tables have moved on)");
  if (c->cn_closed) return fail(c, PLSVO_E_STATE, "candidates_select: landmarks were added behind this run (the tables have moved on); run again");
  if (sp->max_fts < 0 || sp->max_fts_segs < 0 || sp->poseopt_n_iter < 0)
    return fail(c, PLSVO_E_INVALID, "candidates_select: bad parameters");
  const plsvo_cand_params& pr = c->cd_params;
  const int n = c->cd_n;
  const int n_cells = c->cd_b.grid_n_cols * ((pr.cam.height + pr.cell_size - 1) / pr.cell_size);
  const int seg_n_cells = c->cd_b.seg_grid_n_cols * ((pr.cam.height + pr.seg_cell_size - 1) / pr.seg_cell_size);
  std::vector<int> order;
  order.reserve(2 * ((size_t)n_cells + (size_t)seg_n_cells));
  if (!append_cell_order(order, sp->cell_order, n_cells) || !append_cell_order(order, sp->seg_cell_order, seg_n_cells))
    return fail(c, PLSVO_E_INVALID, "candidates_select: a cell order is not a permutation of its grid");
  if (n == 0) { c->cs_selected = true; return PLSVO_OK; }
  HIP_TRY(c, hipSetDevice(c->device));
  if (order != c->cs_order || !c->cs_d_order.p) {   // the visit orders travel when they change (the reference shuffles them once)
    Blob blob; blob.add(order);
    int rc;
    if ((rc = upload_blob(c, c->cs_d_order, blob))) return rc;
    c->cs_order = order;
  }
  const size_t N = (size_t)n, np = c->cd_t_opt, ns = 2 * c->cd_t_oseg;
  Carver w;
  const size_t w_win = w.take<unsigned int>(N * (size_t)n_cells), w_sc = w.take<int>(N * 3), w_plm = w.take<int>(np), w_ppx = w.take<double>(np * 2), w_plev = w.take<int>(np),
               w_pty = w.take<uint8_t>(np), w_pgr = w.take<double>(np * 2), w_slm = w.take<int>(ns), w_spx = w.take<double>(ns * 4), w_slev = w.take<int>(ns),
               w_jobs = w.take<PoseJobDev>(N), w_ptf = w.take<double>(np * 3), w_ptpos = w.take<double>(np * 3), w_ptlev = w.take<int>(np), w_line = w.take<double>(ns * 3),
               w_spos = w.take<double>(ns * 3), w_epos = w.take<double>(ns * 3), w_seglev = w.take<int>(ns);
  HIP_TRY(c, c->cs_d_work.ensure(w.off + 256));
  const QualitySections q = quality_sections(c);
  char* dq = reinterpret_cast<char*>(c->cs_d_q.p); char* dw = reinterpret_cast<char*>(c->cs_d_work.p);
  const int* dord = c->cs_d_order.as<int>();
  auto WD = [&](size_t o) { return reinterpret_cast<double*>(dw + o); };
  auto WI = [&](size_t o) { return reinterpret_cast<int*>(dw + o); };
  SelectBatchDev b{};
  b.c = c->cd_b;
  b.found = c->cd_match.found; b.px_out = c->cd_match.px_out; b.search_level = c->cd_match.search_level;
  b.n_cells = n_cells; b.seg_n_cells = seg_n_cells; b.max_fts = sp->max_fts; b.max_fts_segs = sp->max_fts_segs; b.n_pyr_levels = pr.n_pyr_levels;
  b.cell_order = dord; b.cell_pos = dord + n_cells; b.seg_cell_order = dord + 2 * n_cells; b.seg_cell_pos = dord + 2 * n_cells + seg_n_cells;
  b.pt_nfail = reinterpret_cast<int*>(dq + q.pt_nf); b.pt_nsucc = reinterpret_cast<int*>(dq + q.pt_ns);
  b.seg_nfail = reinterpret_cast<int*>(dq + q.seg_nf); b.seg_nsucc = reinterpret_cast<int*>(dq + q.seg_ns);
  b.pt_event = reinterpret_cast<uint8_t*>(dq + q.pt_ev); b.seg_event = reinterpret_cast<uint8_t*>(dq + q.seg_ev);
  b.cell_win = reinterpret_cast<unsigned int*>(dw + w_win);
  b.f_pt_lm = WI(w_plm); b.f_pt_px = WD(w_ppx); b.f_pt_level = WI(w_plev); b.f_pt_type = reinterpret_cast<uint8_t*>(dw + w_pty); b.f_pt_grad = WD(w_pgr);
  b.f_seg_lm = WI(w_slm); b.f_seg_px = WD(w_spx); b.f_seg_level = WI(w_slev); b.scalars = WI(w_sc);
  b.po_jobs = reinterpret_cast<PoseJobDev*>(dw + w_jobs); b.pt_f = WD(w_ptf); b.pt_pos = WD(w_ptpos); b.pt_level = WI(w_ptlev);
  b.seg_line = WD(w_line); b.seg_spos = WD(w_spos); b.seg_epos = WD(w_epos); b.seg_level = WI(w_seglev);
  b.reproj_thresh = sp->reproj_thresh; b.po_n_iter = sp->poseopt_n_iter; b.ldlt_flavour = c->ldlt_flavour;
  c->cs_b = b;
  c->cs_win_bytes = N * (size_t)n_cells * sizeof(unsigned int);
  {
    EventPair ep{}; prof_begin(c, PLSVO_K_SELECT, &ep);
    // ahead of EVERY launch: the event bytes are zero, the cells' winner words all ones
    hipError_t rearm_then_launch = hipMemsetAsync(dq + q.pt_ev, 0, q.end - q.pt_ev, c->stream);
    if (rearm_then_launch == hipSuccess) rearm_then_launch = hipMemsetAsync(b.cell_win, 0xff, c->cs_win_bytes, c->stream);
    if (rearm_then_launch == hipSuccess) rearm_then_launch = launch_map_select(b, c->stream);
    prof_end(c, PLSVO_K_SELECT, &ep);                // ahead of the error return, as in plsvo_candidates_run
    HIP_TRY(c, rearm_then_launch);
  }
  c->cs_selected = true;
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_select_fetch(plsvo_ctx* c, int n, plsvo_cand_select_out* out) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->cs_selected) return fail(c, PLSVO_E_STATE, "candidates_select_fetch: no selection to fetch");
  if (n != c->cd_n || (n > 0 && !out)) return fail(c, PLSVO_E_INVALID, "candidates_select_fetch: n does not match the staged batch");
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const SelectBatchDev& b = c->cs_b;
  // the features lie between the scalars and the pose optimiser's jobs: one copy
  const char* lo = reinterpret_cast<const char*>(b.scalars); const char* hi = reinterpret_cast<const char*>(b.po_jobs);
  std::vector<char> h((size_t)(hi - lo));
  HIP_TRY(c, hipMemcpyAsync(h.data(), lo, h.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  auto H = [&](const void* dev) { return h.data() + (reinterpret_cast<const char*>(dev) - lo); };
  auto cp = [&](void* dst, const void* dev, size_t at, size_t count, size_t elem) { if (dst && count) memcpy(dst, H(dev) + at * elem, count * elem); };
  const int* sc = reinterpret_cast<const int*>(H(b.scalars));
  for (int s = 0; s < n; ++s) {
    const CandMapDev& M = c->cd_maps[(size_t)s];
    plsvo_cand_select_out& O = out[s];
    O.n_matches = sc[3 * s]; O.n_ls_matches = sc[3 * s + 1]; O.n_trials = sc[3 * s + 2]; O.reserved0 = 0;
    const size_t np = (size_t)O.n_matches, ns = (size_t)O.n_ls_matches, po = (size_t)M.opt_off, so = 2 * (size_t)M.oseg_off;
    cp(O.pt_lm, b.f_pt_lm, po, np, sizeof(int)); cp(O.pt_px, b.f_pt_px, po * 2, np * 2, sizeof(double)); cp(O.pt_level, b.f_pt_level, po, np, sizeof(int));
    cp(O.pt_type, b.f_pt_type, po, np, 1); cp(O.pt_grad, b.f_pt_grad, po * 2, np * 2, sizeof(double));
    cp(O.seg_lm, b.f_seg_lm, so, ns, sizeof(int)); cp(O.seg_px, b.f_seg_px, so * 4, ns * 4, sizeof(double)); cp(O.seg_level, b.f_seg_level, so, ns, sizeof(int));
  }
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_pose_optimize(plsvo_ctx* c) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->cs_selected) return fail(c, PLSVO_E_STATE, "candidates_pose_optimize: no selection on the device");
  if (c->ci_inserted) return fail(c, PLSVO_E_STATE, "candidates_pose_optimize: this run's frame was inserted (the tables have moved on); run again");
  if (c->cn_closed) return fail(c, PLSVO_E_STATE, "candidates_pose_optimize: landmarks were added behind this run (the tables have moved on); run again");
  const int n = c->cd_n;
  c->cs_posed = false;
  if (n == 0) { c->cs_posed = true; return PLSVO_OK; }
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t np = std::max(c->cd_t_opt, (size_t)1), ns = std::max(2 * c->cd_t_oseg, (size_t)1), nft = np + ns;
  HIP_TRY(c, c->cs_d_ptkeep.ensure(np));
  HIP_TRY(c, c->cs_d_segkeep.ensure(ns));
  HIP_TRY(c, c->cs_d_s32.ensure(nft * sizeof(float)));
  HIP_TRY(c, c->cs_d_s64.ensure(nft * 5 * sizeof(double)));
  HIP_TRY(c, c->cs_d_state.ensure((size_t)n * sizeof(PoseStateDev)));
  HIP_TRY(c, c->cs_d_poses.ensure((size_t)n * 7 * sizeof(double)));
  const SelectBatchDev& b = c->cs_b;
  PoseBatchDev& q = c->cs_pose;
  q = PoseBatchDev{};
  q.jobs = b.po_jobs; q.state = c->cs_d_state.as<PoseStateDev>();
  q.pt_f = b.pt_f; q.pt_pos = b.pt_pos; q.pt_level = b.pt_level; q.seg_line = b.seg_line; q.seg_spos = b.seg_spos; q.seg_epos = b.seg_epos; q.seg_level = b.seg_level;
  q.pt_keep = c->cs_d_ptkeep.as<uint8_t>(); q.seg_keep = c->cs_d_segkeep.as<uint8_t>();
  q.scratch_f32 = c->cs_d_s32.as<float>(); q.scratch_f64 = c->cs_d_s64.as<double>();
  q.log = nullptr; q.log_cap = 0; q.n_jobs = n;
  const int threads = pose_opt_threads(c, n, (long)nft);   // (selected features <= filed landmarks)
  c->p_refill_frames = 0;                           // (jobs written on the device, as in plsvo_chain_run)
  EventPair ep{}; prof_begin(c, PLSVO_K_POSEOPT, &ep);
  const hipError_t launched = launch_pose_opt(q, c->cs_d_poses.as<double>(), threads, c->opt_poseopt_select ? 1 : 0, c->stream);
  prof_end(c, PLSVO_K_POSEOPT, &ep);
  HIP_TRY(c, launched);
  c->cs_posed = true;
  return PLSVO_OK;
}

extern "C" const double* plsvo_candidates_poses_dev(plsvo_ctx* c) { return (c && c->cd_staged && c->cs_posed) ? c->cs_d_poses.as<double>() : nullptr; }

extern "C" int plsvo_candidates_pose_fetch(plsvo_ctx* c, int n, plsvo_poseopt_out* out) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->cs_selected || !c->cs_posed) return fail(c, PLSVO_E_STATE, "candidates_pose_fetch: no pose optimisation to fetch");
  if (n != c->cd_n || (n > 0 && !out)) return fail(c, PLSVO_E_INVALID, "candidates_pose_fetch: n does not match the staged batch");
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t NP = std::max(c->cd_t_opt, (size_t)1), NS = std::max(2 * c->cd_t_oseg, (size_t)1);
  std::vector<PoseStateDev> st((size_t)n);
  std::vector<PoseJobDev> jobs((size_t)n);
  std::vector<uint8_t> pk(NP), sk(NS);
  HIP_TRY(c, hipMemcpyAsync(st.data(), c->cs_d_state.p, (size_t)n * sizeof(PoseStateDev), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(jobs.data(), c->cs_b.po_jobs, (size_t)n * sizeof(PoseJobDev), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(pk.data(), c->cs_d_ptkeep.p, NP, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(sk.data(), c->cs_d_segkeep.p, NS, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int j = 0; j < n; ++j) {
    const PoseStateDev& s = st[(size_t)j]; const PoseJobDev& J = jobs[(size_t)j];
    plsvo_poseopt_out& o = out[j];
    uint8_t* pko = o.pt_keep; uint8_t* sko = o.seg_keep;
    memset(&o, 0, sizeof(o));
    o.pt_keep = pko; o.seg_keep = sko;
    for (int k = 0; k < 7; ++k) o.T_f_w[k] = s.T[k];
    for (int k = 0; k < 36; ++k) o.cov[k] = s.cov[k];
    o.estimated_scale = s.estimated_scale; o.error_init = s.error_init; o.error_final = s.error_final;
    o.num_obs_pt = s.num_obs_pt; o.num_obs_ls = s.num_obs_ls;
    o.iters = s.iters; o.iters_ref = s.iters_ref; o.status = s.status;
    if (pko && J.n_pts > 0) memcpy(pko, pk.data() + J.pt_off, (size_t)J.n_pts);
    if (sko && J.n_seg > 0) memcpy(sko, sk.data() + J.seg_off, (size_t)J.n_seg);
  }
  return PLSVO_OK;
}

// ---- keyframe insertion into the resident map tables (insert_device.hpp) ---------------------------------------------
extern "C" int plsvo_candidates_reserve(plsvo_ctx* c, const plsvo_cand_reserve* r) {
  CTX_CHECK(c);
  if (r && (r->extra_kf < 0 || r->extra_kf_pt < 0 || r->extra_kf_seg < 0 || r->extra_pt_obs < 0 || r->extra_seg_obs < 0)) return fail(c, PLSVO_E_INVALID, "candidates_reserve: negative room");
  c->ci_reserve = r ? *r : plsvo_cand_reserve{};
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_insert_keyframe(plsvo_ctx* c, int n, const plsvo_cand_insert* in) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->cd_ran || !c->cs_selected) return fail(c, PLSVO_E_STATE, "candidates_insert_keyframe: no selection on the last run");
  if (c->ci_inserted) return fail(c, PLSVO_E_STATE, "candidates_insert_keyframe: this run's frame was inserted already");
  if (c->cn_closed) return fail(c, PLSVO_E_STATE, "candidates_insert_keyframe: landmarks were added behind this run (the tables have moved on); run again");
  if (n != c->cd_n || (n > 0 && !in)) return fail(c, PLSVO_E_INVALID, "candidates_insert_keyframe: n does not match the staged batch");
  bool any = false, host_masks = false;
  for (int s = 0; s < n; ++s) {
    const plsvo_cand_insert& I = in[s];
    if (!I.is_kf) continue;
    any = true;
    if (I.remove_kf < -1 || I.remove_kf >= c->cd_maps[(size_t)s].n_kf) return fail(c, PLSVO_E_INVALID, "candidates_insert_keyframe: remove_kf outside the keyframe table");
    if (I.kf_slot < 0) return fail(c, PLSVO_E_INVALID, "candidates_insert_keyframe: negative pyramid slot");
    if (I.pose_source < PLSVO_INSERT_POSE_HOST || I.pose_source > PLSVO_INSERT_POSE_RESIDENT || (I.pose_source == PLSVO_INSERT_POSE_DEV && !I.d_T_f_w))
      return fail(c, PLSVO_E_INVALID, "candidates_insert_keyframe: bad pose source");
    if (I.pt_keep || I.seg_keep) host_masks = true;
  }
  for (int s = 0; s < n; ++s)
    if (in[s].is_kf && (!in[s].pt_keep || !in[s].seg_keep || in[s].pose_source == PLSVO_INSERT_POSE_RESIDENT) && !c->cs_posed)
      return fail(c, PLSVO_E_STATE, "candidates_insert_keyframe: no resident pose optimisation for the masks or the pose");
  for (int s = 0; s < n; ++s)                       // the keyframe count needs no launch
    if (in[s].is_kf && c->cd_maps[(size_t)s].n_kf + 1 - (in[s].remove_kf >= 0 ? 1 : 0) > c->ci_cap[5 * (size_t)s])
      return fail(c, PLSVO_E_CAPACITY, "candidates_insert_keyframe: no room for another keyframe (plsvo_candidates_reserve)");
  const size_t N = (size_t)n;
  c->ci_last.assign(N, InsertPlanDev{});
  for (int s = 0; s < n; ++s) {
    InsertPlanDev& O = c->ci_last[(size_t)s]; const CandMapDev& M = c->cd_maps[(size_t)s]; const int* us = c->ci_used.data() + 4 * (size_t)s;
    O.n_kf = M.n_kf; O.new_kf = -1; O.n_kf_pt = us[0]; O.n_kf_seg = us[1]; O.n_pt_obs = us[2]; O.n_seg_obs = us[3]; O.n_pt_cand = M.n_pt_cand; O.n_seg_cand = M.n_seg_cand;
  }
  if (!any) { c->ci_have_out = true; return PLSVO_OK; }
  HIP_TRY(c, hipSetDevice(c->device));
  // -- the records and the caller's masks, laid out like the resident masks (feature rows from opt_off / 2 * oseg_off)
  std::vector<int> sc(N * 3);
  if (host_masks) {
    HIP_TRY(c, hipMemcpyAsync(sc.data(), c->cs_b.scalars, sc.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  Blob blob;
  const size_t b_jobs = blob.reserve<InsertJobDev>(N);
  const size_t b_pk = host_masks ? blob.reserve<uint8_t>(c->cd_t_opt) : 0, b_sk = host_masks ? blob.reserve<uint8_t>(2 * c->cd_t_oseg) : 0;
  HIP_TRY(c, c->ci_d_in.ensure(std::max(blob.host.size(), (size_t)256)));
  HIP_TRY(c, c->ci_d_plan.ensure(N * sizeof(InsertPlanDev)));
  const uint8_t* din = c->ci_d_in.as<uint8_t>();
  InsertJobDev* jobs = blob.at<InsertJobDev>(b_jobs);
  for (int s = 0; s < n; ++s) {
    const plsvo_cand_insert& I = in[s]; const CandMapDev& M = c->cd_maps[(size_t)s];
    InsertJobDev& J = jobs[s];
    memset(&J, 0, sizeof(J));
    J.is_kf = I.is_kf ? 1 : 0; J.remove_kf = I.remove_kf; J.kf_slot = I.kf_slot;
    if (!J.is_kf) continue;
    memcpy(J.T, I.T_f_w, sizeof(J.T));
    J.d_T = I.pose_source == PLSVO_INSERT_POSE_DEV ? I.d_T_f_w : I.pose_source == PLSVO_INSERT_POSE_RESIDENT ? c->cs_d_poses.as<double>() + 7 * (size_t)s : nullptr;
    J.pt_keep = c->cs_d_ptkeep.as<uint8_t>(); J.seg_keep = c->cs_d_segkeep.as<uint8_t>();
    if (I.pt_keep) { J.pt_keep = din + b_pk; if (sc[3 * (size_t)s] > 0) memcpy(blob.at<uint8_t>(b_pk) + M.opt_off, I.pt_keep, (size_t)sc[3 * (size_t)s]); }
    if (I.seg_keep) { J.seg_keep = din + b_sk; if (sc[3 * (size_t)s + 1] > 0) memcpy(blob.at<uint8_t>(b_sk) + 2 * M.oseg_off, I.seg_keep, (size_t)sc[3 * (size_t)s + 1]); }
  }
  int rc;
  if ((rc = upload_blob(c, c->ci_d_in, blob))) return rc;
  // -- scratch per landmark, per candidate entry and per new feature; staging rows of the arrays that shift
  Carver w;
  InsertBatchDev b{};
  size_t o_k[2][17];
  for (int k = 0; k < 2; ++k) {
    const size_t lm = k ? c->cd_t_seg : c->cd_t_pt, cnd = k ? c->cd_t_segc : c->cd_t_ptc, ftr = k ? 2 * c->cd_t_oseg : c->cd_t_opt;
    const size_t kfl = k ? c->ci_t_kfseg : c->ci_t_kfpt, obs = k ? c->ci_t_segobs : c->ci_t_ptobs;
    size_t* o = o_k[k];
    o[0] = w.take<unsigned int>(lm); o[1] = w.take<unsigned int>(lm); o[2] = w.take<int>(lm); o[3] = w.take<int>(lm); o[4] = w.take<int>(lm);
    o[5] = w.take<int>(cnd); o[6] = w.take<int>(ftr); o[7] = w.take<int>(c->ci_t_kf + N); o[8] = w.take<int>(kfl); o[9] = w.take<int>(lm + N);
    o[10] = w.take<int>(obs); o[11] = w.take<int>(obs); o[12] = w.take<double>(obs * 2); o[13] = w.take<double>(obs * (k ? 2 : 3)); o[14] = w.take<double>(obs * (k ? 3 : 2));
    o[15] = w.take<double>(k ? obs * 3 : 1); o[16] = w.take<uint8_t>(k ? 1 : obs);
  }
  HIP_TRY(c, c->ci_d_work.ensure(w.off + 256));
  char* dw = reinterpret_cast<char*>(c->ci_d_work.p);
  for (int k = 0; k < 2; ++k) {
    InsertKindDev& K = k ? b.seg : b.pt; const size_t* o = o_k[k];
    K.f0 = reinterpret_cast<unsigned int*>(dw + o[0]); K.f1 = reinterpret_cast<unsigned int*>(dw + o[1]);
    K.cnt = reinterpret_cast<int*>(dw + o[2]); K.len = reinterpret_cast<int*>(dw + o[3]); K.erase = reinterpret_cast<int*>(dw + o[4]);
    K.cand_kf = reinterpret_cast<int*>(dw + o[5]); K.new_lm = reinterpret_cast<int*>(dw + o[6]); K.kf_off2 = reinterpret_cast<int*>(dw + o[7]);
    K.kf_lm2 = reinterpret_cast<int*>(dw + o[8]); K.obs_off2 = reinterpret_cast<int*>(dw + o[9]); K.obs_kf2 = reinterpret_cast<int*>(dw + o[10]);
    K.obs_level2 = reinterpret_cast<int*>(dw + o[11]); K.obs_a2 = reinterpret_cast<double*>(dw + o[12]); K.obs_b2 = reinterpret_cast<double*>(dw + o[13]);
    K.obs_c2 = reinterpret_cast<double*>(dw + o[14]); K.obs_d2 = reinterpret_cast<double*>(dw + o[15]); K.obs_type2 = reinterpret_cast<uint8_t*>(dw + o[16]);
  }
  b.s = c->cs_b;
  b.jobs = reinterpret_cast<const InsertJobDev*>(din + b_jobs); b.plan = c->ci_d_plan.as<InsertPlanDev>();
  // -- the plan: decisions and counts in scratch; capacity is decided before anything is changed
  HIP_TRY(c, launch_map_insert_plan(b, c->stream));
  std::vector<InsertPlanDev> plan(N);
  HIP_TRY(c, hipMemcpyAsync(plan.data(), b.plan, N * sizeof(InsertPlanDev), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int s = 0; s < n; ++s) {
    if (!in[s].is_kf) continue;
    const InsertPlanDev& P = plan[(size_t)s]; const int* cp = c->ci_cap.data() + 5 * (size_t)s;
    if (P.n_kf > cp[0] || P.n_kf_pt > cp[1] || P.n_kf_seg > cp[2] || P.n_pt_obs > cp[3] || P.n_seg_obs > cp[4])
      return fail(c, PLSVO_E_CAPACITY, "candidates_insert_keyframe: a stream's new sizes exceed its room (plsvo_candidates_reserve); nothing was changed");
  }
  {
    EventPair ep{}; prof_begin(c, PLSVO_K_INSERT, &ep);
    const hipError_t launched = launch_map_insert(b, c->stream);
    prof_end(c, PLSVO_K_INSERT, &ep);                // ahead of the error return, as in plsvo_candidates_run
    HIP_TRY(c, launched);
  }
  // -- the host mirrors describe the new tables
  for (int s = 0; s < n; ++s) {
    if (!in[s].is_kf) { c->ci_last[(size_t)s] = plan[(size_t)s]; continue; }
    const InsertPlanDev& P = plan[(size_t)s];
    CandMapDev& M = c->cd_maps[(size_t)s];
    int* slot = c->cd_kf_slot.data() + M.kf_off;
    if (in[s].remove_kf >= 0) for (int k = in[s].remove_kf; k + 1 < M.n_kf; ++k) slot[k] = slot[k + 1];
    slot[P.new_kf] = in[s].kf_slot;
    for (int k = P.n_kf; k < c->ci_cap[5 * (size_t)s]; ++k) slot[k] = 0;
    M.n_kf = P.n_kf; M.n_pt_cand = P.n_pt_cand; M.n_seg_cand = P.n_seg_cand;
    c->cd_fetch_cand[2 * (size_t)s] = P.n_pt_cand; c->cd_fetch_cand[2 * (size_t)s + 1] = P.n_seg_cand;
    int* us = c->ci_used.data() + 4 * (size_t)s;
    us[0] = P.n_kf_pt; us[1] = P.n_kf_seg; us[2] = P.n_pt_obs; us[3] = P.n_seg_obs;
    c->ci_last[(size_t)s] = P;
  }
  c->cd_max_level = std::max(c->cd_max_level, c->cd_params.n_pyr_levels - 1);   // the new observations' levels are the matcher's search levels
  c->ci_inserted = true; c->ci_have_out = true;
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_capacity(plsvo_ctx* c, int n, plsvo_cand_reserve* out) {
  CTX_CHECK(c);
  if (!c->cd_staged) return fail(c, PLSVO_E_STATE, "candidates_capacity: no staged map tables");
  if (n != c->cd_n || (n > 0 && !out)) return fail(c, PLSVO_E_INVALID, "candidates_capacity: n does not match the staged batch");
  for (int s = 0; s < n; ++s) {
    const int* cp = c->ci_cap.data() + 5 * (size_t)s;
    out[s].extra_kf = cp[0]; out[s].extra_kf_pt = cp[1]; out[s].extra_kf_seg = cp[2]; out[s].extra_pt_obs = cp[3]; out[s].extra_seg_obs = cp[4]; out[s].reserved0 = 0;
  }
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_insert_fetch(plsvo_ctx* c, int n, plsvo_cand_insert_out* out) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->ci_have_out) return fail(c, PLSVO_E_STATE, "candidates_insert_fetch: no insertion since the tables were staged");
  if (n != c->cd_n || (n > 0 && !out)) return fail(c, PLSVO_E_INVALID, "candidates_insert_fetch: n does not match the staged batch");
  for (int s = 0; s < n; ++s) {
    const InsertPlanDev& P = c->ci_last[(size_t)s]; plsvo_cand_insert_out& O = out[s];
    O.n_kf = P.n_kf; O.new_kf = P.new_kf; O.n_kf_pt = P.n_kf_pt; O.n_kf_seg = P.n_kf_seg; O.n_pt_obs = P.n_pt_obs; O.n_seg_obs = P.n_seg_obs;
    O.n_pt_cand = P.n_pt_cand; O.n_seg_cand = P.n_seg_cand; O.n_joined_pt = P.n_joined_pt; O.n_joined_seg = P.n_joined_seg;
    O.n_deleted_pt = P.n_deleted_pt; O.n_deleted_seg = P.n_deleted_seg;
  }
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_fetch_map(plsvo_ctx* c, int n, plsvo_cand_map_out* out) {
  CTX_CHECK(c);
  if (!c->cd_staged) return fail(c, PLSVO_E_STATE, "candidates_fetch_map: no staged map tables");
  if (n != c->cd_n || (n > 0 && !out)) return fail(c, PLSVO_E_INVALID, "candidates_fetch_map: n does not match the staged batch");
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  std::vector<char> h(c->cd_blob_bytes);           // the tables are one allocation: one copy
  HIP_TRY(c, hipMemcpyAsync(h.data(), c->cd_d_blob.p, h.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const CandBatchDev& b = c->cd_b;
  const char* base = reinterpret_cast<const char*>(c->cd_d_blob.p);
  auto H = [&](const void* dev) { return h.data() + (reinterpret_cast<const char*>(dev) - base); };
  auto cp = [&](void* dst, const void* dev, size_t at, size_t count, size_t elem) { if (dst && count) memcpy(dst, H(dev) + at * elem, count * elem); };
  const CandMapDev* maps = reinterpret_cast<const CandMapDev*>(H(b.maps));
  for (int s = 0; s < n; ++s) {
    const CandMapDev& M = maps[s];
    plsvo_cand_map_out& O = out[s];
    const size_t nk = (size_t)M.n_kf, np = (size_t)M.n_pt, ns = (size_t)M.n_seg, S = (size_t)s;
    const int* kpo = reinterpret_cast<const int*>(H(b.kf_pt_off)) + M.kf_off + s; const int* kso = reinterpret_cast<const int*>(H(b.kf_seg_off)) + M.kf_off + s;
    const int* poo = reinterpret_cast<const int*>(H(b.pt_obs_off)) + M.pt_off + s; const int* soo = reinterpret_cast<const int*>(H(b.seg_obs_off)) + M.seg_off + s;
    const size_t kfpt = (size_t)kpo[nk], kfseg = (size_t)kso[nk], ptobs = (size_t)poo[np], segobs = (size_t)soo[ns];
    O.n_kf = M.n_kf; O.n_pt = M.n_pt; O.n_seg = M.n_seg; O.n_pt_cand = M.n_pt_cand; O.n_seg_cand = M.n_seg_cand;
    O.n_kf_pt = (int32_t)kfpt; O.n_kf_seg = (int32_t)kfseg; O.n_pt_obs = (int32_t)ptobs; O.n_seg_obs = (int32_t)segobs; O.reserved0 = 0;
    cp(O.kf_T, b.kf_T, (size_t)M.kf_off * 7, nk * 7, sizeof(double)); cp(O.kf_slot, b.frame_slot, (size_t)M.f_off, nk, sizeof(int));
    cp(O.kf_pt_off, b.kf_pt_off, (size_t)M.kf_off + S, nk + 1, sizeof(int)); cp(O.kf_seg_off, b.kf_seg_off, (size_t)M.kf_off + S, nk + 1, sizeof(int));
    cp(O.kf_pt_lm, b.kf_pt_lm, (size_t)M.kfpt_off, kfpt, sizeof(int)); cp(O.kf_seg_lm, b.kf_seg_lm, (size_t)M.kfseg_off, kfseg, sizeof(int));
    cp(O.pt_pos, b.pt_pos, (size_t)M.pt_off * 3, np * 3, sizeof(double)); cp(O.pt_type, b.pt_type, (size_t)M.pt_off, np, sizeof(int));
    cp(O.pt_obs_off, b.pt_obs_off, (size_t)M.pt_off + S, np + 1, sizeof(int)); cp(O.pt_obs_kf, b.pt_obs_kf, (size_t)M.ptobs_off, ptobs, sizeof(int));
    cp(O.pt_obs_px, b.pt_obs_px, (size_t)M.ptobs_off * 2, ptobs * 2, sizeof(double)); cp(O.pt_obs_f, b.pt_obs_f, (size_t)M.ptobs_off * 3, ptobs * 3, sizeof(double));
    cp(O.pt_obs_level, b.pt_obs_level, (size_t)M.ptobs_off, ptobs, sizeof(int)); cp(O.pt_obs_type, b.pt_obs_type, (size_t)M.ptobs_off, ptobs, 1);
    cp(O.pt_obs_grad, b.pt_obs_grad, (size_t)M.ptobs_off * 2, ptobs * 2, sizeof(double));
    cp(O.seg_spos, b.seg_spos, (size_t)M.seg_off * 3, ns * 3, sizeof(double)); cp(O.seg_epos, b.seg_epos, (size_t)M.seg_off * 3, ns * 3, sizeof(double));
    cp(O.seg_type, b.seg_type, (size_t)M.seg_off, ns, sizeof(int)); cp(O.seg_obs_off, b.seg_obs_off, (size_t)M.seg_off + S, ns + 1, sizeof(int));
    cp(O.seg_obs_kf, b.seg_obs_kf, (size_t)M.segobs_off, segobs, sizeof(int));
    cp(O.seg_obs_spx, b.seg_obs_spx, (size_t)M.segobs_off * 2, segobs * 2, sizeof(double)); cp(O.seg_obs_epx, b.seg_obs_epx, (size_t)M.segobs_off * 2, segobs * 2, sizeof(double));
    cp(O.seg_obs_sf, b.seg_obs_sf, (size_t)M.segobs_off * 3, segobs * 3, sizeof(double)); cp(O.seg_obs_ef, b.seg_obs_ef, (size_t)M.segobs_off * 3, segobs * 3, sizeof(double));
    cp(O.seg_obs_level, b.seg_obs_level, (size_t)M.segobs_off, segobs, sizeof(int));
    cp(O.pt_cand, b.pt_cand, (size_t)M.ptc_off, (size_t)M.n_pt_cand, sizeof(int)); cp(O.seg_cand, b.seg_cand, (size_t)M.segc_off, (size_t)M.n_seg_cand, sizeof(int));
  }
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_set_positions(plsvo_ctx* c, int n, const plsvo_cand_positions* in) {
  CTX_CHECK(c);
  if (!c->cd_staged) return fail(c, PLSVO_E_STATE, "candidates_set_positions: no staged map tables");
  if (n != c->cd_n || (n > 0 && !in)) return fail(c, PLSVO_E_INVALID, "candidates_set_positions: n does not match the staged batch");
  size_t t_pt = 0, t_seg = 0;
  for (int s = 0; s < n; ++s) {
    const plsvo_cand_positions& I = in[s]; const CandMapDev& M = c->cd_maps[(size_t)s];
    if (I.n_pt < 0 || I.n_seg < 0) return fail(c, PLSVO_E_INVALID, "candidates_set_positions: negative count");
    if ((I.n_pt > 0 && (!I.pt_idx || !I.pt_pos)) || (I.n_seg > 0 && (!I.seg_idx || !I.seg_spos || !I.seg_epos))) return fail(c, PLSVO_E_INVALID, "candidates_set_positions: null array");
    if (!cand_idx_ok(I.pt_idx, (size_t)I.n_pt, 0, M.n_pt) || !cand_idx_ok(I.seg_idx, (size_t)I.n_seg, 0, M.n_seg)) return fail(c, PLSVO_E_INVALID, "candidates_set_positions: landmark index out of range");
    t_pt += (size_t)I.n_pt; t_seg += (size_t)I.n_seg;
  }
  if (t_pt + t_seg == 0) return PLSVO_OK;
  if (t_pt > (size_t)INT32_MAX || t_seg > (size_t)INT32_MAX) return fail(c, PLSVO_E_CAPACITY, "candidates_set_positions: batch too large");
  HIP_TRY(c, hipSetDevice(c->device));
  Blob blob;
  const size_t b_pi = blob.reserve<long long>(t_pt), b_pp = blob.reserve<double>(t_pt * 3), b_si = blob.reserve<long long>(t_seg), b_ss = blob.reserve<double>(t_seg * 3),
               b_se = blob.reserve<double>(t_seg * 3);
  size_t ap = 0, as = 0;
  for (int s = 0; s < n; ++s) {
    const plsvo_cand_positions& I = in[s]; const CandMapDev& M = c->cd_maps[(size_t)s];
    for (int k = 0; k < I.n_pt; ++k) blob.at<long long>(b_pi)[ap + (size_t)k] = M.pt_off + I.pt_idx[k];
    if (I.n_pt) memcpy(blob.at<double>(b_pp) + 3 * ap, I.pt_pos, (size_t)I.n_pt * 3 * sizeof(double));
    for (int k = 0; k < I.n_seg; ++k) blob.at<long long>(b_si)[as + (size_t)k] = M.seg_off + I.seg_idx[k];
    if (I.n_seg) { memcpy(blob.at<double>(b_ss) + 3 * as, I.seg_spos, (size_t)I.n_seg * 3 * sizeof(double)); memcpy(blob.at<double>(b_se) + 3 * as, I.seg_epos, (size_t)I.n_seg * 3 * sizeof(double)); }
    ap += (size_t)I.n_pt; as += (size_t)I.n_seg;
  }
  int rc;
  if ((rc = upload_blob(c, c->ci_d_pos, blob))) return rc;
  const char* d = reinterpret_cast<const char*>(c->ci_d_pos.p);
  PositionsBatchDev p{};
  p.n_pt = (int)t_pt; p.n_seg = (int)t_seg;
  p.pt_at = reinterpret_cast<const long long*>(d + b_pi); p.pt_src = reinterpret_cast<const double*>(d + b_pp);
  p.seg_at = reinterpret_cast<const long long*>(d + b_si); p.seg_ssrc = reinterpret_cast<const double*>(d + b_ss); p.seg_esrc = reinterpret_cast<const double*>(d + b_se);
  p.pt_pos = const_cast<double*>(c->cd_b.pt_pos); p.seg_spos = const_cast<double*>(c->cd_b.seg_spos); p.seg_epos = const_cast<double*>(c->cd_b.seg_epos);
  HIP_TRY(c, launch_map_set_positions(p, c->stream));
  return PLSVO_OK;
}

// ---- new candidate landmarks appended to the resident map tables (newcand_device.hpp) -----------------------------------
extern "C" int plsvo_candidates_reserve_landmarks(plsvo_ctx* c, const plsvo_cand_lm_reserve* r) {
  CTX_CHECK(c);
  if (r && (r->extra_pt < 0 || r->extra_seg < 0)) return fail(c, PLSVO_E_INVALID, "candidates_reserve_landmarks: negative room");
  c->cn_reserve = r ? *r : plsvo_cand_lm_reserve{};
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_lm_capacity(plsvo_ctx* c, int n, plsvo_cand_lm_reserve* out) {
  CTX_CHECK(c);
  if (!c->cd_staged) return fail(c, PLSVO_E_STATE, "candidates_lm_capacity: no staged map tables");
  if (n != c->cd_n || (n > 0 && !out)) return fail(c, PLSVO_E_INVALID, "candidates_lm_capacity: n does not match the staged batch");
  for (int s = 0; s < n; ++s) { out[s].extra_pt = c->cn_cap[4 * (size_t)s]; out[s].extra_seg = c->cn_cap[4 * (size_t)s + 1]; }
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_add(plsvo_ctx* c, int n, const plsvo_cand_new* in) {
  CTX_CHECK(c);
  if (!c->cd_staged) return fail(c, PLSVO_E_STATE, "candidates_add: no staged map tables");
  if (n != c->cd_n || (n > 0 && !in)) return fail(c, PLSVO_E_INVALID, "candidates_add: n does not match the staged batch");
  // -- every check before anything is written: arguments, then room (from the host's mirrors: landmark count, used observation entries)
  size_t t_pt = 0, t_seg = 0;
  int max_level = c->cd_max_level;
  for (int s = 0; s < n; ++s) {
    const plsvo_cand_new& I = in[s]; const CandMapDev& M = c->cd_maps[(size_t)s];
    if (I.n_pt < 0 || I.n_seg < 0) return fail(c, PLSVO_E_INVALID, "candidates_add: negative count");
    if (I.n_pt > 0 && (!I.pt_pos || !I.pt_obs_kf || !I.pt_obs_px || !I.pt_obs_f || !I.pt_obs_level || !I.pt_obs_type)) return fail(c, PLSVO_E_INVALID, "candidates_add: null point array");
    if (I.n_seg > 0 && (!I.seg_spos || !I.seg_epos || !I.seg_obs_kf || !I.seg_obs_spx || !I.seg_obs_epx || !I.seg_obs_sf || !I.seg_obs_ef || !I.seg_obs_level))
      return fail(c, PLSVO_E_INVALID, "candidates_add: null segment array");
    if (!cand_idx_ok(I.pt_obs_kf, (size_t)I.n_pt, 0, M.n_kf) || !cand_idx_ok(I.seg_obs_kf, (size_t)I.n_seg, 0, M.n_kf)) return fail(c, PLSVO_E_INVALID, "candidates_add: observation keyframe outside the keyframe table");
    if (!cand_idx_ok(I.pt_obs_level, (size_t)I.n_pt, 0, PLSVO_MAX_LEVELS) || !cand_idx_ok(I.seg_obs_level, (size_t)I.n_seg, 0, PLSVO_MAX_LEVELS))
      return fail(c, PLSVO_E_INVALID, "candidates_add: observation level out of range");
    for (int k = 0; k < I.n_pt; ++k) {
      if (I.pt_obs_type[k] == PLSVO_FTR_EDGELET) { if (!I.pt_obs_grad) return fail(c, PLSVO_E_INVALID, "candidates_add: edgelets without pt_obs_grad"); }
      else if (I.pt_obs_type[k] != PLSVO_FTR_CORNER) return fail(c, PLSVO_E_INVALID, "candidates_add: unknown feature type");
      max_level = std::max(max_level, (int)I.pt_obs_level[k]);
    }
    for (int k = 0; k < I.n_seg; ++k) max_level = std::max(max_level, (int)I.seg_obs_level[k]);
    t_pt += (size_t)I.n_pt; t_seg += (size_t)I.n_seg;
  }
  for (int s = 0; s < n; ++s) {
    const plsvo_cand_new& I = in[s]; const CandMapDev& M = c->cd_maps[(size_t)s];
    const int* lc = c->cn_cap.data() + 4 * (size_t)s; const int* cp = c->ci_cap.data() + 5 * (size_t)s; const int* us = c->ci_used.data() + 4 * (size_t)s;
    if ((long long)M.n_pt + I.n_pt > lc[0] || (long long)M.n_seg + I.n_seg > lc[1])
      return fail(c, PLSVO_E_CAPACITY, "candidates_add: a stream lacks landmark rows (plsvo_candidates_reserve_landmarks); nothing was changed");
    if ((long long)us[2] + I.n_pt > cp[3] || (long long)us[3] + I.n_seg > cp[4])
      return fail(c, PLSVO_E_CAPACITY, "candidates_add: a stream lacks observation entries (plsvo_candidates_reserve); nothing was changed");
  }
  const size_t N = (size_t)n;
  c->cn_last.assign(N, plsvo_cand_add_out{});
  for (int s = 0; s < n; ++s) {
    const plsvo_cand_new& I = in[s]; const CandMapDev& M = c->cd_maps[(size_t)s];
    plsvo_cand_add_out& O = c->cn_last[(size_t)s];
    O.first_pt = I.n_pt ? M.n_pt : -1; O.first_seg = I.n_seg ? M.n_seg : -1; O.n_added_pt = I.n_pt; O.n_added_seg = I.n_seg;
  }
  c->cn_closed = true; c->cn_have_out = true;       // (an add of nothing ends the run too: the rule does not depend on the counts)
  if (t_pt + t_seg == 0) return PLSVO_OK;
  if (t_pt > (size_t)INT32_MAX || t_seg > (size_t)INT32_MAX) return fail(c, PLSVO_E_CAPACITY, "candidates_add: batch too large");
  HIP_TRY(c, hipSetDevice(c->device));
  Blob blob;
  const size_t b_jobs = blob.reserve<NewCandJobDev>(N);
  const size_t b_ppos = blob.reserve<double>(t_pt * 3), b_pkf = blob.reserve<int>(t_pt), b_ppx = blob.reserve<double>(t_pt * 2), b_pf = blob.reserve<double>(t_pt * 3),
               b_plv = blob.reserve<int>(t_pt), b_pty = blob.reserve<uint8_t>(t_pt), b_pgr = blob.reserve<double>(t_pt * 2);
  const size_t b_ss = blob.reserve<double>(t_seg * 3), b_se = blob.reserve<double>(t_seg * 3), b_skf = blob.reserve<int>(t_seg), b_sspx = blob.reserve<double>(t_seg * 2),
               b_sepx = blob.reserve<double>(t_seg * 2), b_ssf = blob.reserve<double>(t_seg * 3), b_sef = blob.reserve<double>(t_seg * 3), b_slv = blob.reserve<int>(t_seg);
  auto put = [&](size_t sec, size_t at, const void* src, size_t count, size_t elem) {
    if (count) { if (src) memcpy(blob.host.data() + sec + at * elem, src, count * elem); else memset(blob.host.data() + sec + at * elem, 0, count * elem); }
  };
  size_t ap = 0, as = 0;
  for (int s = 0; s < n; ++s) {
    const plsvo_cand_new& I = in[s];
    NewCandJobDev& J = blob.at<NewCandJobDev>(b_jobs)[s];
    J.n_pt = I.n_pt; J.n_seg = I.n_seg; J.pt_at = (long long)ap; J.seg_at = (long long)as;
    const size_t np = (size_t)I.n_pt, ns = (size_t)I.n_seg;
    put(b_ppos, ap * 3, I.pt_pos, np * 3, sizeof(double)); put(b_pkf, ap, I.pt_obs_kf, np, sizeof(int)); put(b_ppx, ap * 2, I.pt_obs_px, np * 2, sizeof(double));
    put(b_pf, ap * 3, I.pt_obs_f, np * 3, sizeof(double)); put(b_plv, ap, I.pt_obs_level, np, sizeof(int)); put(b_pty, ap, I.pt_obs_type, np, 1);
    put(b_pgr, ap * 2, I.pt_obs_grad, np * 2, sizeof(double));
    put(b_ss, as * 3, I.seg_spos, ns * 3, sizeof(double)); put(b_se, as * 3, I.seg_epos, ns * 3, sizeof(double)); put(b_skf, as, I.seg_obs_kf, ns, sizeof(int));
    put(b_sspx, as * 2, I.seg_obs_spx, ns * 2, sizeof(double)); put(b_sepx, as * 2, I.seg_obs_epx, ns * 2, sizeof(double));
    put(b_ssf, as * 3, I.seg_obs_sf, ns * 3, sizeof(double)); put(b_sef, as * 3, I.seg_obs_ef, ns * 3, sizeof(double)); put(b_slv, as, I.seg_obs_level, ns, sizeof(int));
    ap += np; as += ns;
  }
  int rc;
  if ((rc = upload_blob(c, c->cn_d_in, blob))) return rc;
  const char* d = reinterpret_cast<const char*>(c->cn_d_in.p);
  const QualitySections q = quality_sections(c);
  char* dq = reinterpret_cast<char*>(c->cs_d_q.p);
  auto D = [&](size_t o) { return reinterpret_cast<const double*>(d + o); };
  auto Iv = [&](size_t o) { return reinterpret_cast<const int*>(d + o); };
  NewCandBatchDev b{};
  b.c = c->cd_b;
  b.pt_nfail = reinterpret_cast<int*>(dq + q.pt_nf); b.pt_nsucc = reinterpret_cast<int*>(dq + q.pt_ns);
  b.seg_nfail = reinterpret_cast<int*>(dq + q.seg_nf); b.seg_nsucc = reinterpret_cast<int*>(dq + q.seg_ns);
  b.pt_event = reinterpret_cast<uint8_t*>(dq + q.pt_ev); b.seg_event = reinterpret_cast<uint8_t*>(dq + q.seg_ev);
  b.jobs = reinterpret_cast<const NewCandJobDev*>(d + b_jobs);
  b.pt_pos = D(b_ppos); b.pt_obs_kf = Iv(b_pkf); b.pt_obs_px = D(b_ppx); b.pt_obs_f = D(b_pf); b.pt_obs_level = Iv(b_plv);
  b.pt_obs_type = reinterpret_cast<const uint8_t*>(d + b_pty); b.pt_obs_grad = D(b_pgr);
  b.seg_spos = D(b_ss); b.seg_epos = D(b_se); b.seg_obs_kf = Iv(b_skf); b.seg_obs_spx = D(b_sspx); b.seg_obs_epx = D(b_sepx); b.seg_obs_sf = D(b_ssf);
  b.seg_obs_ef = D(b_sef); b.seg_obs_level = Iv(b_slv);
  {
    EventPair ep{}; prof_begin(c, PLSVO_K_NEWCAND, &ep);
    const hipError_t launched = launch_map_add_candidates(b, c->stream);
    prof_end(c, PLSVO_K_NEWCAND, &ep);               // ahead of the error return, as in plsvo_candidates_run
    HIP_TRY(c, launched);
  }
  // -- the host mirrors describe the new tables (the candidate counts are upper bounds: the selection shortens the lists on the device)
  for (int s = 0; s < n; ++s) {
    CandMapDev& M = c->cd_maps[(size_t)s]; int* us = c->ci_used.data() + 4 * (size_t)s;
    M.n_pt += in[s].n_pt; M.n_seg += in[s].n_seg; M.n_pt_cand += in[s].n_pt; M.n_seg_cand += in[s].n_seg;
    us[2] += in[s].n_pt; us[3] += in[s].n_seg;
  }
  c->cd_max_level = max_level;
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_add_fetch(plsvo_ctx* c, int n, plsvo_cand_add_out* out) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->cn_have_out) return fail(c, PLSVO_E_STATE, "candidates_add_fetch: no add since the tables were staged");
  if (n != c->cd_n || (n > 0 && !out)) return fail(c, PLSVO_E_INVALID, "candidates_add_fetch: n does not match the staged batch");
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  std::vector<CandMapDev> maps((size_t)n);         // the candidate counts as they stand are the device's
  HIP_TRY(c, hipMemcpyAsync(maps.data(), c->cd_b.maps, (size_t)n * sizeof(CandMapDev), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int s = 0; s < n; ++s) {
    const CandMapDev& M = maps[(size_t)s]; const int* us = c->ci_used.data() + 4 * (size_t)s;
    out[s] = c->cn_last[(size_t)s];
    out[s].n_pt = M.n_pt; out[s].n_seg = M.n_seg; out[s].n_pt_cand = M.n_pt_cand; out[s].n_seg_cand = M.n_seg_cand; out[s].n_pt_obs = us[2]; out[s].n_seg_obs = us[3];
  }
  return PLSVO_OK;
}

// ---- trajectory record (host only; app/run_pipeline.cpp:425-451) ---------------------------------------
extern "C" int plsvo_trajectory_record(const double T_f_w[7], const double cov[36], double out7[7]) {
  if (!T_f_w || !cov || !out7) return 0;
  bool skip_frame = false;
  for (int i = 0; i < 36; ++i) if (!((1.e-16 < std::fabs(cov[i])) && (std::fabs(cov[i]) < 1.e+16))) skip_frame = true;
  const SE3d W = se3_inv(se3_load(T_f_w));   // world_transf = T_f_w_.inverse()
  if ((W.t[0] == 0. && W.t[1] == 0. && W.t[2] == 0.) && (W.q.x == -0. && W.q.y == -0. && W.q.z == -0. && W.q.w == 1.)) skip_frame = true;
  out7[0] = W.t[0]; out7[1] = W.t[1]; out7[2] = W.t[2]; out7[3] = W.q.x; out7[4] = W.q.y; out7[5] = W.q.z; out7[6] = W.q.w;
  return skip_frame ? 0 : 1;
}

// ---- depth-filter seed update ----------------------------------------------------------------------------
extern "C" int plsvo_update_seeds(plsvo_ctx* c, const plsvo_seeds_in* in, plsvo_seeds_out* out) {
  CTX_CHECK(c);
  if (!in || !out || in->n_pt < 0 || in->n_seg < 0 || in->n_frames < 0 || in->n_pyr_levels < 1 || in->align_max_iter < 0 || in->max_epi_search_steps < 0)
    return fail(c, PLSVO_E_INVALID, "update_seeds: bad arguments");
  const int np = in->n_pt, ns = in->n_seg, nf = in->n_frames;
  if (np + ns == 0) return PLSVO_OK;
  if (!c->pyr.base) return fail(c, PLSVO_E_STATE, "update_seeds: pyramids not configured");
  if (nf <= 0 || !in->frame_T || !in->frame_slot) return fail(c, PLSVO_E_INVALID, "update_seeds: no frames");
  if (in->n_pyr_levels > c->pyr.n_levels) return fail(c, PLSVO_E_INVALID, "update_seeds: n_pyr_levels exceeds the configured pyramid");
  if (in->cam.width != c->pyr.w[0] || in->cam.height != c->pyr.h[0]) return fail(c, PLSVO_E_INVALID, "update_seeds: camera size does not match the configured pyramid");
  if (np > 0 && (!in->pt_ref_frame || !in->pt_cur_frame || !in->pt_px || !in->pt_f || !in->pt_level || !in->pt_type || !in->pt_a || !in->pt_b || !in->pt_mu || !in->pt_z_range || !in->pt_sigma2))
    return fail(c, PLSVO_E_INVALID, "update_seeds: null point-seed array");
  if (ns > 0 && (!in->seg_ref_frame || !in->seg_cur_frame || !in->seg_px || !in->seg_f || !in->seg_sf || !in->seg_ef || !in->seg_level || !in->seg_a || !in->seg_b ||
                 !in->seg_mu_s || !in->seg_mu_e || !in->seg_z_range_s || !in->seg_z_range_e || !in->seg_sigma2_s || !in->seg_sigma2_e))
    return fail(c, PLSVO_E_INVALID, "update_seeds: null line-seed array");
  for (int k = 0; k < nf; ++k) if (in->frame_slot[k] < 0 || in->frame_slot[k] >= c->pyr.n_slots) return fail(c, PLSVO_E_CAPACITY, "update_seeds: pyramid slot out of range");
  bool any_edgelet = false;
  for (int i = 0; i < np; ++i) {
    if (in->pt_ref_frame[i] < 0 || in->pt_ref_frame[i] >= nf || in->pt_cur_frame[i] < 0 || in->pt_cur_frame[i] >= nf) return fail(c, PLSVO_E_INVALID, "update_seeds: frame index out of range");
    if (in->pt_level[i] < 0 || in->pt_level[i] >= c->pyr.n_levels) return fail(c, PLSVO_E_INVALID, "update_seeds: feature level outside the configured pyramid");
    if (in->pt_type[i] == PLSVO_FTR_EDGELET) any_edgelet = true;
  }
  if (any_edgelet && in->edgelet_filtering && !in->pt_grad) return fail(c, PLSVO_E_INVALID, "update_seeds: edgelets without pt_grad");
  for (int i = 0; i < ns; ++i) {
    if (in->seg_ref_frame[i] < 0 || in->seg_ref_frame[i] >= nf || in->seg_cur_frame[i] < 0 || in->seg_cur_frame[i] >= nf) return fail(c, PLSVO_E_INVALID, "update_seeds: frame index out of range");
    if (in->seg_level[i] < 0 || in->seg_level[i] >= c->pyr.n_levels) return fail(c, PLSVO_E_INVALID, "update_seeds: feature level outside the configured pyramid");
  }
  HIP_TRY(c, hipSetDevice(c->device));
  // one packed upload per element type
  std::vector<double> d; std::vector<int> iv; std::vector<float> fv;
  auto putd = [&](const double* p, size_t k) { const size_t o = d.size(); if (p) d.insert(d.end(), p, p + k); else d.resize(d.size() + k, 0.0); return o; };
  auto puti = [&](const int32_t* p, size_t k) { const size_t o = iv.size(); iv.insert(iv.end(), p, p + k); return o; };
  auto putf = [&](const float* p, size_t k) { const size_t o = fv.size(); fv.insert(fv.end(), p, p + k); return o; };
  const size_t NP = (size_t)np, NS = (size_t)ns;
  const size_t o_T = putd(in->frame_T, (size_t)nf * 7), o_ppx = putd(in->pt_px, NP * 2), o_pf = putd(in->pt_f, NP * 3), o_pg = putd(in->pt_grad, NP * 2);
  const size_t o_spx = putd(in->seg_px, NS * 2), o_sf0 = putd(in->seg_f, NS * 3), o_ssf = putd(in->seg_sf, NS * 3), o_sef = putd(in->seg_ef, NS * 3);
  const size_t o_slot = puti(in->frame_slot, (size_t)nf), o_prf = puti(in->pt_ref_frame, NP), o_pcf = puti(in->pt_cur_frame, NP), o_plv = puti(in->pt_level, NP);
  const size_t o_srf = puti(in->seg_ref_frame, NS), o_scf = puti(in->seg_cur_frame, NS), o_slv = puti(in->seg_level, NS);
  const size_t o_pa = putf(in->pt_a, NP), o_pb = putf(in->pt_b, NP), o_pmu = putf(in->pt_mu, NP), o_pzr = putf(in->pt_z_range, NP), o_ps2 = putf(in->pt_sigma2, NP);
  const size_t o_sa = putf(in->seg_a, NS), o_sb = putf(in->seg_b, NS), o_smus = putf(in->seg_mu_s, NS), o_smue = putf(in->seg_mu_e, NS);
  const size_t o_szrs = putf(in->seg_z_range_s, NS), o_szre = putf(in->seg_z_range_e, NS), o_ss2s = putf(in->seg_sigma2_s, NS), o_ss2e = putf(in->seg_sigma2_e, NS);
  auto pad16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
  const size_t dbytes = pad16(d.size() * sizeof(double)), ibytes = pad16(iv.size() * sizeof(int)), fbytes = pad16(fv.size() * sizeof(float)), bbytes = pad16(NP);
  HIP_TRY(c, c->s_d_in.ensure(dbytes + ibytes + fbytes + bbytes + 16));
  char* din = reinterpret_cast<char*>(c->s_d_in.p);
  HIP_TRY(c, hipMemcpyAsync(din, d.data(), d.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(din + dbytes, iv.data(), iv.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  if (!fv.empty()) HIP_TRY(c, hipMemcpyAsync(din + dbytes + ibytes, fv.data(), fv.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  if (np > 0) HIP_TRY(c, hipMemcpyAsync(din + dbytes + ibytes + fbytes, in->pt_type, NP, hipMemcpyHostToDevice, c->stream));
  // outputs: doubles, then floats, then ints
  const size_t od_n = NP * 6 + NS * 8, of_n = NP * 4 + NS * 6, oi_n = NP + NS;
  const size_t od_b = pad16(od_n * sizeof(double)), of_b = pad16(of_n * sizeof(float)), oi_b = pad16(oi_n * sizeof(int));
  HIP_TRY(c, c->s_d_out.ensure(od_b + of_b + oi_b + 16));
  char* dout = reinterpret_cast<char*>(c->s_d_out.p);
  const double* dd = reinterpret_cast<const double*>(din);
  const int* di = reinterpret_cast<const int*>(din + dbytes);
  const float* df = reinterpret_cast<const float*>(din + dbytes + ibytes);
  double* od = reinterpret_cast<double*>(dout);
  float* of = reinterpret_cast<float*>(dout + od_b);
  int* oi = reinterpret_cast<int*>(dout + od_b + of_b);
  SeedsBatchDev b{};
  b.pyr_base = c->pyr.base; b.slot_bytes = c->pyr.slot_bytes; b.width = c->pyr.w[0]; b.height = c->pyr.h[0];
  b.fx = in->cam.fx; b.fy = in->cam.fy; b.cx = in->cam.cx; b.cy = in->cam.cy; b.cam_width = in->cam.width; b.cam_height = in->cam.height;
  b.n_pyr_levels = in->n_pyr_levels; b.align_max_iter = in->align_max_iter; b.max_epi_search_steps = in->max_epi_search_steps;
  b.edgelet_filtering = in->edgelet_filtering; b.edgelet_max_angle = in->edgelet_max_angle;
  b.px_error_angle = std::atan(in->px_noise / (2.0 * std::fabs(in->cam.fx))) * 2.0;   // depth_filter.cpp:279-280 (host libm, like the reference)
  b.convergence_sigma2_thresh = in->convergence_sigma2_thresh;
  b.n_pt = np; b.n_seg = ns;
  b.frame_T = dd + o_T; b.frame_slot = di + o_slot;
  b.pt_ref_frame = di + o_prf; b.pt_cur_frame = di + o_pcf; b.pt_level = di + o_plv; b.pt_px = dd + o_ppx; b.pt_f = dd + o_pf;
  b.pt_grad = in->pt_grad ? dd + o_pg : nullptr; b.pt_type = reinterpret_cast<const uint8_t*>(din + dbytes + ibytes + fbytes);
  b.pt_a = df + o_pa; b.pt_b = df + o_pb; b.pt_mu = df + o_pmu; b.pt_z_range = df + o_pzr; b.pt_sigma2 = df + o_ps2;
  b.seg_ref_frame = di + o_srf; b.seg_cur_frame = di + o_scf; b.seg_level = di + o_slv;
  b.seg_px = dd + o_spx; b.seg_f = dd + o_sf0; b.seg_sf = dd + o_ssf; b.seg_ef = dd + o_sef;
  b.seg_a = df + o_sa; b.seg_b = df + o_sb; b.seg_mu_s = df + o_smus; b.seg_mu_e = df + o_smue; b.seg_z_range_s = df + o_szrs;
  b.seg_z_range_e = df + o_szre; b.seg_sigma2_s = df + o_ss2s; b.seg_sigma2_e = df + o_ss2e;
  b.o_pt_xyz = od; b.o_pt_px = od + NP * 3; b.o_pt_depth = od + NP * 5;
  double* ods = od + NP * 6;
  b.o_seg_xyz_s = ods; b.o_seg_xyz_e = ods + NS * 3; b.o_seg_depth_s = ods + NS * 6; b.o_seg_depth_e = ods + NS * 7;
  b.o_pt_a = of; b.o_pt_b = of + NP; b.o_pt_mu = of + NP * 2; b.o_pt_sigma2 = of + NP * 3;
  float* ofs = of + NP * 4;
  b.o_seg_a = ofs; b.o_seg_b = ofs + NS; b.o_seg_mu_s = ofs + NS * 2; b.o_seg_mu_e = ofs + NS * 3; b.o_seg_sigma2_s = ofs + NS * 4; b.o_seg_sigma2_e = ofs + NS * 5;
  b.o_pt_status = oi; b.o_seg_status = oi + NP;
  {
    EventPair ep{}; prof_begin(c, PLSVO_K_SEEDS, &ep);
    HIP_TRY(c, launch_update_seeds(b, c->stream));
    prof_end(c, PLSVO_K_SEEDS, &ep);
  }
  std::vector<char> h(od_b + of_b + oi_b);
  HIP_TRY(c, hipMemcpyAsync(h.data(), dout, h.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const double* hd = reinterpret_cast<const double*>(h.data());
  const float* hf = reinterpret_cast<const float*>(h.data() + od_b);
  const int* hi = reinterpret_cast<const int*>(h.data() + od_b + of_b);
  auto cpd = [&](double* dst, const double* src, size_t k) { if (dst && k) memcpy(dst, src, k * sizeof(double)); };
  auto cpf = [&](float* dst, const float* src, size_t k) { if (dst && k) memcpy(dst, src, k * sizeof(float)); };
  cpd(out->pt_xyz_world, hd, NP * 3); cpd(out->pt_px_cur, hd + NP * 3, NP * 2); cpd(out->pt_depth, hd + NP * 5, NP);
  const double* hds = hd + NP * 6;
  cpd(out->seg_xyz_world_s, hds, NS * 3); cpd(out->seg_xyz_world_e, hds + NS * 3, NS * 3); cpd(out->seg_depth_s, hds + NS * 6, NS); cpd(out->seg_depth_e, hds + NS * 7, NS);
  cpf(out->pt_a, hf, NP); cpf(out->pt_b, hf + NP, NP); cpf(out->pt_mu, hf + NP * 2, NP); cpf(out->pt_sigma2, hf + NP * 3, NP);
  const float* hfs = hf + NP * 4;
  cpf(out->seg_a, hfs, NS); cpf(out->seg_b, hfs + NS, NS); cpf(out->seg_mu_s, hfs + NS * 2, NS); cpf(out->seg_mu_e, hfs + NS * 3, NS);
  cpf(out->seg_sigma2_s, hfs + NS * 4, NS); cpf(out->seg_sigma2_e, hfs + NS * 5, NS);
  if (out->pt_status && np) memcpy(out->pt_status, hi, NP * sizeof(int));
  if (out->seg_status && ns) memcpy(out->seg_status, hi + NP, NS * sizeof(int));
  return PLSVO_OK;
}

// ---- multi-GPU gather ------------------------------------------------------------------------------
// which resident state the records come from, and how many there are -- decided BEFORE anything is sized or launched
namespace {
struct RecordSource { const AlignStateDev* ast = nullptr; const PoseStateDev* pst = nullptr; int n = 0; const char* why_not = nullptr; };
RecordSource pick_record_source(plsvo_ctx* c) {
  RecordSource r;
  if (c->ch_staged && c->a_staged && c->a_n == c->ch_n) {   // the resident frame step: its own pose-optimisation state
    if (c->ch_run_seq == 0) { r.why_not = "pack_pose_records: the staged frame step has not run"; return r; }
    r.ast = c->a_d_state.as<AlignStateDev>(); r.pst = c->ch_d_state.as<PoseStateDev>(); r.n = c->ch_n;
    return r;
  }
  // both batches when they describe the same streams (same size); otherwise the one that ran last
  const bool use_a = c->a_staged && c->a_run_seq > 0, use_p = c->p_staged && c->p_run_seq > 0;
  const bool both = use_a && use_p && c->a_n == c->p_n;
  if (use_a && (both || !use_p || c->a_run_seq > c->p_run_seq)) { r.ast = c->a_d_state.as<AlignStateDev>(); r.n = c->a_n; }
  if (use_p && (both || !use_a || c->p_run_seq > c->a_run_seq)) { r.pst = c->p_d_state.as<PoseStateDev>(); r.n = c->p_n; }
  if (!r.ast && !r.pst) r.why_not = "pack_pose_records: no staged batch has run";
  return r;
}
}  // namespace

extern "C" int plsvo_pack_pose_records(plsvo_ctx* c, plsvo_pose_record* d_dst, int* n_out) {
  CTX_CHECK(c);
  if (!d_dst) return fail(c, PLSVO_E_INVALID, "pack_pose_records: null destination");
  const RecordSource src = pick_record_source(c);
  if (src.why_not) return fail(c, PLSVO_E_STATE, src.why_not);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, launch_pack_pose_records(src.ast, src.pst, src.n, d_dst, c->stream));
  if (n_out) *n_out = src.n;
  return PLSVO_OK;
}

extern "C" int plsvo_fetch_pose_records(plsvo_ctx* c, int n, plsvo_pose_record* out) {
  CTX_CHECK(c);
  if (!out || n <= 0) return fail(c, PLSVO_E_INVALID, "fetch_pose_records: bad arguments");
  const RecordSource src = pick_record_source(c);
  if (src.why_not) return fail(c, PLSVO_E_STATE, src.why_not);
  // (the pack kernel writes one record per RESIDENT stream: a caller's n that is not that count is rejected before the buffer is sized)
  if (src.n != n) return fail(c, PLSVO_E_INVALID, "fetch_pose_records: n does not match the resident batch");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, c->rec_d.ensure((size_t)n * sizeof(plsvo_pose_record)));
  HIP_TRY(c, launch_pack_pose_records(src.ast, src.pst, src.n, c->rec_d.as<plsvo_pose_record>(), c->stream));
  HIP_TRY(c, hipMemcpyAsync(out, c->rec_d.p, (size_t)n * sizeof(plsvo_pose_record), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PLSVO_OK;
}

extern "C" int plsvo_gather_poses(plsvo_ctx* c, void* rccl_comm, const plsvo_pose_record* d_local, int n_local, plsvo_pose_record* d_all) {
  CTX_CHECK(c);
  if (!rccl_comm || !d_local || !d_all || n_local <= 0) return fail(c, PLSVO_E_INVALID, "gather_poses: bad arguments");
  HIP_TRY(c, hipSetDevice(c->device));
  static_assert(sizeof(plsvo_pose_record) == 96, "plsvo_pose_record is a 96-byte wire record");
  ncclResult_t r = ncclAllGather(d_local, d_all, (size_t)n_local * (sizeof(plsvo_pose_record) / sizeof(double)), ncclDouble,
                                 reinterpret_cast<ncclComm_t>(rccl_comm), c->stream);
  if (r != ncclSuccess) return fail(c, PLSVO_E_RCCL, std::string("ncclAllGather: ") + ncclGetErrorString(r));
  return PLSVO_OK;
}

// ---- timing ------------------------------------------------------------------------------------------
extern "C" int plsvo_hip_set_profiling(plsvo_ctx* c, int enable) { CTX_CHECK(c); c->profiling = enable != 0; return PLSVO_OK; }
extern "C" int plsvo_hip_kernel_time(plsvo_ctx* c, int k, double* total_ms, int64_t* launches) {
  CTX_CHECK(c);
  if (k < 0 || k >= PLSVO_K_COUNT) return fail(c, PLSVO_E_INVALID, "kernel_time: bad kernel family");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  prof_collect(c);
  if (total_ms) *total_ms = c->ev_ms[k];
  if (launches) *launches = c->ev_launches[k];
  return PLSVO_OK;
}
extern "C" int plsvo_hip_reset_profiling(plsvo_ctx* c) {
  CTX_CHECK(c);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  prof_collect(c);
  for (int k = 0; k < PLSVO_K_COUNT; ++k) { c->ev_ms[k] = 0.0; c->ev_launches[k] = 0; }
  return PLSVO_OK;
}
