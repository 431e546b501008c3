// plsvo_capi.hip -- implementation of the C ABI declared in include/plsvo_hip.h.
// Host side only: context, HBM buffers, staging of flattened features, kernel launches, result fetch,
// hipEvent timing, RCCL gather.  All device work is enqueued on the ctx stream; nothing here computes
// any part of the hot path on the CPU (there is no fallback).
#include <dlfcn.h>
#include <rccl/rccl.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "capi_ctx.hpp"
#include "plsvo_math.hpp"
#include "poseopt_refill.hpp"
#include "poseopt_select.hpp"

static thread_local std::string g_create_error;

// ---- profiling helpers ----------------------------------------------------------------------
void prof_begin(plsvo_ctx* c, int k, EventPair* ep) {
  if (!c->profiling) return;
  if (!c->ev_pool.empty()) { *ep = c->ev_pool.back(); c->ev_pool.pop_back(); }
  else { (void)hipEventCreate(&ep->a); (void)hipEventCreate(&ep->b); }
  (void)hipEventRecord(ep->a, c->stream);
  (void)k;
}
void prof_end(plsvo_ctx* c, int k, EventPair* ep) {
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
  if (const char* s = getenv("PLSVO_ALIGN_STATIC_SOLVE")) c->opt_align_static_solve = atoi(s) != 0;
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
  c->a_d_tailflag.release(); c->a_d_alive_tail.release(); c->a_d_xbuf.release(); c->a_order.release(); c->p_order.release();
  c->p_d_carry.release(); c->p_d_refill_next.release();
  c->aj_d_batch.release(); c->aj_d_in.release(); c->aj_d_out.release(); c->aj_d_order.release(); c->tg_d_in.release(); c->tg_d_out.release(); c->aj_d_kf_in.release();
  for (DevBuf* b : { &c->cd_d_blob, &c->cd_d_work, &c->cd_d_run, &c->cd_d_kfcount, &c->ck_d_keypts, &c->ck_d_in, &c->ck_d_upkeep, &c->ck_d_work, &c->ck_d_dec_in, &c->ck_d_dec,&c->ci_d_work, &c->ci_d_in, &c->ci_d_plan, &c->ci_d_pos, &c->co_d_key, &c->co_d_in, &c->co_d_rep, &c->cn_d_in, &c->cc_d_in, &c->cc_d_work, &c->sd_d_tab, &c->sd_d_work, &c->sd_d_in, &c->cs_d_q,
                     &c->cs_d_work, &c->cs_d_order, &c->pyr_slab, &c->pyr_tiled, &c->pyr_upload, &c->a_d_blob, &c->a_d_state, &c->a_d_alive, &c->a_d_pxyz, &c->a_d_puv,
                     &c->a_d_cref, &c->a_d_chi, &c->a_d_log, &c->a_d_poses, &c->p_d_blob, &c->p_d_log, &c->s_d_in, &c->s_d_out, &c->ch_d_blob, &c->ch_d_work,
                     &c->ch_d_po, &c->rec_d }) b->release();
  c->p_w.release(); c->ch_w.release(); c->cs_w.release();
  for (auto& r : c->rect) r.map.release();
  c->det_keys.release(); c->det_occ.release(); c->det_corners.release(); c->det_counts.release(); c->det_stage.release(); c->sk_d_occ.release(); c->sk_d_slots.release(); c->sk_d_report.release();
  c->kl_d_store.release(); c->kl_d_lists.release(); c->kl_d_in.release(); c->kl_d_diag.release();
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
  if (option == PLSVO_OPT_ALIGN_STATIC_SOLVE) {
    if (value != 0 && value != 1) return fail(c, PLSVO_E_INVALID, "set_option: the alignment's static-order solve is 0 (pivot search in every elimination step) or 1 (pivot order sorted once, search on ties and NaN only)");
    c->opt_align_static_solve = value != 0;
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
  for (int l = 1; l < c->pyr.n_levels; ++l)
    HIP_TRY_TIMED(c, PLSVO_K_HALFSAMPLE, launch_halfsample(base + c->pyr.off[l - 1], c->pyr.slot_bytes, c->pyr.w[l - 1], c->pyr.h[l - 1], c->pyr.w[l - 1],
                                                          base + c->pyr.off[l], c->pyr.slot_bytes, n, rounding, c->stream));
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

// checks shared by the detect entry points (and plsvo_seeds_keyframe_detect, capi_candidates.hip): nothing has been enqueued or written when one fails
int detect_check_params(plsvo_ctx* c, int n, const plsvo_detect_params* p, const char* what, int* cols, int* rows) {
  if (p->n_levels < 1 || p->n_levels > c->pyr.n_levels) return fail(c, PLSVO_E_INVALID, std::string(what) + ": n_levels outside the configured pyramid");
  if (p->cell_size < 1) return fail(c, PLSVO_E_INVALID, std::string(what) + ": cell_size < 1");
  if (c->pyr.w[0] > 8191 || c->pyr.h[0] > 8191) return fail(c, PLSVO_E_INVALID, std::string(what) + ": image wider or higher than 8191 (13 bits per coordinate of a cell key)");
  if (c->pyr.w[p->n_levels - 1] < 7 || c->pyr.h[p->n_levels - 1] < 7) return fail(c, PLSVO_E_INVALID, std::string(what) + ": a level smaller than 7 x 7");
  if (p->fast_threshold < 1 || p->fast_threshold > 254) return fail(c, PLSVO_E_INVALID, std::string(what) + ": fast_threshold outside 1..254");
  const double t = p->detection_threshold;
  if (!std::isfinite(t) || t < 0.0 || (double)(float)t != t) return fail(c, PLSVO_E_INVALID, std::string(what) + ": detection_threshold negative, not finite or not a float");
  if (plsvo_detect_grid(c->pyr.w[0], c->pyr.h[0], p->cell_size, cols, rows) != PLSVO_OK || (long long)*cols * *rows * std::max(n, 1) > INT32_MAX)
    return fail(c, PLSVO_E_INVALID, std::string(what) + ": grid too large");
  return PLSVO_OK;
}

static int detect_check(plsvo_ctx* c, int first_slot, int n, const plsvo_detect_params* p, const void* corners, const void* counts, const char* what,
                        int* cols, int* rows) {
  if (!c->pyr.base) return fail(c, PLSVO_E_STATE, std::string(what) + ": pyramids not configured");
  if (!p || !corners || !counts) return fail(c, PLSVO_E_INVALID, std::string(what) + ": NULL params, corners or counts");
  if (n <= 0 || first_slot < 0 || first_slot > c->pyr.n_slots - n) return fail(c, PLSVO_E_INVALID, std::string(what) + ": slot range out of bounds");
  return detect_check_params(c, n, p, what, cols, rows);
}

int detect_enqueue_keys(plsvo_ctx* c, int first_slot, const int* d_slot_table, int n, const plsvo_detect_params* p, int cells, int cols, const uint8_t* d_occ) {
  const size_t key_bytes = (size_t)n * cells * sizeof(unsigned long long);
  if (key_bytes > c->det_keys.cap) {   // a new buffer starts armed; every compaction (and every seed start) leaves it armed
    HIP_TRY(c, c->det_keys.ensure(key_bytes));
    HIP_TRY(c, hipMemsetAsync(c->det_keys.p, 0, c->det_keys.cap, c->stream));
  }
  DetectLaunch a{};
  a.pyr = c->pyr_slab.as<uint8_t>() + (size_t)first_slot * c->pyr.slot_bytes;
  a.slot_bytes = c->pyr.slot_bytes;
  detect_fill_levels(c, 0, p->n_levels - 1, &a);
  a.fast_b = p->fast_threshold; a.thr = (float)p->detection_threshold;
  a.cell = p->cell_size; a.cols = cols; a.n_cells = cells;
  a.occupancy = d_occ; a.keys = c->det_keys.as<unsigned long long>(); a.slot_table = d_slot_table;
  HIP_TRY(c, launch_detect_fast(a, n, c->stream));
  return PLSVO_OK;
}

static int detect_enqueue(plsvo_ctx* c, int first_slot, int n, const plsvo_detect_params* p, int cells, int cols, const uint8_t* d_occ,
                          plsvo_corner* d_corners, int32_t* d_counts) {
  if (const int rc = detect_enqueue_keys(c, first_slot, nullptr, n, p, cells, cols, d_occ)) return rc;
  HIP_TRY(c, launch_detect_compact(c->det_keys.as<unsigned long long>(), cells, d_corners, d_counts, n, c->stream));
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
  Readback rb;
  rb.add(c->det_counts.p, (size_t)n * sizeof(int32_t));
  if ((rc = rb.wait(c))) return rc;
  const int32_t* const cnt = rb.at<int32_t>(0);
  for (int i = 0; i < n; ++i) {
    if (cnt[i] < 0 || cnt[i] > cells) return fail(c, PLSVO_E_HIP, "detect_fast: corrupt count");
    if (cnt[i] > 0)
      HIP_TRY(c, hipMemcpyAsync(corners + (size_t)i * cells, c->det_corners.as<plsvo_corner>() + (size_t)i * cells, (size_t)cnt[i] * sizeof(plsvo_corner),
                                hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  memcpy(counts, cnt, (size_t)n * sizeof(int32_t));
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

extern "C" int plsvo_align_stage(plsvo_ctx* c, int n, const plsvo_align_in* in) {
  CTX_CHECK(c);
  if (n <= 0 || !in) return fail(c, PLSVO_E_INVALID, "align_stage: bad arguments");
  if (!c->pyr.base) return fail(c, PLSVO_E_STATE, "align_stage: pyramids not configured");
  HIP_TRY(c, hipSetDevice(c->device));
  c->a_staged = false;
  c->aj_built = false;    // (a batch built on the device, plsvo_candidates_align_build, is replaced like any other)
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
  b.pair = 0; b.xseq0 = 0; b.xbuf = nullptr; b.work_key = nullptr; b.tail_n = 0; b.static_solve = 1; b.tail_flag = nullptr; b.seg_alive_tail = nullptr;   // (plsvo_align_run decides)
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
int pose_opt_threads(const plsvo_ctx* c, int n, long feats) {
  const int cus = c->cu_count > 0 ? c->cu_count : 256;
  const int threads = n <= 2 * cus ? 256 : (feats <= 580l * n ? 16 : 64);
  return c->env_poseopt_threads ? c->env_poseopt_threads : threads;
}

void pick_align_config(const plsvo_ctx* c, int n_jobs, int cap, int scap, int max_pts, int* threads, size_t* lds, int* chi_lds_pts) {
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

// the launch configuration of the staged batch: the slot capacities the host mirrors hold, and pick_align_config on them
static void staged_align_config(const plsvo_ctx* c, int* cap, int* scap, int* threads, size_t* lds, int* chi_lds_pts) {
  *cap = 4;
  if (c->a_gmax >= c->a_gmin && c->a_gmax >= 0) for (int l = c->a_gmin; l <= c->a_gmax; ++l) *cap = std::max(*cap, c->a_cap[l]);
  *scap = (c->a_scap + 3) & ~3;
  int max_pts = 0;
  for (const AlignJobDev& J : c->a_jobs) max_pts = std::max(max_pts, J.n_pts);
  pick_align_config(c, c->a_n, *cap, *scap, max_pts, threads, lds, chi_lds_pts);
}
// diagnostic (measurements): what plsvo_align_run would launch the staged batch with
extern "C" int plsvo_align_launch_shape(plsvo_ctx* c, int32_t* threads, uint64_t* lds_bytes) {
  CTX_CHECK(c);
  if (!c->a_staged) return fail(c, PLSVO_E_STATE, "align_launch_shape: no staged batch");
  if (!threads || !lds_bytes) return fail(c, PLSVO_E_INVALID, "align_launch_shape: NULL output");
  int cap, scap, t, chi; size_t lds;
  staged_align_config(c, &cap, &scap, &t, &lds, &chi);
  *threads = t; *lds_bytes = (uint64_t)lds;
  return PLSVO_OK;
}

constexpr int kAlignTailRounds = 2;   // tail set of the split, in rounds of resident workgroups (measured: DESIGN.md 3.1)
extern "C" int plsvo_align_run(plsvo_ctx* c) {
  CTX_CHECK(c);
  RoctxRange range("sparse_img_align");
  if (!c->a_staged) return fail(c, PLSVO_E_STATE, "align_run: no staged batch");
  HIP_TRY(c, hipSetDevice(c->device));
  // one launch: the workgroup of a job resets its solver state, runs its levels and writes its pose
  // (jobs without features, src/sparse_img_align.cpp:58-62, only do the first and the last)
  const bool have_levels = c->a_gmax >= c->a_gmin && c->a_gmax >= 0;
  int cap, scap, threads, chi_lds_pts; size_t lds;
  staged_align_config(c, &cap, &scap, &threads, &lds, &chi_lds_pts);
  c->a_b.chi_lds_pts = chi_lds_pts;
  if (lds > c->lds_per_block) return fail(c, PLSVO_E_CAPACITY, "align_run: slot tables do not fit in LDS (too many features in one job)");
  if (threads <= 64 && c->tiled_stale_count > 0) {   // the one-wave-per-frame shape reads the tiled mirror: bring the uploaded slots' tiles up to date first
    std::vector<int> slots;
    slots.reserve(2 * c->a_jobs.size());
    for (const AlignJobDev& J : c->a_jobs) { slots.push_back(J.ref_slot); slots.push_back(J.cur_slot); }
    if (c->aj_built) for (const std::vector<int>& v : c->aj_kf_slots) slots.insert(slots.end(), v.begin(), v.end());   // (a reference keyframe picked on the device)
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
  c->a_b.static_solve = c->opt_align_static_solve ? 1 : 0;
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
  if (reorder && !(c->a_b.work_key = c->a_order.arm(c, c->a_n))) return PLSVO_E_HIP;
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
    HIP_TRY_TIMED(c, PLSVO_K_ALIGN_LEVEL, launch_align_levels(c->a_b, cap, scap, have_levels ? c->a_gmax : 0, have_levels ? c->a_gmin : 0, 1, threads, lds, c->stream));
    // a batch with more frames than resident slots: the NEXT launch of this staged batch starts its frames longest-first by what they cost in
    // this one (LaunchOrder); a launch that does not reorder keeps the order it has
    if (reorder) {
      const int* const next_order = c->a_order.sort(c, c->a_n, 7);
      if (!next_order) return PLSVO_E_HIP;
      c->a_b.order = next_order;
    }
  } else {
    for (int level = c->a_gmax; level >= c->a_gmin; --level)   // debug: one launch per level, state carried in HBM
      HIP_TRY_TIMED(c, PLSVO_K_ALIGN_LEVEL, launch_align_levels(c->a_b, cap, scap, level, level, level == c->a_gmax ? 1 : 0, threads, lds, c->stream));
  }
  c->a_run_seq = ++c->run_seq; c->a_run_threads = threads;
  return PLSVO_OK;
}

extern "C" int plsvo_align_fetch(plsvo_ctx* c, int n, plsvo_align_out* out) {
  CTX_CHECK(c);
  if (!c->a_staged) return fail(c, PLSVO_E_STATE, "align_fetch: no staged batch");
  if (n != c->a_n || !out) return fail(c, PLSVO_E_INVALID, "align_fetch: n does not match the staged batch");
  HIP_TRY(c, hipSetDevice(c->device));
  Readback rb;
  const int r_st = rb.add(c->a_d_state.p, (size_t)n * sizeof(AlignStateDev)), r_alive = rb.add(c->a_d_alive.p, (size_t)std::max(c->a_total_seg, 0));
  if (const int rc = rb.wait(c)) return rc;
  const AlignStateDev* const st = rb.at<AlignStateDev>(r_st);
  const uint8_t* const alive = rb.at<uint8_t>(r_alive);
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

// Diagnostic view of a level's set-up (tests): what the last plsvo_align_run left in the job's patch slots -- the 64-byte records and the
// reference pixel positions of the LAST level it ran (every level's set-up writes the same slots).  Two plain copies behind the stream.
extern "C" int plsvo_align_fetch_records(plsvo_ctx* c, int job, int n_slots, unsigned char* records, float* uvref) {
  CTX_CHECK(c);
  if (!c->a_staged || c->a_run_seq == 0) return fail(c, PLSVO_E_STATE, "fetch_records: the staged batch has not run");
  if (c->a_run_threads >= kQuadMinThreads) return fail(c, PLSVO_E_STATE, "fetch_records: the last run used a latency shape, which keeps float rows instead of records");
  if (job < 0 || job >= c->a_n || n_slots < 0 || n_slots > c->a_jobs[(size_t)job].patch_cap || !records || !uvref)
    return fail(c, PLSVO_E_INVALID, "fetch_records: bad arguments (n_slots is bounded by the job's slot allocation)");
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t p0 = (size_t)c->a_jobs[(size_t)job].patch_off;
  if (n_slots > 0) {
    HIP_TRY(c, hipMemcpyAsync(records, c->a_d_cref.as<unsigned char>() + p0 * 64, (size_t)n_slots * 64, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(uvref, c->a_d_puv.as<float>() + p0 * 2, (size_t)n_slots * 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PLSVO_OK;
}

extern "C" const double* plsvo_align_poses_dev(plsvo_ctx* c) { return (c && c->a_staged) ? c->a_d_poses.as<double>() : nullptr; }

// the diagnostics below sum fields over a staged batch's state array (AlignStateDev / PoseStateDev): fetch its n states, visit each
template <typename S, typename F>
static int for_each_state(plsvo_ctx* c, const DevBuf& states, int n, F visit) {
  HIP_TRY(c, hipSetDevice(c->device));
  Readback rb;
  rb.add(states.p, (size_t)n * sizeof(S));
  if (const int rc = rb.wait(c)) return rc;
  for (int j = 0; j < n; ++j) visit(rb.at<S>(0)[j]);
  return PLSVO_OK;
}

// debug: per-phase s_memtime ticks summed over the batch (all zero unless built with -DPLSVO_TIMING); not in the public header
extern "C" int plsvo_align_phase_ticks(plsvo_ctx* c, unsigned long long* out8) {
  CTX_CHECK(c);
  if (!c->a_staged || !out8) return fail(c, PLSVO_E_STATE, "phase_ticks: no staged batch");
  std::fill(out8, out8 + 8, 0ull);
  return for_each_state<AlignStateDev>(c, c->a_d_state, c->a_n, [&](const AlignStateDev& s) { for (int k = 0; k < 8; ++k) out8[k] += s.phase_ticks[k]; });
}

extern "C" int plsvo_poseopt_phase_ticks(plsvo_ctx* c, unsigned long long* out8) {
  CTX_CHECK(c);
  if (!c->p_staged || !out8) return fail(c, PLSVO_E_STATE, "phase_ticks: no staged batch");
  std::fill(out8, out8 + 8, 0ull);
  return for_each_state<PoseStateDev>(c, c->p_w.state, c->p_n, [&](const PoseStateDev& s) { for (int k = 0; k < 8; ++k) out8[k] += s.phase_ticks[k]; });
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
  uint64_t pl = 0, pi = 0;
  if (const int rc = for_each_state<AlignStateDev>(c, c->a_d_state, c->a_n, [&](const AlignStateDev& s) { pl += s.patch_levels; pi += s.patch_iters; })) return rc;
  if (patch_levels) *patch_levels = pl;
  if (patch_iters) *patch_iters = pi;
  return PLSVO_OK;
}

extern "C" int plsvo_align_work_points(plsvo_ctx* c, uint64_t* point_patch_iters) {
  CTX_CHECK(c);
  if (!c->a_staged) return fail(c, PLSVO_E_STATE, "align_work_points: no staged batch");
  uint64_t n = 0;
  if (const int rc = for_each_state<AlignStateDev>(c, c->a_d_state, c->a_n, [&](const AlignStateDev& s) { n += s.patch_iters_pt; })) return rc;
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
  uint64_t it = 0, t = 0, un = 0;
  if (const int rc = for_each_state<AlignStateDev>(c, c->a_d_state, c->a_n, [&](const AlignStateDev& s) {
        t += (uint64_t)s.chi2_ties; un += (uint64_t)s.chi2_unarmed; for (int l = 0; l < PLSVO_MAX_LEVELS; ++l) it += (uint64_t)s.iters[l]; })) return rc;
  if (iterations) *iterations = it;
  if (ties) *ties = t;
  if (near_ties_without_terms) *near_ties_without_terms = un;
  return PLSVO_OK;
}

// ---- pose optimisation ---------------------------------------------------------------------------
// The one sizing of a pose-optimiser work set: each feature count floored at 1, the scratch by the SUM of the two floored counts (the candidates' rule).
// The staged batch and the frame step sized the scratch by max(n_pt + n_seg, 1), never more than that sum, and the masks as here: no buffer shrinks.
int PoseWork::ensure(plsvo_ctx* c, size_t n_jobs, size_t n_pt, size_t n_seg) {
  const size_t np = std::max(n_pt, (size_t)1), ns = std::max(n_seg, (size_t)1), nft = np + ns;
  HIP_TRY(c, ptkeep.ensure(np));
  HIP_TRY(c, segkeep.ensure(ns));
  HIP_TRY(c, s32.ensure(nft * sizeof(float)));
  HIP_TRY(c, s64.ensure(nft * 5 * sizeof(double)));
  HIP_TRY(c, state.ensure(n_jobs * sizeof(PoseStateDev)));
  HIP_TRY(c, poses.ensure(n_jobs * 7 * sizeof(double)));
  return PLSVO_OK;
}

void pose_state_to_out(const PoseStateDev& s, plsvo_poseopt_out& o) {
  uint8_t* const pko = o.pt_keep; uint8_t* const sko = o.seg_keep;   // the caller's buffers: each fetch fills them from its own layout
  memset(&o, 0, sizeof(o));
  o.pt_keep = pko; o.seg_keep = sko;
  for (int k = 0; k < 7; ++k) o.T_f_w[k] = s.T[k];
  for (int k = 0; k < 36; ++k) o.cov[k] = s.cov[k];
  o.estimated_scale = s.estimated_scale; o.error_init = s.error_init; o.error_final = s.error_final;
  o.num_obs_pt = s.num_obs_pt; o.num_obs_ls = s.num_obs_ls;
  o.iters = s.iters; o.iters_ref = s.iters_ref; o.status = s.status;
}

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
  const size_t npt = plev.size(), nsg = slev.size();
  if ((rc = c->p_w.ensure(c, (size_t)n, npt, nsg))) return rc;
  if (c->p_trace_cap > 0) HIP_TRY(c, c->p_d_log.ensure((size_t)n * c->p_trace_cap * sizeof(plsvo_poseopt_iterlog)));
  PoseBatchDev& b = c->p_b;
  uint8_t* const base = c->p_d_blob.as<uint8_t>();
  b.jobs = reinterpret_cast<const PoseJobDev*>(base + o_jobs); c->p_w.bind(b);
  b.pt_f = reinterpret_cast<const double*>(base + o_f); b.pt_pos = reinterpret_cast<const double*>(base + o_pos);
  b.pt_level = reinterpret_cast<const int*>(base + o_plev);
  b.seg_line = reinterpret_cast<const double*>(base + o_line); b.seg_spos = reinterpret_cast<const double*>(base + o_spos);
  b.seg_epos = reinterpret_cast<const double*>(base + o_epos); b.seg_level = reinterpret_cast<const int*>(base + o_slev);
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
  if (!reorder) c->p_b.order = nullptr;
  else if (!(c->p_b.work_key = c->p_order.arm(c, c->p_n))) return PLSVO_E_HIP;
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
  if (refill) {
    const int wgs = (c->p_n + 3) / 4;
    const int gn_grid = std::max(1, std::min(wgs, c->env_poseopt_refill_waves > 0 ? c->env_poseopt_refill_waves : resident_wgs));
    HIP_TRY(c, c->p_d_carry.ensure((size_t)c->p_n * sizeof(PoseRefillCarry)));
    HIP_TRY(c, c->p_d_refill_next.ensure(16));
    const PoseRefillDev q{ c->p_d_carry.as<PoseRefillCarry>(), c->p_d_refill_next.as<int>() };
    const auto rearm_then_launch = [&]() -> hipError_t {   // the queue is re-armed ahead of every launch
      const hipError_t e = hipMemsetAsync(c->p_d_refill_next.p, 0, 16, c->stream);
      return e != hipSuccess ? e : launch_pose_opt_refill(c->p_b, q, c->p_w.poses.as<double>(), gn_grid, c->opt_poseopt_select ? 1 : 0, c->stream);
    };
    HIP_TRY_TIMED(c, PLSVO_K_POSEOPT, rearm_then_launch());
    c->p_refill_frames = c->p_n;
  } else {
    HIP_TRY_TIMED(c, PLSVO_K_POSEOPT, launch_pose_opt(c->p_b, c->p_w.poses.as<double>(), threads, c->opt_poseopt_select ? 1 : 0, c->stream));
  }
  c->p_run_seq = ++c->run_seq;   // (a launch that failed has returned above: the sequence counts launches that were enqueued)
  if (reorder) {
    const int* const next_order = c->p_order.sort(c, c->p_n, c->p_key_shift);
    if (!next_order) return PLSVO_E_HIP;
    c->p_b.order = next_order;
  }
  return PLSVO_OK;
}

extern "C" int plsvo_poseopt_fetch(plsvo_ctx* c, int n, plsvo_poseopt_out* out) {
  CTX_CHECK(c);
  if (!c->p_staged) return fail(c, PLSVO_E_STATE, "poseopt_fetch: no staged batch");
  if (n != c->p_n || !out) return fail(c, PLSVO_E_INVALID, "poseopt_fetch: n does not match the staged batch");
  HIP_TRY(c, hipSetDevice(c->device));
  Readback rb;
  const int r_st = rb.add(c->p_w.state.p, (size_t)n * sizeof(PoseStateDev)), r_pk = rb.add(c->p_w.ptkeep.p, (size_t)std::max(c->p_total_pt, 0)),
            r_sk = rb.add(c->p_w.segkeep.p, (size_t)std::max(c->p_total_seg, 0));
  if (const int rc = rb.wait(c)) return rc;
  const PoseStateDev* const st = rb.at<PoseStateDev>(r_st);
  const uint8_t* const pk = rb.at<uint8_t>(r_pk); const uint8_t* const sk = rb.at<uint8_t>(r_sk);
  for (int j = 0; j < n; ++j) {
    const PoseStateDev& s = st[(size_t)j];
    const PoseJobDev& J = c->p_jobs[(size_t)j];
    plsvo_poseopt_out& o = out[j];
    pose_state_to_out(s, o);
    if (o.pt_keep && J.n_pts > 0) memcpy(o.pt_keep, pk + J.pt_off, (size_t)J.n_pts);
    if (o.seg_keep && J.n_seg > 0) memcpy(o.seg_keep, sk + J.seg_off, (size_t)J.n_seg);
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
  const size_t width = (size_t)in->bits / 8, NR = (size_t)nr;
  Blob blob;
  const size_t b_pat = blob.add(static_cast<const uint8_t*>(in->patterns), (size_t)in->n_patterns * width), b_off = blob.add(in->row_off, NR),
               b_n = blob.add(in->row_n, NR), b_k = blob.add(in->row_k, NR), b_act = blob.add(in->row_active, NR);
  if (const int rc = upload_blob(c, c->s_d_in, blob)) return rc;
  Carver cv;
  const size_t o_sel = cv.take<uint8_t>(NR * width), o_path = cv.take<int>(NR);
  HIP_TRY(c, c->s_d_out.ensure(cv.off + 256));
  HIP_TRY(c, hipMemsetAsync(c->s_d_out.p, 0, cv.off, c->stream));
  RowSelectDev t{};
  t.patterns = Blob::dev<uint8_t>(c->s_d_in, b_pat); t.row_off = Blob::dev<long long>(c->s_d_in, b_off); t.row_n = Blob::dev<int>(c->s_d_in, b_n);
  t.row_k = Blob::dev<int>(c->s_d_in, b_k); t.row_active = Blob::dev<uint8_t>(c->s_d_in, b_act);
  t.selected = Carver::dev<uint8_t>(c->s_d_out, o_sel); t.path = Carver::dev<int>(c->s_d_out, o_path);
  t.n_rows = nr; t.bits = in->bits; t.select = c->opt_poseopt_select ? 1 : 0;
  HIP_TRY(c, launch_pose_row_select(t, c->stream));
  Readback rb;
  const int r_sel = rb.add(t.selected, NR * width), r_path = rb.add(t.path, NR * sizeof(int));
  if (const int rc = rb.wait(c)) return rc;
  memcpy(selected, rb.at<uint8_t>(r_sel), NR * width);
  memcpy(path, rb.at<int>(r_path), NR * sizeof(int));
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
  HIP_TRY(c, hipMemcpyAsync(&s, c->p_w.state.as<PoseStateDev>() + job, sizeof(s), hipMemcpyDeviceToHost, c->stream));
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

extern "C" const double* plsvo_poseopt_poses_dev(plsvo_ctx* c) { return (c && c->p_staged) ? c->p_w.poses.as<double>() : nullptr; }

extern "C" int plsvo_poseopt_copy_poses(plsvo_ctx* c, double* d_dst) {
  CTX_CHECK(c);
  if (!c->p_staged || !d_dst) return fail(c, PLSVO_E_STATE, "poseopt_copy_poses: no staged batch / null destination");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(d_dst, c->p_w.poses.p, (size_t)c->p_n * 7 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  return PLSVO_OK;
}

extern "C" int plsvo_poseopt_work(plsvo_ctx* c, uint64_t* pt_iters, uint64_t* seg_iters) {
  CTX_CHECK(c);
  if (!c->p_staged) return fail(c, PLSVO_E_STATE, "poseopt_work: no staged batch");
  uint64_t a = 0, b2 = 0;
  if (const int rc = for_each_state<PoseStateDev>(c, c->p_w.state, c->p_n, [&](const PoseStateDev& s) { a += s.pt_iters; b2 += s.seg_iters; })) return rc;
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
  // the kernel reads observations [off[i], off[i+1]) of every landmark: a table must start at 0 and never decrease (so no entry is
  // negative and none exceeds the last, which sizes the upload) -- checked here, before anything is uploaded or launched
  auto bad_offsets = [](const int32_t* off, int n) {
    if (n <= 0) return false;
    if (off[0] != 0) return true;
    for (int i = 0; i < n; ++i) if (off[i + 1] < off[i]) return true;
    return false;
  };
  if (bad_offsets(in->pt_obs_off, in->n_pts) || bad_offsets(in->seg_obs_off, in->n_seg))
    return fail(c, PLSVO_E_INVALID, "structure_optimize: observation offsets must start at 0 and not decrease");
  HIP_TRY(c, hipSetDevice(c->device));
  const int np = in->n_pts, ns = in->n_seg;
  const int npo = np > 0 ? in->pt_obs_off[np] : 0, nso = ns > 0 ? in->seg_obs_off[ns] : 0;
  if (npo < 0 || nso < 0 || (npo > 0 && (!in->pt_obs_frame || !in->pt_obs_f)) || (nso > 0 && (!in->seg_obs_frame || !in->seg_obs_sf || !in->seg_obs_ef)) ||
      ((npo > 0 || nso > 0) && (!in->frame_T || in->n_frames <= 0)))
    return fail(c, PLSVO_E_INVALID, "structure_optimize: bad observation tables");
  for (int i = 0; i < npo; ++i) if (in->pt_obs_frame[i] < 0 || in->pt_obs_frame[i] >= in->n_frames) return fail(c, PLSVO_E_INVALID, "structure_optimize: frame index out of range");
  for (int i = 0; i < nso; ++i) if (in->seg_obs_frame[i] < 0 || in->seg_obs_frame[i] >= in->n_frames) return fail(c, PLSVO_E_INVALID, "structure_optimize: frame index out of range");
  const size_t NP = (size_t)np, NS = (size_t)ns;
  Blob blob;
  const size_t b_T = blob.add(in->frame_T, (size_t)in->n_frames * 7), b_pp = blob.add(in->pt_pos, NP * 3), b_pf = blob.add(in->pt_obs_f, (size_t)npo * 3),
               b_ss = blob.add(in->seg_spos, NS * 3), b_se = blob.add(in->seg_epos, NS * 3), b_sf = blob.add(in->seg_obs_sf, (size_t)nso * 3),
               b_ef = blob.add(in->seg_obs_ef, (size_t)nso * 3), b_po = blob.add(in->pt_obs_off, np > 0 ? NP + 1 : 0), b_pfr = blob.add(in->pt_obs_frame, (size_t)npo),
               b_so = blob.add(in->seg_obs_off, ns > 0 ? NS + 1 : 0), b_sfr = blob.add(in->seg_obs_frame, (size_t)nso);
  if (const int rc = upload_blob(c, c->s_d_in, blob)) return rc;
  Carver cv;
  const size_t o_pp = cv.take<double>(NP * 3), o_ss = cv.take<double>(NS * 3), o_se = cv.take<double>(NS * 3), o_pi = cv.take<int>(NP), o_si = cv.take<int>(NS);
  HIP_TRY(c, c->s_d_out.ensure(cv.off + 256));
  const DevBuf& din = c->s_d_in; const DevBuf& dout = c->s_d_out;
  StructBatchDev s{};
  s.frame_T = Blob::dev<double>(din, b_T); s.pt_pos = Blob::dev<double>(din, b_pp); s.pt_obs_f = Blob::dev<double>(din, b_pf);
  s.seg_spos = Blob::dev<double>(din, b_ss); s.seg_epos = Blob::dev<double>(din, b_se);
  s.seg_obs_sf = Blob::dev<double>(din, b_sf); s.seg_obs_ef = Blob::dev<double>(din, b_ef);
  s.pt_obs_off = Blob::dev<int>(din, b_po); s.pt_obs_frame = Blob::dev<int>(din, b_pfr); s.seg_obs_off = Blob::dev<int>(din, b_so); s.seg_obs_frame = Blob::dev<int>(din, b_sfr);
  s.pt_pos_out = Carver::dev<double>(dout, o_pp); s.seg_spos_out = Carver::dev<double>(dout, o_ss); s.seg_epos_out = Carver::dev<double>(dout, o_se);
  s.pt_iters = Carver::dev<int>(dout, o_pi); s.seg_iters = Carver::dev<int>(dout, o_si);
  s.n_pts = np; s.n_seg = ns; s.n_iter_pts = in->n_iter_pts; s.n_iter_segs = in->n_iter_segs;
  HIP_TRY_TIMED(c, PLSVO_K_STRUCTOPT, launch_structopt(s, c->stream));
  Readback rb;
  const int r_pp = rb.add(s.pt_pos_out, NP * 3 * sizeof(double)), r_ss = rb.add(s.seg_spos_out, NS * 3 * sizeof(double)), r_se = rb.add(s.seg_epos_out, NS * 3 * sizeof(double)),
            r_pi = rb.add(s.pt_iters, NP * sizeof(int)), r_si = rb.add(s.seg_iters, NS * sizeof(int));
  if (const int rc = rb.wait(c)) return rc;
  if (out->pt_pos && np) memcpy(out->pt_pos, rb.at<double>(r_pp), NP * 3 * sizeof(double));
  if (out->seg_spos && ns) memcpy(out->seg_spos, rb.at<double>(r_ss), NS * 3 * sizeof(double));
  if (out->seg_epos && ns) memcpy(out->seg_epos, rb.at<double>(r_se), NS * 3 * sizeof(double));
  if (out->pt_iters && np) memcpy(out->pt_iters, rb.at<int>(r_pi), NP * sizeof(int));
  if (out->seg_iters && ns) memcpy(out->seg_iters, rb.at<int>(r_si), NS * sizeof(int));
  return PLSVO_OK;
}

// diagnostic view of the 3x3 solve inside structopt_kernel (tests): n systems, one lane each
extern "C" int plsvo_structure_solve3(plsvo_ctx* c, int32_t n, const double* A, const double* b, double* x) {
  CTX_CHECK(c);
  if (n < 0 || (n > 0 && (!A || !b || !x))) return fail(c, PLSVO_E_INVALID, "structure_solve3: bad arguments");
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t na = (size_t)n * 9, nb = (size_t)n * 3;
  Blob blob;
  const size_t b_A = blob.add(A, na), b_b = blob.add(b, nb);
  if (const int rc = upload_blob(c, c->s_d_in, blob)) return rc;
  HIP_TRY(c, c->s_d_out.ensure(nb * sizeof(double)));
  HIP_TRY(c, launch_structopt_solve3(Blob::dev<double>(c->s_d_in, b_A), Blob::dev<double>(c->s_d_in, b_b), c->s_d_out.as<double>(), n, c->stream));
  HIP_TRY(c, hipMemcpyAsync(x, c->s_d_out.p, nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));   // (one whole range into the caller's own buffer: a plain copy)
  HIP_TRY(c, hipStreamSynchronize(c->stream));
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
  const size_t N = (size_t)n;
  Blob blob;
  const size_t b_T = blob.add(in->frame_T, (size_t)nf * 7), b_px = blob.add(in->ref_px, N * 2), b_f = blob.add(in->ref_f, N * 3), b_g = blob.add(in->ref_grad, N * 2),   // (no ref_grad: zeros)
               b_pos = blob.add(in->pos, N * 3), b_pc = blob.add(in->px_cur, N * 2), b_slot = blob.add(in->frame_slot, (size_t)nf), b_cf = blob.add(in->cur_frame, N),
               b_rf = blob.add(in->ref_frame, N), b_lv = blob.add(in->ref_level, N), b_ty = blob.add(in->ref_type, N);
  if (const int rc = upload_blob(c, c->s_d_in, blob)) return rc;
  Carver cv;
  const size_t o_px = cv.take<double>(N * 2), o_lv = cv.take<int>(N), o_it = cv.take<int>(N), o_found = cv.take<uint8_t>(N);
  // the diagnostic view appends: A (4 doubles), then warped, staged, patch (100 bytes) per candidate
  const size_t o_A = wout ? cv.take<double>(N * 4) : 0, o_wp = wout ? cv.take<uint8_t>(N) : 0, o_st = wout ? cv.take<uint8_t>(N) : 0, o_pa = wout ? cv.take<uint8_t>(N * kWarpPatchBytes) : 0;
  HIP_TRY(c, c->s_d_out.ensure(cv.off + 256));
  const DevBuf& din = c->s_d_in; const DevBuf& dout = c->s_d_out;
  MatchBatchDev b{};
  b.pyr_base = c->pyr.base; b.slot_bytes = c->pyr.slot_bytes; b.width = c->pyr.w[0]; b.height = c->pyr.h[0];
  b.fx = in->cam.fx; b.fy = in->cam.fy; b.cx = in->cam.cx; b.cy = in->cam.cy; b.cam_width = in->cam.width; b.cam_height = in->cam.height;
  b.n = n; b.n_pyr_levels = in->n_pyr_levels; b.align_max_iter = in->align_max_iter;
  b.frame_T = Blob::dev<double>(din, b_T); b.ref_px = Blob::dev<double>(din, b_px); b.ref_f = Blob::dev<double>(din, b_f); b.ref_grad = Blob::dev<double>(din, b_g);
  b.pos = Blob::dev<double>(din, b_pos); b.px_cur = Blob::dev<double>(din, b_pc);
  b.frame_slot = Blob::dev<int>(din, b_slot); b.cur_frame = Blob::dev<int>(din, b_cf); b.ref_frame = Blob::dev<int>(din, b_rf); b.ref_level = Blob::dev<int>(din, b_lv);
  b.ref_type = Blob::dev<uint8_t>(din, b_ty);
  b.px_out = Carver::dev<double>(dout, o_px); b.search_level = Carver::dev<int>(dout, o_lv); b.n_iter = Carver::dev<int>(dout, o_it); b.found = Carver::dev<uint8_t>(dout, o_found);
  Readback rb;
  if (wout) {
    HIP_TRY(c, hipMemsetAsync(Carver::dev<uint8_t>(dout, o_A), 0, cv.off - o_A, c->stream));
    b.diag_A = Carver::dev<double>(dout, o_A);
    b.diag_warped = Carver::dev<uint8_t>(dout, o_wp); b.diag_staged = Carver::dev<uint8_t>(dout, o_st); b.diag_patch = Carver::dev<uint8_t>(dout, o_pa);
    HIP_TRY(c, launch_match_warp_patches(b, c->stream));
    const int r_A = rb.add(b.diag_A, N * 4 * sizeof(double)), r_lv = rb.add(b.search_level, N * sizeof(int)), r_wp = rb.add(b.diag_warped, N), r_st = rb.add(b.diag_staged, N),
              r_pa = rb.add(b.diag_patch, N * kWarpPatchBytes);
    if (const int rc = rb.wait(c)) return rc;
    if (wout->A) memcpy(wout->A, rb.at<double>(r_A), N * 4 * sizeof(double));
    if (wout->search_level) memcpy(wout->search_level, rb.at<int>(r_lv), N * sizeof(int));
    if (wout->warped) memcpy(wout->warped, rb.at<uint8_t>(r_wp), N);
    if (wout->staged) memcpy(wout->staged, rb.at<uint8_t>(r_st), N);
    if (wout->patch) memcpy(wout->patch, rb.at<uint8_t>(r_pa), N * kWarpPatchBytes);
    return PLSVO_OK;
  }
  HIP_TRY_TIMED(c, PLSVO_K_MATCH, launch_match_direct(b, c->stream));
  const int r_px = rb.add(b.px_out, N * 2 * sizeof(double)), r_lv = rb.add(b.search_level, N * sizeof(int)), r_it = rb.add(b.n_iter, N * sizeof(int)), r_found = rb.add(b.found, N);
  if (const int rc = rb.wait(c)) return rc;
  if (out->px_cur) memcpy(out->px_cur, rb.at<double>(r_px), N * 2 * sizeof(double));
  if (out->search_level) memcpy(out->search_level, rb.at<int>(r_lv), N * sizeof(int));
  if (out->n_iter) memcpy(out->n_iter, rb.at<int>(r_it), N * sizeof(int));
  if (out->found) memcpy(out->found, rb.at<uint8_t>(r_found), N);
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
  const size_t N = (size_t)n;
  Blob blob;
  const size_t b_T = blob.add(in->frame_T, (size_t)nf * 7), b_pos = blob.add(in->pos, N * 3), b_fr = blob.add(in->frame, N);
  if (const int rc = upload_blob(c, c->s_d_in, blob)) return rc;
  Carver cv;
  const size_t o_px = cv.take<double>(N * 2), o_cell = cv.take<int>(N);
  HIP_TRY(c, c->s_d_out.ensure(cv.off + 256));
  ReprojBatchDev b{};
  b.fx = in->cam.fx; b.fy = in->cam.fy; b.cx = in->cam.cx; b.cy = in->cam.cy; b.cam_width = in->cam.width; b.cam_height = in->cam.height;
  b.n = n; b.cell_size = in->cell_size; b.grid_n_cols = in->grid_n_cols; b.boundary = in->boundary;
  b.frame_T = Blob::dev<double>(c->s_d_in, b_T); b.pos = Blob::dev<double>(c->s_d_in, b_pos); b.frame = Blob::dev<int>(c->s_d_in, b_fr);
  b.px = Carver::dev<double>(c->s_d_out, o_px); b.cell = Carver::dev<int>(c->s_d_out, o_cell);
  HIP_TRY_TIMED(c, PLSVO_K_MATCH, launch_reproject(b, c->stream));
  Readback rb;
  const int r_px = rb.add(b.px, N * 2 * sizeof(double)), r_cell = rb.add(b.cell, N * sizeof(int));
  if (const int rc = rb.wait(c)) return rc;
  if (out->px) memcpy(out->px, rb.at<double>(r_px), N * 2 * sizeof(double));
  if (out->cell) memcpy(out->cell, rb.at<int>(r_cell), N * sizeof(int));
  return PLSVO_OK;
}

// ---- resident frame step ------------------------------------------------------------------------------

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
  const DevBuf& din = c->s_d_in; const DevBuf& dout = c->s_d_out;
  CloseKfBatchDev b{};
  b.jobs = Blob::dev<CloseKfJobDev>(din, o_jobs); b.n_jobs = n;
  b.kf_T = Blob::dev<double>(din, o_T); b.keypt_pos = Blob::dev<double>(din, o_kp); b.keypt_valid = Blob::dev<uint8_t>(din, o_kv);
  b.tmp_dist = Carver::dev<double>(dout, o_tmp); b.close_idx = Carver::dev<int>(dout, o_idx);
  b.close_dist = Carver::dev<double>(dout, o_dist); b.counts = Carver::dev<int>(dout, o_cnt);
  HIP_TRY_TIMED(c, PLSVO_K_KEYFRAME, launch_close_keyframes(b, c->stream));
  Readback rb;   // (the scratch row tmp_dist stays on the device)
  const int r_idx = rb.add(b.close_idx, total * sizeof(int)), r_dist = rb.add(b.close_dist, total * sizeof(double)), r_cnt = rb.add(b.counts, (size_t)n * 2 * sizeof(int));
  if ((rc = rb.wait(c))) return rc;
  const int* h_idx = rb.at<int>(r_idx); const double* h_dist = rb.at<double>(r_dist); const int* h_cnt = rb.at<int>(r_cnt);
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
  Carver cv;
  const size_t r_out = cv.take<KfDecideOutDev>((size_t)n), r_dt = cv.take<double>(t_ov), r_dr = cv.take<double>(t_ov);
  const size_t r_keys = cv.take<unsigned long long>(o_depth);
  HIP_TRY(c, c->s_d_out.ensure(cv.off + 256));
  const DevBuf& din = c->s_d_in; const DevBuf& dout = c->s_d_out;
  KfDecideBatchDev b{};
  b.jobs = Blob::dev<KfDecideJobDev>(din, b_jobs); b.out = Carver::dev<KfDecideOutDev>(dout, r_out); b.n_jobs = n;
  b.pt_px = Blob::dev<double>(din, b_px); b.pt_pos = Blob::dev<double>(din, b_pos); b.pt_alive = Blob::dev<uint8_t>(din, b_pa);
  b.seg_spos = Blob::dev<double>(din, b_sp); b.seg_epos = Blob::dev<double>(din, b_ep); b.seg_alive = Blob::dev<uint8_t>(din, b_sa);
  b.kf_T = Blob::dev<double>(din, b_kf); b.overlap_idx = Blob::dev<int>(din, b_ov);
  b.depth_keys = Carver::dev<unsigned long long>(dout, r_keys);
  b.delta_t = Carver::dev<double>(dout, r_dt); b.delta_r = Carver::dev<double>(dout, r_dr);
  HIP_TRY_TIMED(c, PLSVO_K_KEYFRAME, launch_keyframe_decide(b, c->stream));
  Readback rb;   // (the depth rows stay on the device)
  const int h_out = rb.add(b.out, (size_t)n * sizeof(KfDecideOutDev)), h_t = rb.add(b.delta_t, t_ov * sizeof(double)), h_r = rb.add(b.delta_r, t_ov * sizeof(double));
  if ((rc = rb.wait(c))) return rc;
  const KfDecideOutDev* ho = rb.at<KfDecideOutDev>(h_out);
  const double* h_dt = rb.at<double>(h_t); const double* h_dr = rb.at<double>(h_r);
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
  if ((rc = c->ch_w.ensure(c, (size_t)n, (size_t)npt_total, (size_t)nseg_total))) return rc;
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
  c->ch_w.bind_resident(c->ch_pose, b, n);
  c->ch_jobs.swap(jobs);
  c->ch_n = n; c->ch_ncand = (int)NC; c->ch_npt_cap = npt_total; c->ch_nseg_cap = nseg_total;
  c->ch_staged = true; c->ch_run_seq = 0; c->ch_stage_seq = ++c->run_seq;
  return PLSVO_OK;
}

extern "C" int plsvo_chain_run(plsvo_ctx* c) {
  CTX_CHECK(c);
  RoctxRange range("frame_step");
  if (!c->ch_staged || !c->a_staged || c->a_n != c->ch_n) return fail(c, PLSVO_E_STATE, "chain_run: no staged frame step (or the alignment batch was re-staged since)");
  int rc = plsvo_align_run(c); if (rc) return rc;
  HIP_TRY(c, launch_chain_pose(c->ch_b, c->stream));
  const auto reproject_match_select = [&]() -> hipError_t {   // four launches timed as one: the first failure ends them
    hipError_t e = launch_reproject(c->ch_reproj, c->stream);
    if (e == hipSuccess) e = launch_chain_active(c->ch_b, c->stream);
    if (e == hipSuccess) e = launch_match_direct(c->ch_match, c->stream);
    return e != hipSuccess ? e : launch_chain_select(c->ch_b, c->stream);
  };
  HIP_TRY_TIMED(c, PLSVO_K_MATCH, reproject_match_select());
  const int threads = pose_opt_threads(c, c->ch_n, (long)c->ch_b.n_cand);   // (selected features <= candidates)
  c->p_refill_frames = 0;   // (the chain's jobs are written on the device: the host cannot see whether one has a refinement loop -- pose_opt_rows_kernel)
  HIP_TRY_TIMED(c, PLSVO_K_POSEOPT, launch_pose_opt(c->ch_pose, c->ch_w.poses.as<double>(), threads, c->opt_poseopt_select ? 1 : 0, c->stream));
  c->ch_run_seq = ++c->run_seq;
  return PLSVO_OK;
}

extern "C" const double* plsvo_chain_poses_dev(plsvo_ctx* c) { return (c && c->ch_staged) ? c->ch_w.poses.as<double>() : nullptr; }

extern "C" int plsvo_chain_fetch(plsvo_ctx* c, int n, plsvo_chain_out* out) {
  CTX_CHECK(c);
  if (!c->ch_staged) return fail(c, PLSVO_E_STATE, "chain_fetch: no staged frame step");
  if (n != c->ch_n || !out) return fail(c, PLSVO_E_INVALID, "chain_fetch: n does not match the staged batch");
  // the alignment results through the ordinary fetch (the caller's seg_alive_out buffers are honoured)
  std::vector<plsvo_align_out> ao((size_t)n);
  for (int j = 0; j < n; ++j) ao[(size_t)j].seg_alive_out = out[j].align.seg_alive_out;
  int rc = plsvo_align_fetch(c, n, ao.data()); if (rc) return rc;
  const size_t NC = (size_t)c->ch_ncand, NP = (size_t)c->ch_npt_cap, NS = (size_t)c->ch_nseg_cap;
  const ChainBatchDev& b = c->ch_b;
  Readback rb;   // (behind the alignment's fetch, whose views have been consumed into ao)
  const int r_st = rb.add(c->ch_w.state.p, (size_t)n * sizeof(PoseStateDev)), r_nsel = rb.add(b.n_sel, (size_t)n * 2 * sizeof(int)), r_found = rb.add(b.found, NC),
            r_mpx = rb.add(b.m_px, NC * 2 * sizeof(double)), r_slev = rb.add(b.search_level, NC * sizeof(int)), r_pk = rb.add(c->ch_w.ptkeep.p, NP),
            r_selp = rb.add(b.sel_pt, NP * sizeof(int)), r_sk = rb.add(c->ch_w.segkeep.p, NS), r_sels = rb.add(b.sel_seg, NS * sizeof(int));
  if ((rc = rb.wait(c))) return rc;
  const PoseStateDev* st = rb.at<PoseStateDev>(r_st); const int* nsel = rb.at<int>(r_nsel);
  for (int j = 0; j < n; ++j) {
    const ChainJobDev& J = c->ch_jobs[(size_t)j];
    plsvo_chain_out& o = out[j];
    o.align = ao[(size_t)j];
    pose_state_to_out(st[j], o.pose);
    o.n_sel_pt = nsel[(size_t)j * 2]; o.n_sel_seg = nsel[(size_t)j * 2 + 1];
    const int nc = J.n_pt + 2 * J.n_seg;
    if (o.pose.pt_keep && o.n_sel_pt > 0) memcpy(o.pose.pt_keep, rb.at<uint8_t>(r_pk) + J.po_pt_off, (size_t)o.n_sel_pt);
    if (o.pose.seg_keep && o.n_sel_seg > 0) memcpy(o.pose.seg_keep, rb.at<uint8_t>(r_sk) + J.po_seg_off, (size_t)o.n_sel_seg);
    if (o.found && nc) memcpy(o.found, rb.at<uint8_t>(r_found) + J.cand_off, (size_t)nc);
    if (o.px && nc) memcpy(o.px, rb.at<double>(r_mpx) + 2 * (size_t)J.cand_off, (size_t)nc * 2 * sizeof(double));
    if (o.search_level && nc) memcpy(o.search_level, rb.at<int>(r_slev) + J.cand_off, (size_t)nc * sizeof(int));
    if (o.sel_pt && o.n_sel_pt > 0) memcpy(o.sel_pt, rb.at<int>(r_selp) + J.po_pt_off, (size_t)o.n_sel_pt * sizeof(int));
    if (o.sel_seg && o.n_sel_seg > 0) memcpy(o.sel_seg, rb.at<int>(r_sels) + J.po_seg_off, (size_t)o.n_sel_seg * sizeof(int));
  }
  return PLSVO_OK;
}

extern "C" int plsvo_frame_step_batch(plsvo_ctx* c, int n, const plsvo_chain_in* in, const plsvo_chain_params* params, plsvo_chain_out* out) {
  int rc = plsvo_chain_stage(c, n, in, params); if (rc) return rc;
  rc = plsvo_chain_run(c); if (rc) return rc;
  return plsvo_chain_fetch(c, n, out);
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
  const size_t NP = (size_t)np, NS = (size_t)ns;
  Blob blob;
  const size_t b_T = blob.add(in->frame_T, (size_t)nf * 7), b_ppx = blob.add(in->pt_px, NP * 2), b_pf = blob.add(in->pt_f, NP * 3), b_pg = blob.add(in->pt_grad, NP * 2),
               b_spx = blob.add(in->seg_px, NS * 2), b_sf0 = blob.add(in->seg_f, NS * 3), b_ssf = blob.add(in->seg_sf, NS * 3), b_sef = blob.add(in->seg_ef, NS * 3),
               b_slot = blob.add(in->frame_slot, (size_t)nf), b_prf = blob.add(in->pt_ref_frame, NP), b_pcf = blob.add(in->pt_cur_frame, NP), b_plv = blob.add(in->pt_level, NP),
               b_srf = blob.add(in->seg_ref_frame, NS), b_scf = blob.add(in->seg_cur_frame, NS), b_slv = blob.add(in->seg_level, NS),
               b_pa = blob.add(in->pt_a, NP), b_pb = blob.add(in->pt_b, NP), b_pmu = blob.add(in->pt_mu, NP), b_pzr = blob.add(in->pt_z_range, NP), b_ps2 = blob.add(in->pt_sigma2, NP),
               b_sa = blob.add(in->seg_a, NS), b_sb = blob.add(in->seg_b, NS), b_smus = blob.add(in->seg_mu_s, NS), b_smue = blob.add(in->seg_mu_e, NS),
               b_szrs = blob.add(in->seg_z_range_s, NS), b_szre = blob.add(in->seg_z_range_e, NS), b_ss2s = blob.add(in->seg_sigma2_s, NS), b_ss2e = blob.add(in->seg_sigma2_e, NS),
               b_pty = blob.add(in->pt_type, NP);
  if (const int rc = upload_blob(c, c->s_d_in, blob)) return rc;
  // outputs: doubles, floats, ints -- one section per element type, the arrays of a type one behind the other
  const size_t od_n = NP * 6 + NS * 8, of_n = NP * 4 + NS * 6, oi_n = NP + NS;
  Carver cv;
  const size_t o_d = cv.take<double>(od_n), o_f = cv.take<float>(of_n), o_i = cv.take<int>(oi_n);
  HIP_TRY(c, c->s_d_out.ensure(cv.off + 256));
  const DevBuf& din = c->s_d_in;
  double* od = Carver::dev<double>(c->s_d_out, o_d);
  float* of = Carver::dev<float>(c->s_d_out, o_f);
  int* oi = Carver::dev<int>(c->s_d_out, o_i);
  SeedsBatchDev b{};
  b.pyr_base = c->pyr.base; b.slot_bytes = c->pyr.slot_bytes; b.width = c->pyr.w[0]; b.height = c->pyr.h[0];
  b.fx = in->cam.fx; b.fy = in->cam.fy; b.cx = in->cam.cx; b.cy = in->cam.cy; b.cam_width = in->cam.width; b.cam_height = in->cam.height;
  b.n_pyr_levels = in->n_pyr_levels; b.align_max_iter = in->align_max_iter; b.max_epi_search_steps = in->max_epi_search_steps;
  b.edgelet_filtering = in->edgelet_filtering; b.edgelet_max_angle = in->edgelet_max_angle;
  b.px_error_angle = std::atan(in->px_noise / (2.0 * std::fabs(in->cam.fx))) * 2.0;   // depth_filter.cpp:279-280 (host libm, like the reference)
  b.convergence_sigma2_thresh = in->convergence_sigma2_thresh;
  b.n_pt = np; b.n_seg = ns;
  const auto D = [&](size_t o) { return Blob::dev<double>(din, o); };
  const auto I = [&](size_t o) { return Blob::dev<int>(din, o); };
  const auto F = [&](size_t o) { return Blob::dev<float>(din, o); };
  b.frame_T = D(b_T); b.frame_slot = I(b_slot);
  b.pt_ref_frame = I(b_prf); b.pt_cur_frame = I(b_pcf); b.pt_level = I(b_plv); b.pt_px = D(b_ppx); b.pt_f = D(b_pf);
  b.pt_grad = in->pt_grad ? D(b_pg) : nullptr; b.pt_type = Blob::dev<uint8_t>(din, b_pty);
  b.pt_a = F(b_pa); b.pt_b = F(b_pb); b.pt_mu = F(b_pmu); b.pt_z_range = F(b_pzr); b.pt_sigma2 = F(b_ps2);
  b.seg_ref_frame = I(b_srf); b.seg_cur_frame = I(b_scf); b.seg_level = I(b_slv);
  b.seg_px = D(b_spx); b.seg_f = D(b_sf0); b.seg_sf = D(b_ssf); b.seg_ef = D(b_sef);
  b.seg_a = F(b_sa); b.seg_b = F(b_sb); b.seg_mu_s = F(b_smus); b.seg_mu_e = F(b_smue); b.seg_z_range_s = F(b_szrs);
  b.seg_z_range_e = F(b_szre); b.seg_sigma2_s = F(b_ss2s); b.seg_sigma2_e = F(b_ss2e);
  b.o_pt_xyz = od; b.o_pt_px = od + NP * 3; b.o_pt_depth = od + NP * 5;
  double* ods = od + NP * 6;
  b.o_seg_xyz_s = ods; b.o_seg_xyz_e = ods + NS * 3; b.o_seg_depth_s = ods + NS * 6; b.o_seg_depth_e = ods + NS * 7;
  b.o_pt_a = of; b.o_pt_b = of + NP; b.o_pt_mu = of + NP * 2; b.o_pt_sigma2 = of + NP * 3;
  float* ofs = of + NP * 4;
  b.o_seg_a = ofs; b.o_seg_b = ofs + NS; b.o_seg_mu_s = ofs + NS * 2; b.o_seg_mu_e = ofs + NS * 3; b.o_seg_sigma2_s = ofs + NS * 4; b.o_seg_sigma2_e = ofs + NS * 5;
  b.o_pt_status = oi; b.o_seg_status = oi + NP;
  HIP_TRY_TIMED(c, PLSVO_K_SEEDS, launch_update_seeds(b, c->stream));
  Readback rb;
  const int r_d = rb.add(od, od_n * sizeof(double)), r_f = rb.add(of, of_n * sizeof(float)), r_i = rb.add(oi, oi_n * sizeof(int));
  if (const int rc = rb.wait(c)) return rc;
  const double* hd = rb.at<double>(r_d);
  const float* hf = rb.at<float>(r_f);
  const int* hi = rb.at<int>(r_i);
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
  // the resident frame step: its own pose-optimisation state -- unless a staged pose-optimisation batch has run since the step was staged
  // and last ran (the records then describe that batch: "the one that ran last", as between the two batches below)
  const bool p_later = c->p_staged && c->p_run_seq > std::max(c->ch_stage_seq, c->ch_run_seq);
  if (c->ch_staged && c->a_staged && c->a_n == c->ch_n && !p_later) {
    if (c->ch_run_seq == 0) { r.why_not = "pack_pose_records: the staged frame step has not run"; return r; }
    r.ast = c->a_d_state.as<AlignStateDev>(); r.pst = c->ch_w.state.as<PoseStateDev>(); r.n = c->ch_n;
    return r;
  }
  // both batches when they describe the same streams (same size); otherwise the one that ran last
  const bool use_a = c->a_staged && c->a_run_seq > 0, use_p = c->p_staged && c->p_run_seq > 0;
  const bool both = use_a && use_p && c->a_n == c->p_n;
  if (use_a && (both || !use_p || c->a_run_seq > c->p_run_seq)) { r.ast = c->a_d_state.as<AlignStateDev>(); r.n = c->a_n; }
  if (use_p && (both || !use_a || c->p_run_seq > c->a_run_seq)) { r.pst = c->p_w.state.as<PoseStateDev>(); r.n = c->p_n; }
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

// ---- bootstrap KLT (plsvo_klt_*) ----
#include "capi_klt.hpp"
