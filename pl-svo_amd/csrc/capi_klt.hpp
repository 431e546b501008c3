// capi_klt.hpp -- the plsvo_klt_* entry points of include/plsvo_hip.h: the bootstrap's KLT track of the first keyframe's corners
// (klt_device.hpp); host side only.  Included once, at the end of plsvo_capi.hip, beside the pyramids and the detector
// whose slots and records it reads: the library's list of translation units, and the host emulation build's, stay as they were.
#pragma once
#include <cmath>

#include "capi_ctx.hpp"

namespace {
// the top level of calcOpticalFlowPyrLK's pyramid and the level sizes (buildOpticalFlowPyramid's loop)
static int klt_fill_levels(int width, int height, int win, int max_level, KltLevelsDev* lv) {
  int w = width, h = height, L = max_level;
  for (int level = 0; level <= max_level; ++level) {
    lv->w[level] = w; lv->h[level] = h;
    const int nw = (w + 1) / 2, nh = (h + 1) / 2;
    if (nw <= win || nh <= win) { L = level; break; }
    w = nw; h = nh;
  }
  lv->n_lv = L + 1;
  unsigned long long off = 0;
  for (int l = 1; l <= L; ++l) { lv->off[l] = (unsigned int)off; off += ((unsigned long long)lv->w[l] * lv->h[l] + 64 + 255) & ~255ull; }
  lv->pyr_bytes = off ? off : 256;
  return L;
}
static bool klt_cfg_ok(const plsvo_klt_cfg* f) {
  return f && f->win == kKltWin && f->max_level >= 0 && f->max_level <= PLSVO_KLT_MAX_LEVEL && f->max_iter >= 1 && f->max_iter <= 255 &&
         std::isfinite(f->eps) && f->eps >= 0.0 && std::isfinite(f->min_eig) && f->min_eig >= 0.0;
}
struct KltSections { size_t px_ref, px_cur, f_ref, f_cur, disparity, next, status, keys, count, st, report, end; };
static KltSections klt_sections(size_t streams, size_t cap) {
  Carver q; KltSections s;
  const size_t t = streams * cap;
  s.px_ref = q.take<float>(2 * t); s.px_cur = q.take<float>(2 * t); s.f_ref = q.take<double>(3 * t); s.f_cur = q.take<double>(3 * t);
  s.disparity = q.take<double>(t); s.next = q.take<float>(2 * t); s.status = q.take<uint8_t>(t); s.keys = q.take<unsigned long long>(t);
  s.count = q.take<int>(streams); s.st = q.take<KltStreamDev>(streams); s.report = q.take<plsvo_klt_report>(streams); s.end = q.off;
  return s;
}
static void klt_bind(KltBatchDev& b, const DevBuf& buf, const KltSections& s) {
  b.px_ref = Carver::dev<float>(buf, s.px_ref); b.px_cur = Carver::dev<float>(buf, s.px_cur); b.f_ref = Carver::dev<double>(buf, s.f_ref);
  b.f_cur = Carver::dev<double>(buf, s.f_cur); b.disparity = Carver::dev<double>(buf, s.disparity); b.next = Carver::dev<float>(buf, s.next);
  b.status = Carver::dev<uint8_t>(buf, s.status); b.keys = Carver::dev<unsigned long long>(buf, s.keys); b.count = Carver::dev<int>(buf, s.count);
  b.st = Carver::dev<KltStreamDev>(buf, s.st); b.report = Carver::dev<plsvo_klt_report>(buf, s.report);
}
static int klt_state(plsvo_ctx* c, const char* who) {
  if (!c->kl_reserved) return fail(c, PLSVO_E_STATE, std::string(who) + ": no plsvo_klt_reserve");
  if (!c->pyr.base || c->pyr.base != c->kl_pyr_base || c->pyr.w[0] != c->kl_b.lv.w[0] || c->pyr.h[0] != c->kl_b.lv.h[0] || c->pyr.slot_bytes != c->kl_b.slot_bytes)
    return fail(c, PLSVO_E_STATE, std::string(who) + ": the pyramids were reconfigured since plsvo_klt_reserve");
  return PLSVO_OK;
}
// levels 1 .. L of the rows' pyramids (which = 0: reference frame, 1: current frame), one launch per level
static int klt_enqueue_pyramids(plsvo_ctx* c, const KltBatchDev& b, int which) {
  for (int l = 1; l < b.lv.n_lv; ++l) HIP_TRY_TIMED(c, PLSVO_K_HALFSAMPLE, launch_klt_pyrdown(b, l, which, c->stream));
  return PLSVO_OK;
}
}  // namespace

extern "C" int plsvo_klt_levels(int width, int height, int win, int max_level, int32_t* w, int32_t* h) {
  if (width < 1 || height < 1 || win < 1 || max_level < 0 || max_level > PLSVO_KLT_MAX_LEVEL) return PLSVO_E_INVALID;
  KltLevelsDev lv{};
  const int L = klt_fill_levels(width, height, win, max_level, &lv);
  for (int l = 0; l <= L; ++l) { if (w) w[l] = lv.w[l]; if (h) h[l] = lv.h[l]; }
  return L;
}

extern "C" int plsvo_klt_reserve(plsvo_ctx* c, const plsvo_klt_cfg* cfg) {
  CTX_CHECK(c);
  if (!c->pyr.base) return fail(c, PLSVO_E_STATE, "klt_reserve: pyramids not configured");
  if (!klt_cfg_ok(cfg) || cfg->streams < 1 || cfg->streams > 65535 || cfg->cap_pts < 1 || cfg->cap_pts > (1 << 20))
    return fail(c, PLSVO_E_INVALID, "klt_reserve: bad configuration (win is 30, max_level 0 .. 4, max_iter 1 .. 255, streams 1 .. 65535, cap_pts 1 .. 2^20)");
  HIP_TRY(c, hipSetDevice(c->device));
  KltBatchDev b{};
  klt_fill_levels(c->pyr.w[0], c->pyr.h[0], cfg->win, cfg->max_level, &b.lv);
  b.lv.off[0] = c->pyr.off[0];
  const KltSections s = klt_sections((size_t)cfg->streams, (size_t)cfg->cap_pts);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, c->kl_d_store.ensure((size_t)2 * cfg->streams * b.lv.pyr_bytes + 256));
  HIP_TRY(c, c->kl_d_lists.ensure(s.end + 256));
  HIP_TRY(c, hipMemsetAsync(c->kl_d_lists.p, 0, s.end, c->stream));
  klt_bind(b, c->kl_d_lists, s);
  std::vector<plsvo_klt_report> rep((size_t)cfg->streams);
  for (auto& r : rep) { memset(&r, 0, sizeof(r)); r.result = PLSVO_KLT_INACTIVE; r.levels = b.lv.n_lv; }
  HIP_TRY(c, hipMemcpyAsync(b.report, rep.data(), rep.size() * sizeof(plsvo_klt_report), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  b.pyr = c->pyr_slab.as<uint8_t>(); b.slot_bytes = c->pyr.slot_bytes; b.store = c->kl_d_store.as<uint8_t>();
  b.cap_pts = cfg->cap_pts; b.max_iter = cfg->max_iter; b.eps2 = cfg->eps * cfg->eps; b.min_eig = cfg->min_eig;
  c->kl_b = b; c->kl_cfg = *cfg; c->kl_pyr_base = c->pyr.base; c->kl_ref_slot.assign((size_t)cfg->streams, -1);
  c->kl_reserved = true;
  return PLSVO_OK;
}

extern "C" int plsvo_klt_first_frame(plsvo_ctx* c, int n, const plsvo_klt_first* in) {
  CTX_CHECK(c);
  if (const int rc = klt_state(c, "klt_first_frame")) return rc;
  if (n != c->kl_cfg.streams || !in) return fail(c, PLSVO_E_INVALID, "klt_first_frame: another n than reserved, or NULL in");
  std::vector<KltFirstDev> jobs;
  std::vector<KltRowDev> rows;
  long long n_host = 0, n_extra = 0;
  for (int i = 0; i < n; ++i) {
    const plsvo_klt_first& f = in[i];
    if (!f.active) continue;
    const bool cam_ok = f.cam.width == c->pyr.w[0] && f.cam.height == c->pyr.h[0] && std::isfinite(f.cam.fx) && std::isfinite(f.cam.fy) &&
                        std::isfinite(f.cam.cx) && std::isfinite(f.cam.cy) && f.cam.fx != 0.0 && f.cam.fy != 0.0;
    if (f.slot < 0 || f.slot >= c->pyr.n_slots || !cam_ok || (f.d_corners && !f.d_count) || f.n_host < 0 || f.n_extra < 0 ||
        (!f.d_corners && f.n_host > 0 && !f.host_px) || (f.n_extra > 0 && (!f.extra_px || !f.extra_f)))
      return fail(c, PLSVO_E_INVALID, "klt_first_frame: stream " + std::to_string(i) + ": bad slot, camera, count or NULL array");
    KltFirstDev j{};
    j.stream = i; j.n_host = f.d_corners ? 0 : f.n_host; j.n_extra = f.n_extra;
    j.fx = f.cam.fx; j.fy = f.cam.fy; j.cx = f.cam.cx; j.cy = f.cam.cy;
    j.d_corners = f.d_corners; j.d_count = f.d_count; j.host_at = n_host; j.extra_at = n_extra;
    n_host += j.n_host; n_extra += j.n_extra;
    jobs.push_back(j);
    rows.push_back(KltRowDev{ i, f.slot, f.slot, 0 });
  }
  if (jobs.empty()) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  Blob blob;
  const size_t o_jobs = blob.add(jobs), o_rows = blob.add(rows);
  const size_t o_host = blob.reserve<float>(2 * (size_t)n_host), o_epx = blob.reserve<float>(2 * (size_t)n_extra), o_ef = blob.reserve<double>(3 * (size_t)n_extra);
  for (const KltFirstDev& j : jobs) {
    const plsvo_klt_first& f = in[j.stream];
    if (j.n_host) memcpy(blob.at<float>(o_host) + 2 * j.host_at, f.host_px, 2 * (size_t)j.n_host * sizeof(float));
    if (j.n_extra) {
      memcpy(blob.at<float>(o_epx) + 2 * j.extra_at, f.extra_px, 2 * (size_t)j.n_extra * sizeof(float));
      memcpy(blob.at<double>(o_ef) + 3 * j.extra_at, f.extra_f, 3 * (size_t)j.n_extra * sizeof(double));
    }
  }
  if (const int rc = upload_blob(c, c->kl_d_in, blob)) return rc;
  KltBatchDev b = c->kl_b;
  b.first = Blob::dev<KltFirstDev>(c->kl_d_in, o_jobs); b.rows = Blob::dev<KltRowDev>(c->kl_d_in, o_rows); b.n_rows = (int)rows.size();
  b.host_px = Blob::dev<float>(c->kl_d_in, o_host); b.extra_px = Blob::dev<float>(c->kl_d_in, o_epx); b.extra_f = Blob::dev<double>(c->kl_d_in, o_ef);
  HIP_TRY_TIMED(c, PLSVO_K_NEWCAND, launch_klt_first(b, (int)jobs.size(), c->stream));
  if (const int rc = klt_enqueue_pyramids(c, b, 0)) return rc;
  for (const KltRowDev& r : rows) c->kl_ref_slot[(size_t)r.stream] = r.ref_slot;
  return PLSVO_OK;
}

extern "C" int plsvo_klt_second_frame(plsvo_ctx* c, int n, const plsvo_klt_second* in, const plsvo_klt_params* params) {
  CTX_CHECK(c);
  if (const int rc = klt_state(c, "klt_second_frame")) return rc;
  if (n != c->kl_cfg.streams || !in || !params || params->init_min_tracked < 0 || !std::isfinite(params->init_min_disparity))
    return fail(c, PLSVO_E_INVALID, "klt_second_frame: another n than reserved, NULL in or params, a negative init_min_tracked or a non-finite init_min_disparity");
  std::vector<KltRowDev> rows;
  for (int i = 0; i < n; ++i) {
    if (!in[i].active) continue;
    if (in[i].cur_slot < 0 || in[i].cur_slot >= c->pyr.n_slots) return fail(c, PLSVO_E_INVALID, "klt_second_frame: stream " + std::to_string(i) + ": slot outside the pyramids");
    const int ref = c->kl_ref_slot[(size_t)i];
    rows.push_back(KltRowDev{ i, ref < 0 ? in[i].cur_slot : ref, in[i].cur_slot, 0 });   // (a stream without a first frame holds no entries: nothing reads its reference)
  }
  if (rows.empty()) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  Blob blob;
  const size_t o_rows = blob.add(rows);
  if (const int rc = upload_blob(c, c->kl_d_in, blob)) return rc;
  KltBatchDev b = c->kl_b;
  b.rows = Blob::dev<KltRowDev>(c->kl_d_in, o_rows); b.n_rows = (int)rows.size();
  b.min_tracked = params->init_min_tracked; b.min_disparity = params->init_min_disparity;
  if (const int rc = klt_enqueue_pyramids(c, b, 1)) return rc;
  HIP_TRY_TIMED(c, PLSVO_K_MATCH, launch_klt_track(b, b.cap_pts, c->stream));
  HIP_TRY_TIMED(c, PLSVO_K_NEWCAND, launch_klt_commit(b, c->stream));
  return PLSVO_OK;
}

extern "C" int plsvo_klt_fetch(plsvo_ctx* c, int n, plsvo_klt_report* report) {
  CTX_CHECK(c);
  if (!c->kl_reserved) return fail(c, PLSVO_E_STATE, "klt_fetch: no plsvo_klt_reserve");
  if (n != c->kl_cfg.streams || !report) return fail(c, PLSVO_E_INVALID, "klt_fetch: another n than reserved, or NULL report");
  HIP_TRY(c, hipSetDevice(c->device));
  Readback rb;
  rb.add(c->kl_b.report, (size_t)n * sizeof(plsvo_klt_report));
  if (const int rc = rb.wait(c)) return rc;
  memcpy(report, rb.at<plsvo_klt_report>(0), (size_t)n * sizeof(plsvo_klt_report));
  return PLSVO_OK;
}

extern "C" int plsvo_klt_fetch_tracks(plsvo_ctx* c, int stream, plsvo_klt_tracks* out) {
  CTX_CHECK(c);
  if (!c->kl_reserved) return fail(c, PLSVO_E_STATE, "klt_fetch_tracks: no plsvo_klt_reserve");
  if (stream < 0 || stream >= c->kl_cfg.streams || !out) return fail(c, PLSVO_E_INVALID, "klt_fetch_tracks: stream outside the batch, or NULL out");
  HIP_TRY(c, hipSetDevice(c->device));
  const KltBatchDev& b = c->kl_b;
  const size_t cap = (size_t)b.cap_pts, at = (size_t)stream * cap;
  Readback rb;
  rb.add(b.count + stream, sizeof(int));
  rb.add(b.px_ref + 2 * at, 2 * cap * sizeof(float)); rb.add(b.px_cur + 2 * at, 2 * cap * sizeof(float));
  rb.add(b.f_ref + 3 * at, 3 * cap * sizeof(double)); rb.add(b.f_cur + 3 * at, 3 * cap * sizeof(double)); rb.add(b.disparity + at, cap * sizeof(double));
  if (const int rc = rb.wait(c)) return rc;
  const int cnt = *rb.at<int>(0);
  if (cnt < 0 || (size_t)cnt > cap) return fail(c, PLSVO_E_HIP, "klt_fetch_tracks: corrupt count");
  out->n = cnt; out->cap_pts = b.cap_pts;
  if (out->px_ref) memcpy(out->px_ref, rb.at<float>(1), 2 * (size_t)cnt * sizeof(float));
  if (out->px_cur) memcpy(out->px_cur, rb.at<float>(2), 2 * (size_t)cnt * sizeof(float));
  if (out->f_ref) memcpy(out->f_ref, rb.at<double>(3), 3 * (size_t)cnt * sizeof(double));
  if (out->f_cur) memcpy(out->f_cur, rb.at<double>(4), 3 * (size_t)cnt * sizeof(double));
  if (out->disparity) memcpy(out->disparity, rb.at<double>(5), (size_t)cnt * sizeof(double));
  return PLSVO_OK;
}

extern "C" int plsvo_klt_tracks_dev(plsvo_ctx* c, plsvo_klt_tracks* out) {
  CTX_CHECK(c);
  if (!c->kl_reserved) return fail(c, PLSVO_E_STATE, "klt_tracks_dev: no plsvo_klt_reserve");
  if (!out) return fail(c, PLSVO_E_INVALID, "klt_tracks_dev: NULL out");
  const KltBatchDev& b = c->kl_b;
  out->n = c->kl_cfg.streams; out->cap_pts = b.cap_pts;
  out->px_ref = b.px_ref; out->px_cur = b.px_cur; out->f_ref = b.f_ref; out->f_cur = b.f_cur; out->disparity = b.disparity; out->count = b.count;
  return PLSVO_OK;
}

extern "C" int plsvo_klt_download_level(plsvo_ctx* c, int stream, int which, int level, uint8_t* out) {
  CTX_CHECK(c);
  if (!c->kl_reserved) return fail(c, PLSVO_E_STATE, "klt_download_level: no plsvo_klt_reserve");
  const KltBatchDev& b = c->kl_b;
  if (stream < 0 || stream >= c->kl_cfg.streams || (which != 0 && which != 1) || level < 1 || level >= b.lv.n_lv || !out)
    return fail(c, PLSVO_E_INVALID, "klt_download_level: stream, pyramid or level outside the store (it holds levels 1 .. top), or NULL out");
  HIP_TRY(c, hipSetDevice(c->device));
  const uint8_t* src = b.store + (size_t)(2 * stream + which) * b.lv.pyr_bytes + b.lv.off[level];
  HIP_TRY(c, hipMemcpyAsync(out, src, (size_t)b.lv.w[level] * b.lv.h[level], hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return PLSVO_OK;
}

extern "C" int plsvo_klt_track_points(plsvo_ctx* c, const plsvo_klt_cfg* cfg, int ref_slot, int cur_slot, int n, const float* prev, const float* next_in,
                                      float* next_out, uint8_t* status, uint8_t* exit_code, uint8_t* iters) {
  CTX_CHECK(c);
  if (!c->pyr.base) return fail(c, PLSVO_E_STATE, "klt_track_points: pyramids not configured");
  if (!klt_cfg_ok(cfg) || n < 0 || n > (1 << 20) || ref_slot < 0 || ref_slot >= c->pyr.n_slots || cur_slot < 0 || cur_slot >= c->pyr.n_slots ||
      (n > 0 && (!prev || !next_in || !next_out || !status || !exit_code || !iters)))
    return fail(c, PLSVO_E_INVALID, "klt_track_points: bad configuration, slot, count or NULL array");
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  KltBatchDev b{};
  klt_fill_levels(c->pyr.w[0], c->pyr.h[0], cfg->win, cfg->max_level, &b.lv);
  b.lv.off[0] = c->pyr.off[0];
  b.pyr = c->pyr_slab.as<uint8_t>(); b.slot_bytes = c->pyr.slot_bytes;
  b.cap_pts = n; b.max_iter = cfg->max_iter; b.eps2 = cfg->eps * cfg->eps; b.min_eig = cfg->min_eig;
  Carver q;
  const size_t o_store = q.take<uint8_t>(2 * (size_t)b.lv.pyr_bytes), o_next = q.take<float>(2 * (size_t)n), o_status = q.take<uint8_t>((size_t)n);
  const size_t o_exit = q.take<uint8_t>((size_t)n * kKltLevels), o_iters = q.take<uint8_t>((size_t)n * kKltLevels);
  HIP_TRY(c, c->kl_d_diag.ensure(q.off + 256));
  HIP_TRY(c, hipMemsetAsync(Carver::dev<uint8_t>(c->kl_d_diag, o_exit), 0, (o_iters - o_exit) + (size_t)n * kKltLevels, c->stream));
  Blob blob;
  const KltRowDev row{ 0, ref_slot, cur_slot, 0 };
  const int32_t count = n;
  const size_t o_row = blob.add(&row, 1), o_count = blob.add(&count, 1), o_prev = blob.add(prev, 2 * (size_t)n), o_nin = blob.add(next_in, 2 * (size_t)n);
  if (const int rc = upload_blob(c, c->kl_d_in, blob)) return rc;
  b.store = Carver::dev<uint8_t>(c->kl_d_diag, o_store);
  b.rows = Blob::dev<KltRowDev>(c->kl_d_in, o_row); b.n_rows = 1;
  b.count = const_cast<int*>(Blob::dev<int>(c->kl_d_in, o_count));
  b.px_ref = const_cast<float*>(Blob::dev<float>(c->kl_d_in, o_prev)); b.px_cur = const_cast<float*>(Blob::dev<float>(c->kl_d_in, o_nin));
  b.next = Carver::dev<float>(c->kl_d_diag, o_next); b.status = Carver::dev<uint8_t>(c->kl_d_diag, o_status);
  b.diag_exit = Carver::dev<uint8_t>(c->kl_d_diag, o_exit); b.diag_iters = Carver::dev<uint8_t>(c->kl_d_diag, o_iters);
  if (const int rc = klt_enqueue_pyramids(c, b, 0)) return rc;
  if (const int rc = klt_enqueue_pyramids(c, b, 1)) return rc;
  HIP_TRY_TIMED(c, PLSVO_K_MATCH, launch_klt_track(b, n, c->stream));
  Readback rb;
  rb.add(b.next, 2 * (size_t)n * sizeof(float)); rb.add(b.status, (size_t)n); rb.add(b.diag_exit, (size_t)n * kKltLevels); rb.add(b.diag_iters, (size_t)n * kKltLevels);
  if (const int rc = rb.wait(c)) return rc;
  memcpy(next_out, rb.at<float>(0), 2 * (size_t)n * sizeof(float)); memcpy(status, rb.at<uint8_t>(1), (size_t)n);
  memcpy(exit_code, rb.at<uint8_t>(2), (size_t)n * kKltLevels); memcpy(iters, rb.at<uint8_t>(3), (size_t)n * kKltLevels);
  return PLSVO_OK;
}
