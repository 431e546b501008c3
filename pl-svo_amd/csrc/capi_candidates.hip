// capi_candidates.hip -- every plsvo_candidates_* entry point of include/plsvo_hip.h (candidates, cell selection, keyframe insertion, new candidates)
// and the plsvo_seeds_* ones, whose seed lists hand their converged seeds to the same tables; host side only
#include "capi_ctx.hpp"

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
// the sections of cs_d_q (the landmark quality the selection maintains: n_failed_reproj_, n_succeeded_reproj_ of points and segments, then their event bytes)
struct QualitySections { size_t pt_nf, pt_ns, seg_nf, seg_ns, pt_ev, seg_ev, end; };
static QualitySections quality_sections(const plsvo_ctx* c) {
  Carver q; QualitySections s;
  s.pt_nf = q.take<int>(c->cd_t_pt); s.pt_ns = q.take<int>(c->cd_t_pt); s.seg_nf = q.take<int>(c->cd_t_seg); s.seg_ns = q.take<int>(c->cd_t_seg);
  s.pt_ev = q.take<uint8_t>(c->cd_t_pt); s.seg_ev = q.take<uint8_t>(c->cd_t_seg); s.end = q.off;
  return s;
}
static void cand_reset_run(plsvo_ctx* c) { c->cd_ran = c->cd_matched = c->cs_selected = c->cs_posed = c->ci_inserted = c->cn_closed = c->cc_closed = c->co_done = c->ck_have_close = c->ck_decided = false; }   // the steps taken on the last run's results
static void cand_reset_stage(plsvo_ctx* c) { cand_reset_run(c); c->cd_staged = c->ci_have_out = c->cn_have_out = c->cc_have_out = c->co_have_out = c->sd_staged = c->sd_pending = c->sd_have_report = c->sk_have_report = c->ck_live = c->tg_have = false; }   // those, the tables, the key-point table, the last insertion's and add's reports
// PLSVO_OK while the last run's candidates still describe the tables; once an insertion or an add came behind it, the refusal of entry point `who`
static int cand_run_open(plsvo_ctx* c, const char* who) {
  const char* why = c->ci_inserted ? "this run's frame was inserted" : c->cn_closed ? "landmarks were added behind this run" : c->cc_closed ? "the tables were compacted behind this run" : nullptr;
  return why ? fail(c, PLSVO_E_STATE, std::string(who) + ": " + why + " (the tables have moved on); run again") : PLSVO_OK;
}
// between plsvo_seeds_update and plsvo_seeds_update_fetch the tables' sizes are known to the device alone: the refusal of entry point `who`
static int cand_seeds_pending(plsvo_ctx* c, const char* who) {
  return c->sd_pending ? fail(c, PLSVO_E_STATE, std::string(who) + ": a seed update is not fetched yet (plsvo_seeds_update_fetch refreshes the tables' sizes)") : PLSVO_OK;
}
// the key-point table's upkeep behind a launch that changed the keyframes' feature lists (keystage_device.hpp); d_jobs: one record per stream, on the device
static int keypts_enqueue(plsvo_ctx* c, const KeyPtsJobDev* d_jobs) {
  KeyStageBatchDev b = c->ck_b;
  b.c = c->cd_b; b.keypts = c->ck_d_keypts.as<int>(); b.kp_jobs = d_jobs; b.decided = c->ck_decided ? c->ck_dec_b.out : nullptr;
  HIP_TRY_TIMED(c, PLSVO_K_KEYFRAME, launch_map_keypts(b, c->stream));
  return PLSVO_OK;
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
  std::vector<CandStreamHost> host((size_t)n);
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
    CandStreamHost& H = host[(size_t)s];
    H.rows_pt = I.n_pt + L.extra_pt; H.rows_seg = I.n_seg + L.extra_seg; H.rows_pt_cand = I.n_pt_cand + L.extra_pt; H.rows_seg_cand = I.n_seg_cand + L.extra_seg;
    H.fetch_pt_cand = I.n_pt_cand; H.fetch_seg_cand = I.n_seg_cand;
    M.cap_pt = H.rows_pt + H.rows_pt_cand; M.cap_seg = H.rows_seg + H.rows_seg_cand; M.stream = s;   // (what the candidate kernel switches off behind the filed entries: the rows as laid out)
    M.kf_off = (long long)t.kf; M.kfpt_off = (long long)t.kfpt; M.kfseg_off = (long long)t.kfseg; M.pt_off = (long long)t.pt; M.seg_off = (long long)t.seg;
    M.ptobs_off = (long long)t.ptobs; M.segobs_off = (long long)t.segobs; M.ptc_off = (long long)t.ptc; M.segc_off = (long long)t.segc;
    M.opt_off = (long long)t.opt; M.oseg_off = (long long)t.oseg; M.m_off = (long long)t.m; M.f_off = (long long)t.f;
    M.vis_pt_off = (long long)t.vis; t.vis += ((size_t)H.rows_pt + 63) & ~(size_t)63;
    M.vis_seg_off = (long long)t.vis; t.vis += ((size_t)H.rows_seg + 63) & ~(size_t)63;
    if (kfpt + (size_t)R.extra_kf_pt > (size_t)INT32_MAX || kfseg + (size_t)R.extra_kf_seg > (size_t)INT32_MAX || ptobs + (size_t)R.extra_pt_obs > (size_t)INT32_MAX ||
        segobs + (size_t)R.extra_seg_obs > (size_t)INT32_MAX || (size_t)I.n_kf + (size_t)R.extra_kf > (size_t)INT32_MAX) return fail(c, PLSVO_E_CAPACITY, "candidates_stage: stream too large");
    H.cap_kf = I.n_kf + R.extra_kf; H.cap_kf_pt = (int)kfpt + R.extra_kf_pt; H.cap_kf_seg = (int)kfseg + R.extra_kf_seg; H.cap_pt_obs = (int)ptobs + R.extra_pt_obs; H.cap_seg_obs = (int)segobs + R.extra_seg_obs;
    H.n_kf_pt = (int)kfpt; H.n_kf_seg = (int)kfseg; H.n_pt_obs = (int)ptobs; H.n_seg_obs = (int)segobs;
    t.kf += (size_t)H.cap_kf; t.kfpt += (size_t)H.cap_kf_pt; t.kfseg += (size_t)H.cap_kf_seg; t.pt += (size_t)H.rows_pt; t.seg += (size_t)H.rows_seg; t.ptobs += (size_t)H.cap_pt_obs; t.segobs += (size_t)H.cap_seg_obs;
    t.ptc += (size_t)H.rows_pt_cand; t.segc += (size_t)H.rows_seg_cand; t.opt += (size_t)M.cap_pt; t.oseg += (size_t)M.cap_seg;
    t.m += (size_t)M.cap_pt + 2 * (size_t)M.cap_seg; t.f += (size_t)H.cap_kf + 1;
  }
  if (t.m > (size_t)INT32_MAX || t.f > (size_t)INT32_MAX || t.vis > (size_t)INT32_MAX) return fail(c, PLSVO_E_CAPACITY, "candidates_stage: batch too large");
  cand_reset_stage(c);
  c->cd_host = std::move(host);
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
  CandFetchSections& F = c->cd_off;
  F.counts = cv.take<int>(N * 2); F.pt_lm = cv.take<int>(t.opt); F.pt_px = cv.take<double>(t.opt * 2); F.pt_cell = cv.take<int>(t.opt); F.pt_obs = cv.take<int>(t.opt);
  F.pt_view = cv.take<uint8_t>(t.opt); F.pt_active = cv.take<uint8_t>(t.opt); F.seg_lm = cv.take<int>(t.oseg); F.seg_px = cv.take<double>(t.oseg * 4);
  F.seg_cell = cv.take<int>(t.oseg * 2); F.seg_obs = cv.take<int>(t.oseg); F.seg_view = cv.take<uint8_t>(t.oseg); F.seg_active = cv.take<uint8_t>(t.oseg);
  F.pt_cand_failed = cv.take<uint8_t>(t.ptc); F.seg_cand_failed = cv.take<uint8_t>(t.segc);
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
  b.counts = WI(F.counts);
  b.o_pt_lm = WI(F.pt_lm); b.o_pt_px = WD(F.pt_px); b.o_pt_cell = WI(F.pt_cell); b.o_pt_obs = WI(F.pt_obs); b.o_pt_view = WB(F.pt_view); b.o_pt_active = WB(F.pt_active);
  b.o_seg_lm = WI(F.seg_lm); b.o_seg_px = WD(F.seg_px); b.o_seg_cell = WI(F.seg_cell); b.o_seg_obs = WI(F.seg_obs); b.o_seg_view = WB(F.seg_view); b.o_seg_active = WB(F.seg_active);
  b.pt_cand_failed = WB(F.pt_cand_failed); b.seg_cand_failed = WB(F.seg_cand_failed);
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
  c->cd_vis_off = w_vis; c->cd_vis_bytes = t.vis * sizeof(unsigned int);
  c->cd_maps = std::move(md); c->cd_params = *pr; c->cd_n = n; c->cd_total_m = t.m; c->cd_total_f = t.f; c->cd_max_level = max_level;
  c->cd_t_pt = t.pt; c->cd_t_seg = t.seg; c->cd_t_ptc = t.ptc; c->cd_t_segc = t.segc; c->cd_t_opt = t.opt; c->cd_t_oseg = t.oseg;
  const size_t q_bytes = quality_sections(c).end;   // the landmark quality starts at zero
  HIP_TRY(c, c->cs_d_q.ensure(q_bytes + 256));
  HIP_TRY(c, hipMemsetAsync(c->cs_d_q.p, 0, q_bytes, c->stream));
  const size_t key_bytes = (t.pt + t.seg) * sizeof(int);   // last_structure_optim_ of every landmark row of capacity starts at zero, as the reference's constructors set it
  HIP_TRY(c, c->co_d_key.ensure(key_bytes + 256));
  HIP_TRY(c, hipMemsetAsync(c->co_d_key.p, 0, key_bytes, c->stream));
  c->cd_staged = true;
  return PLSVO_OK;
}

// plsvo_candidates_run (max_n_kfs < 0: the caller's overlap lists) and plsvo_candidates_run_close (the lists decided on the device by one
// launch ahead of the candidate launch; a stream's overlap row then has room for every keyframe of its table)
static int cand_run(plsvo_ctx* c, int n, const plsvo_cand_frame* fr, int max_n_kfs) {
  const bool close = max_n_kfs >= 0;
  size_t t_ov = 0;
  for (int s = 0; s < n; ++s) t_ov += close ? (size_t)c->cd_maps[(size_t)s].n_kf : (size_t)fr[s].n_overlap;
  cand_reset_run(c);
  for (int s = 0; s < n; ++s) { c->cd_host[(size_t)s].fetch_pt_cand = c->cd_maps[(size_t)s].n_pt_cand; c->cd_host[(size_t)s].fetch_seg_cand = c->cd_maps[(size_t)s].n_seg_cand; }
  c->cd_ov_off.assign((size_t)n + 1, 0);
  if (n == 0) { c->cd_ran = true; return PLSVO_OK; }
  HIP_TRY(c, hipSetDevice(c->device));
  Blob blob;
  const size_t b_jobs = blob.reserve<CandJobDev>((size_t)n), b_ov = blob.reserve<int>(t_ov), b_room = close ? blob.reserve<int>((size_t)n) : 0;
  CandJobDev* jobs = blob.at<CandJobDev>(b_jobs); int* ov = blob.at<int>(b_ov);
  c->cd_cur_slot.resize((size_t)n);
  size_t o = 0;
  for (int s = 0; s < n; ++s) {
    CandJobDev& J = jobs[s];
    memcpy(J.T, fr[s].T_f_w, sizeof(J.T)); J.d_T = fr[s].d_T_f_w; J.cur_slot = fr[s].cur_slot; J.n_ov = fr[s].n_overlap; J.ov_off = (long long)o;
    if (J.n_ov) memcpy(ov + o, fr[s].overlap_idx, (size_t)J.n_ov * sizeof(int));
    c->cd_cur_slot[(size_t)s] = fr[s].cur_slot; c->cd_ov_off[(size_t)s] = (long long)o;
    if (close) blob.at<int>(b_room)[s] = c->cd_maps[(size_t)s].n_kf;
    o += close ? (size_t)c->cd_maps[(size_t)s].n_kf : (size_t)J.n_ov;
  }
  c->cd_ov_off[(size_t)n] = (long long)o;
  int rc;
  if ((rc = upload_blob(c, c->cd_d_run, blob))) return rc;
  HIP_TRY(c, c->cd_d_kfcount.ensure(std::max(t_ov, (size_t)1) * sizeof(int)));
  CandBatchDev b = c->cd_b;
  const char* dr = reinterpret_cast<const char*>(c->cd_d_run.p);
  b.jobs = reinterpret_cast<const CandJobDev*>(dr + b_jobs); b.overlap_idx = reinterpret_cast<const int*>(dr + b_ov); b.kf_count = c->cd_d_kfcount.as<int>();
  c->cd_run_jobs = b.jobs; c->cd_run_ov = b.overlap_idx;
  const auto rearm_then_launch = [&]() -> hipError_t {   // the first-visit words are all ones ahead of EVERY launch: a run must not see the visits of the one before
    const hipError_t e = c->cd_vis_bytes ? hipMemsetAsync(c->cd_d_work.as<char>() + c->cd_vis_off, 0xff, c->cd_vis_bytes, c->stream) : hipSuccess;
    return e != hipSuccess ? e : launch_map_candidates(b, c->stream);
  };
  if (close) {                                      // results first (what plsvo_candidates_close_fetch brings back), then scratch
    Carver w;
    const size_t w_cnt = w.take<int>((size_t)n * 2), w_idx = w.take<int>(c->ci_t_kf), w_dist = w.take<double>(c->ci_t_kf);
    c->ck_fetch_bytes = w.off;
    const size_t w_tmp = w.take<double>(c->ci_t_kf);
    HIP_TRY(c, c->ck_d_work.ensure(w.off + 256));
    KeyStageBatchDev kb{};
    kb.c = b; kb.keypts = c->ck_d_keypts.as<int>(); kb.ov_room = reinterpret_cast<const int*>(dr + b_room); kb.max_n_kfs = max_n_kfs;
    kb.close_counts = Carver::dev<int>(c->ck_d_work, w_cnt); kb.close_idx = Carver::dev<int>(c->ck_d_work, w_idx); kb.close_dist = Carver::dev<double>(c->ck_d_work, w_dist);
    kb.tmp_dist = Carver::dev<double>(c->ck_d_work, w_tmp);
    HIP_TRY_TIMED(c, PLSVO_K_KEYFRAME, launch_map_close(kb, c->stream));
    c->ck_b = kb;
  }
  HIP_TRY_TIMED(c, PLSVO_K_CANDIDATES, rearm_then_launch());
  c->cd_ran = true; c->ck_have_close = close;
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_run(plsvo_ctx* c, int n, const plsvo_cand_frame* fr) {
  CTX_CHECK(c);
  if (!c->cd_staged) return fail(c, PLSVO_E_STATE, "candidates_run: no staged map tables");
  if (const int rc = cand_seeds_pending(c, "candidates_run")) return rc;
  if (n != c->cd_n || (n > 0 && !fr)) return fail(c, PLSVO_E_INVALID, "candidates_run: n does not match the staged batch");
  for (int s = 0; s < n; ++s) {
    if (fr[s].n_overlap < 0 || fr[s].cur_slot < 0) return fail(c, PLSVO_E_INVALID, "candidates_run: negative count or slot");
    if (fr[s].n_overlap > 0 && !fr[s].overlap_idx) return fail(c, PLSVO_E_INVALID, "candidates_run: null overlap list");
    if (!cand_idx_ok(fr[s].overlap_idx, (size_t)fr[s].n_overlap, 0, c->cd_maps[(size_t)s].n_kf)) return fail(c, PLSVO_E_INVALID, "candidates_run: overlap index outside the keyframe table");
  }
  return cand_run(c, n, fr, -1);
}

// ---- keyframe stage on the resident tables: the key-point table, close keyframes ahead of the candidate launch (keystage_device.hpp) ---------
extern "C" int plsvo_candidates_set_keypts(plsvo_ctx* c, int n, const plsvo_cand_keypts* in) {
  CTX_CHECK(c);
  if (!c->cd_staged) return fail(c, PLSVO_E_STATE, "candidates_set_keypts: no staged map tables");
  if (const int rc = cand_seeds_pending(c, "candidates_set_keypts")) return rc;
  if (n != c->cd_n) return fail(c, PLSVO_E_INVALID, "candidates_set_keypts: n does not match the staged batch");
  for (int s = 0; in && s < n; ++s)
    if (in[s].key_pts && !cand_idx_ok(in[s].key_pts, 5 * (size_t)c->cd_maps[(size_t)s].n_kf, -1, INT32_MAX)) return fail(c, PLSVO_E_INVALID, "candidates_set_keypts: a key point below -1");
  if (n == 0) { c->ck_live = true; return PLSVO_OK; }
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t N = (size_t)n, rows = 5 * c->ci_t_kf;
  Blob blob;
  const size_t b_up = blob.reserve<KeyPtsJobDev>(N), b_jobs = blob.reserve<KeyPtsJobDev>(N), b_tab = blob.reserve<int>(rows);
  bool any_fresh = false;
  for (size_t k = 0; k < rows; ++k) blob.at<int>(b_tab)[k] = -1;
  for (int s = 0; s < n; ++s) {
    const int32_t* kp = in ? in[s].key_pts : nullptr; const CandMapDev& M = c->cd_maps[(size_t)s];
    blob.at<KeyPtsJobDev>(b_up)[s] = KeyPtsJobDev{ kKeyPtsUpkeep, -1, 0, 0 };
    blob.at<KeyPtsJobDev>(b_jobs)[s] = KeyPtsJobDev{ kp ? kKeyPtsStandBy : kKeyPtsFresh, -1, 0, 0 };
    if (kp) { if (M.n_kf) memcpy(blob.at<int>(b_tab) + 5 * M.kf_off, kp, 5 * (size_t)M.n_kf * sizeof(int)); } else any_fresh = true;
  }
  int rc;
  if ((rc = upload_blob(c, c->ck_d_in, blob))) return rc;
  HIP_TRY(c, c->ck_d_upkeep.ensure(N * sizeof(KeyPtsJobDev)));
  HIP_TRY(c, c->ck_d_keypts.ensure(std::max(rows, (size_t)1) * sizeof(int)));
  const char* din = reinterpret_cast<const char*>(c->ck_d_in.p);
  HIP_TRY(c, hipMemcpyAsync(c->ck_d_upkeep.p, din + b_up, N * sizeof(KeyPtsJobDev), hipMemcpyDeviceToDevice, c->stream));
  if (rows) HIP_TRY(c, hipMemcpyAsync(c->ck_d_keypts.p, din + b_tab, rows * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
  if (any_fresh && (rc = keypts_enqueue(c, reinterpret_cast<const KeyPtsJobDev*>(din + b_jobs)))) return rc;
  c->ck_live = true;
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_fetch_keypts(plsvo_ctx* c, int n, plsvo_cand_keypts_out* out) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->ck_live) return fail(c, PLSVO_E_STATE, "candidates_fetch_keypts: no live key-point table (plsvo_candidates_set_keypts)");
  if (const int rc = cand_seeds_pending(c, "candidates_fetch_keypts")) return rc;
  if (n != c->cd_n || (n > 0 && !out)) return fail(c, PLSVO_E_INVALID, "candidates_fetch_keypts: n does not match the staged batch");
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  Readback rb;
  rb.add(c->ck_d_keypts.p, 5 * c->ci_t_kf * sizeof(int));
  if (const int rc = rb.wait(c)) return rc;
  for (int s = 0; s < n; ++s) {
    if (!out[s].key_pts) continue;
    const CandMapDev& M = c->cd_maps[(size_t)s]; const size_t used = 5 * (size_t)M.n_kf, cap = 5 * (size_t)c->cd_host[(size_t)s].cap_kf;
    if (used) memcpy(out[s].key_pts, rb.at<int>(0) + 5 * M.kf_off, used * sizeof(int));
    for (size_t k = used; k < cap; ++k) out[s].key_pts[k] = -1;
  }
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_run_close(plsvo_ctx* c, int n, const plsvo_cand_frame* fr, int max_n_kfs) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->ck_live) return fail(c, PLSVO_E_STATE, "candidates_run_close: no live key-point table (plsvo_candidates_set_keypts)");
  if (const int rc = cand_seeds_pending(c, "candidates_run_close")) return rc;
  if (n != c->cd_n || (n > 0 && !fr)) return fail(c, PLSVO_E_INVALID, "candidates_run_close: n does not match the staged batch");
  if (max_n_kfs < 0) return fail(c, PLSVO_E_INVALID, "candidates_run_close: negative max_n_kfs");
  for (int s = 0; s < n; ++s) {
    if (fr[s].cur_slot < 0) return fail(c, PLSVO_E_INVALID, "candidates_run_close: negative slot");
    if (fr[s].n_overlap != 0 || fr[s].overlap_idx) return fail(c, PLSVO_E_INVALID, "candidates_run_close: the overlap list is decided on the device (n_overlap 0, overlap_idx NULL)");
  }
  return cand_run(c, n, fr, max_n_kfs);
}

extern "C" int plsvo_candidates_close_fetch(plsvo_ctx* c, int n, plsvo_close_kf_out* out) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->cd_ran || !c->ck_have_close) return fail(c, PLSVO_E_STATE, "candidates_close_fetch: the last run was no plsvo_candidates_run_close");
  if (n != c->cd_n || (n > 0 && !out)) return fail(c, PLSVO_E_INVALID, "candidates_close_fetch: n does not match the staged batch");
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  Readback rb;
  rb.add(c->ck_d_work.p, c->ck_fetch_bytes);
  if (const int rc = rb.wait(c)) return rc;
  const char* const h = rb.at<char>(0); const char* const base = reinterpret_cast<const char*>(c->ck_d_work.p);
  const KeyStageBatchDev& b = c->ck_b;
  const int* cnt = reinterpret_cast<const int*>(h + (reinterpret_cast<const char*>(b.close_counts) - base));
  const int* idx = reinterpret_cast<const int*>(h + (reinterpret_cast<const char*>(b.close_idx) - base));
  const double* dist = reinterpret_cast<const double*>(h + (reinterpret_cast<const char*>(b.close_dist) - base));
  for (int s = 0; s < n; ++s) {
    const size_t at = (size_t)c->cd_maps[(size_t)s].kf_off, nc = (size_t)cnt[2 * s];
    out[s].n_close = cnt[2 * s]; out[s].n_overlap = cnt[2 * s + 1];
    if (out[s].close_idx && nc) memcpy(out[s].close_idx, idx + at, nc * sizeof(int));
    if (out[s].close_dist && nc) memcpy(out[s].close_dist, dist + at, nc * sizeof(double));
  }
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_fetch(plsvo_ctx* c, int n, plsvo_cand_out* out) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->cd_ran) return fail(c, PLSVO_E_STATE, "candidates_fetch: no run to fetch");
  if (n != c->cd_n || (n > 0 && !out)) return fail(c, PLSVO_E_INVALID, "candidates_fetch: n does not match the staged batch");
  if (n == 0) return PLSVO_OK;
  Readback rb;   // (the fetched arrays are the first sections of the work allocation: one range)
  const int r_work = rb.add(c->cd_d_work.p, c->cd_fetch_bytes), r_kfc = rb.add(c->cd_d_kfcount.p, (size_t)c->cd_ov_off[(size_t)n] * sizeof(int));
  if (const int rc = rb.wait(c)) return rc;
  const char* const h = rb.at<char>(r_work); const int* const kfc = rb.at<int>(r_kfc);
  const CandFetchSections& F = c->cd_off;
  const int* cnt = reinterpret_cast<const int*>(h + F.counts);
  auto cp = [&](void* dst, size_t sec, size_t at, size_t count, size_t elem) { if (dst && count) memcpy(dst, h + sec + at * elem, count * elem); };
  for (int s = 0; s < n; ++s) {
    const CandMapDev& M = c->cd_maps[(size_t)s]; const CandStreamHost& H = c->cd_host[(size_t)s];
    plsvo_cand_out& O = out[s];
    const size_t np = (size_t)cnt[2 * s], ns = (size_t)cnt[2 * s + 1], po = (size_t)M.opt_off, so = (size_t)M.oseg_off;
    O.n_filed_pt = (int32_t)np; O.n_filed_seg = (int32_t)ns;
    cp(O.pt_lm, F.pt_lm, po, np, sizeof(int)); cp(O.pt_px, F.pt_px, po * 2, np * 2, sizeof(double)); cp(O.pt_cell, F.pt_cell, po, np, sizeof(int));
    cp(O.pt_obs, F.pt_obs, po, np, sizeof(int)); cp(O.pt_has_view, F.pt_view, po, np, 1); cp(O.pt_active, F.pt_active, po, np, 1);
    cp(O.seg_lm, F.seg_lm, so, ns, sizeof(int)); cp(O.seg_px, F.seg_px, so * 4, ns * 4, sizeof(double)); cp(O.seg_cell, F.seg_cell, so * 2, ns * 2, sizeof(int));
    cp(O.seg_obs, F.seg_obs, so, ns, sizeof(int)); cp(O.seg_has_view, F.seg_view, so, ns, 1); cp(O.seg_active, F.seg_active, so, ns, 1);
    cp(O.pt_cand_failed, F.pt_cand_failed, (size_t)M.ptc_off, (size_t)H.fetch_pt_cand, 1); cp(O.seg_cand_failed, F.seg_cand_failed, (size_t)M.segc_off, (size_t)H.fetch_seg_cand, 1);
    const size_t a = (size_t)c->cd_ov_off[(size_t)s], e = (size_t)c->cd_ov_off[(size_t)s + 1];
    if (O.kf_count && e > a) memcpy(O.kf_count, kfc + a, (e - a) * sizeof(int));
  }
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_match(plsvo_ctx* c) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->cd_ran) return fail(c, PLSVO_E_STATE, "candidates_match: no candidates on the device");
  if (const int rc = cand_seeds_pending(c, "candidates_match")) return rc;
  if (const int rc = cand_run_open(c, "candidates_match")) return rc;
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
  HIP_TRY_TIMED(c, PLSVO_K_MATCH, launch_match_direct(mb, c->stream));
  c->cd_matched = true;
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_match_fetch(plsvo_ctx* c, int n, plsvo_cand_match_out* out) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->cd_ran || !c->cd_matched) return fail(c, PLSVO_E_STATE, "candidates_match_fetch: no match to fetch");
  if (n != c->cd_n || (n > 0 && !out)) return fail(c, PLSVO_E_INVALID, "candidates_match_fetch: n does not match the staged batch");
  if (n == 0 || c->cd_total_m == 0) return PLSVO_OK;
  const size_t NM = c->cd_total_m;
  const MatchBatchDev& mb = c->cd_match;
  Readback rb;
  const int r_cnt = rb.add(c->cd_b.counts, (size_t)n * 2 * sizeof(int)), r_px = rb.add(mb.px_out, NM * 2 * sizeof(double)), r_lev = rb.add(mb.search_level, NM * sizeof(int)),
            r_found = rb.add(mb.found, NM);
  if (const int rc = rb.wait(c)) return rc;
  const int* cnt = rb.at<int>(r_cnt); const double* px = rb.at<double>(r_px); const int* lev = rb.at<int>(r_lev); const uint8_t* found = rb.at<uint8_t>(r_found);
  for (int s = 0; s < n; ++s) {
    const size_t at = (size_t)c->cd_maps[(size_t)s].m_off, k = (size_t)cnt[2 * s] + 2 * (size_t)cnt[2 * s + 1];
    if (!k) continue;
    if (out[s].found) memcpy(out[s].found, found + at, k);
    if (out[s].px) memcpy(out[s].px, px + 2 * at, k * 2 * sizeof(double));
    if (out[s].search_level) memcpy(out[s].search_level, lev + at, k * sizeof(int));
  }
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_dev(plsvo_ctx* c, plsvo_cand_dev* o) {
  CTX_CHECK(c);
  if (!o) return fail(c, PLSVO_E_INVALID, "candidates_dev: bad arguments");
  if (!c->cd_staged || !c->cd_ran || c->cd_n == 0 || c->ci_inserted || c->cn_closed || c->cc_closed) return fail(c, PLSVO_E_STATE, "candidates_dev: no candidates on the device");
  if (const int rc = cand_seeds_pending(c, "candidates_dev")) return rc;
  const CandBatchDev& b = c->cd_b; const MatchBatchDev& mb = c->cd_match;
  o->n_entries = (int64_t)c->cd_total_m; o->n_frames = (int64_t)c->cd_total_f;
  o->m_off = c->cd_m_off.data(); o->f_off = c->cd_f_off.data();
  o->d_counts = b.counts; o->d_frame_T = b.frame_T; o->d_frame_slot = b.frame_slot; o->d_cur_frame = b.m_cur_frame; o->d_ref_frame = b.m_ref_frame;
  o->d_ref_px = b.m_ref_px; o->d_ref_f = b.m_ref_f; o->d_ref_level = b.m_ref_level; o->d_ref_type = b.m_ref_type; o->d_ref_grad = b.m_ref_grad;
  o->d_pos = b.m_pos; o->d_px_cur = b.m_px_cur; o->d_active = b.m_active;
  o->d_found = mb.found; o->d_px_out = mb.px_out; o->d_search_level = mb.search_level;
  return PLSVO_OK;
}

// ---- the keyframe decision on the resident selection (keystage_device.hpp) ---------------------------------------------
extern "C" int plsvo_candidates_keyframe_decide(plsvo_ctx* c, int n, const plsvo_cand_kf_decide* in) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->cd_ran || !c->cs_selected || !c->cs_posed) return fail(c, PLSVO_E_STATE, "candidates_keyframe_decide: no resident pose optimisation on the last run");
  if (const int rc = cand_seeds_pending(c, "candidates_keyframe_decide")) return rc;
  if (const int rc = cand_run_open(c, "candidates_keyframe_decide")) return rc;
  if (n != c->cd_n || (n > 0 && !in)) return fail(c, PLSVO_E_INVALID, "candidates_keyframe_decide: n does not match the staged batch");
  if (n == 0) { c->ck_decided = true; return PLSVO_OK; }
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t N = (size_t)n, t_ov = (size_t)c->cd_ov_off[N];
  Blob blob;
  const size_t b_jobs = blob.reserve<KeyDecideJobDev>(N);
  if (!c->ck_decided) c->ck_dec_active.assign(N, 0);
  for (int s = 0; s < n; ++s) {
    KeyDecideJobDev& J = blob.at<KeyDecideJobDev>(b_jobs)[s];
    memset(&J, 0, sizeof(J));
    memcpy(J.T_last, in[s].T_last_w, sizeof(J.T_last)); J.d_T_last = in[s].d_T_last_w;
    J.min_t = in[s].kfselect_mindist_t; J.min_r = in[s].kfselect_mindist_r; J.active = in[s].active ? 1 : 0;
    if (J.active) c->ck_dec_active[(size_t)s] = 1;
  }
  int rc;
  if ((rc = upload_blob(c, c->ck_d_dec_in, blob))) return rc;
  Carver w;   // the records and the deltas come back with a fetch; the depth keys stay
  const size_t w_out = w.take<KfDecideOutDev>(N), w_dt = w.take<double>(t_ov), w_dr = w.take<double>(t_ov), w_keys = w.take<unsigned long long>(c->cd_t_opt + 4 * c->cd_t_oseg);   // per stream n_matches + 2 * n_ls_matches keys: a segment can be a feature twice
  HIP_TRY(c, c->ck_d_dec.ensure(w.off + 256));
  if (!c->ck_decided) HIP_TRY(c, hipMemsetAsync(c->ck_d_dec.as<char>() + w_out, 0, N * sizeof(KfDecideOutDev), c->stream));   // the run's first decision: a stream that sits it out reads as zeros, not as the run before
  KeyDecideBatchDev b{};
  b.s = c->cs_b; b.s.c.jobs = c->cd_run_jobs; b.s.c.overlap_idx = c->cd_run_ov;
  b.jobs = Blob::dev<KeyDecideJobDev>(c->ck_d_dec_in, b_jobs); b.out = Carver::dev<KfDecideOutDev>(c->ck_d_dec, w_out);
  b.poses = c->cs_w.poses.as<double>(); b.pt_keep = c->cs_w.ptkeep.as<uint8_t>(); b.seg_keep = c->cs_w.segkeep.as<uint8_t>();
  b.depth_keys = Carver::dev<unsigned long long>(c->ck_d_dec, w_keys); b.delta_t = Carver::dev<double>(c->ck_d_dec, w_dt); b.delta_r = Carver::dev<double>(c->ck_d_dec, w_dr);
  HIP_TRY_TIMED(c, PLSVO_K_KEYFRAME, launch_map_keyframe_decide(b, c->stream));
  c->ck_dec_b = b; c->ck_decided = true;
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_decide_fetch(plsvo_ctx* c, int n, plsvo_kf_decide_out* out) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->ck_decided) return fail(c, PLSVO_E_STATE, "candidates_decide_fetch: no decision on the last run");
  if (n != c->cd_n || (n > 0 && !out)) return fail(c, PLSVO_E_INVALID, "candidates_decide_fetch: n does not match the staged batch");
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const KeyDecideBatchDev& b = c->ck_dec_b;
  const size_t N = (size_t)n, t_ov = (size_t)c->cd_ov_off[N];
  bool deltas = false;
  for (int s = 0; s < n; ++s) deltas = deltas || out[s].delta_t || out[s].delta_r;
  Readback rb;   // the records: at most 64 bytes per stream; the deltas and the device-decided counts only when they are asked for
  const int r_out = rb.add(b.out, N * sizeof(KfDecideOutDev));
  const int r_dt = deltas ? rb.add(b.delta_t, t_ov * sizeof(double)) : -1, r_dr = deltas ? rb.add(b.delta_r, t_ov * sizeof(double)) : -1;
  const int r_cnt = (deltas && c->ck_have_close) ? rb.add(c->ck_b.close_counts, N * 2 * sizeof(int)) : -1;
  if (const int rc = rb.wait(c)) return rc;
  const KfDecideOutDev* ho = rb.at<KfDecideOutDev>(r_out);
  for (int s = 0; s < n; ++s) {
    const KfDecideOutDev& o = ho[s];
    plsvo_kf_decide_out& O = out[s];
    O.depth_mean = o.depth_mean; O.depth_min = o.depth_min; O.has_depth = o.has_depth; O.n_depth = o.n_depth;
    O.need_new_kf = o.need_new_kf; O.blocking = o.blocking; O.furthest_kf = o.furthest_kf;
    for (int k = 0; k < 5; ++k) O.key_pts[k] = o.key_pts[k];
    if (!deltas || !c->ck_dec_active[(size_t)s]) continue;
    const size_t at = (size_t)c->cd_ov_off[(size_t)s];
    const size_t no = r_cnt >= 0 ? (size_t)rb.at<int>(r_cnt)[2 * s + 1] : (size_t)(c->cd_ov_off[(size_t)s + 1] - c->cd_ov_off[(size_t)s]);
    if (O.delta_t && no) memcpy(O.delta_t, rb.at<double>(r_dt) + at, no * sizeof(double));
    if (O.delta_r && no) memcpy(O.delta_r, rb.at<double>(r_dr) + at, no * sizeof(double));
  }
  return PLSVO_OK;
}

// ---- cell selection of the map candidates: one per cell, landmark quality, features, pose-optimiser input (select_device.hpp) ---------
namespace {
constexpr int kInsJoinedBit = 32;                  // insert_device.hpp's kInsJoined
constexpr int kNewCandBit = 64;                    // newcand_device.hpp's kNewCand
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
  if (const int rc = cand_seeds_pending(c, "candidates_set_quality")) return rc;
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
  if (const int rc = cand_seeds_pending(c, "candidates_fetch_quality")) return rc;
  if (n != c->cd_n || (n > 0 && !out)) return fail(c, PLSVO_E_INVALID, "candidates_fetch_quality: n does not match the staged batch");
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const QualitySections q = quality_sections(c);
  const CandBatchDev& b = c->cd_b;
  Readback rb;
  const int r_q = rb.add(c->cs_d_q.p, q.end), r_maps = rb.add(b.maps, (size_t)n * sizeof(CandMapDev)), r_pty = rb.add(b.pt_type, c->cd_t_pt * sizeof(int)),
            r_sty = rb.add(b.seg_type, c->cd_t_seg * sizeof(int)), r_ptc = rb.add(b.pt_cand, c->cd_t_ptc * sizeof(int)), r_segc = rb.add(b.seg_cand, c->cd_t_segc * sizeof(int));
  if (const int rc = rb.wait(c)) return rc;
  const char* const hq = rb.at<char>(r_q); const CandMapDev* const maps = rb.at<CandMapDev>(r_maps);
  auto cp = [&](void* dst, const void* src, size_t at, size_t count, size_t elem) { if (dst && count) memcpy(dst, reinterpret_cast<const char*>(src) + at * elem, count * elem); };
  for (int s = 0; s < n; ++s) {
    const CandMapDev& M = maps[s];
    plsvo_cand_quality_out& O = out[s];
    const size_t np = (size_t)M.n_pt, ns = (size_t)M.n_seg, po = (size_t)M.pt_off, so = (size_t)M.seg_off;
    O.n_pt_cand = M.n_pt_cand; O.n_seg_cand = M.n_seg_cand;
    cp(O.pt_n_failed, hq + q.pt_nf, po, np, sizeof(int)); cp(O.pt_n_succeeded, hq + q.pt_ns, po, np, sizeof(int));
    cp(O.seg_n_failed, hq + q.seg_nf, so, ns, sizeof(int)); cp(O.seg_n_succeeded, hq + q.seg_ns, so, ns, sizeof(int));
    cp(O.pt_type, rb.at<int>(r_pty), po, np, sizeof(int)); cp(O.seg_type, rb.at<int>(r_sty), so, ns, sizeof(int));
    // (the insertion's bit sits above the selection's internal ones)
    auto public_event = [](char ev) { return (uint8_t)((ev & (PLSVO_LM_EVENT_PROMOTED | PLSVO_LM_EVENT_DELETED)) | ((ev & kInsJoinedBit) ? PLSVO_LM_EVENT_JOINED : 0) |
                                                    ((ev & kNewCandBit) ? PLSVO_LM_EVENT_NEW : 0)); };
    if (O.pt_event) for (size_t k = 0; k < np; ++k) O.pt_event[k] = public_event(hq[q.pt_ev + po + k]);
    if (O.seg_event) for (size_t k = 0; k < ns; ++k) O.seg_event[k] = public_event(hq[q.seg_ev + so + k]);
    cp(O.pt_cand, rb.at<int>(r_ptc), (size_t)M.ptc_off, (size_t)M.n_pt_cand, sizeof(int)); cp(O.seg_cand, rb.at<int>(r_segc), (size_t)M.segc_off, (size_t)M.n_seg_cand, sizeof(int));
  }
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_set_match(plsvo_ctx* c, int n, const plsvo_cand_match_out* in) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->cd_ran) return fail(c, PLSVO_E_STATE, "candidates_set_match: no candidates on the device");
  if (const int rc = cand_seeds_pending(c, "candidates_set_match")) return rc;
  if (const int rc = cand_run_open(c, "candidates_set_match")) return rc;
  if (n != c->cd_n || (n > 0 && !in)) return fail(c, PLSVO_E_INVALID, "candidates_set_match: n does not match the staged batch");
  for (int s = 0; s < n; ++s) if (!in[s].found || !in[s].px || !in[s].search_level) return fail(c, PLSVO_E_INVALID, "candidates_set_match: null array");
  if (n == 0 || c->cd_total_m == 0) { c->cd_matched = true; return PLSVO_OK; }
  HIP_TRY(c, hipSetDevice(c->device));
  Readback rb;
  rb.add(c->cd_b.counts, (size_t)n * 2 * sizeof(int));
  if (const int rc = rb.wait(c)) return rc;
  const int* cnt = rb.at<int>(0);
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
  if (const int rc = cand_seeds_pending(c, "candidates_select")) return rc;
  if (c->cs_selected) return fail(c, PLSVO_E_STATE, "candidates_select: this run's candidates were selected already (the tables have moved on)");
  if (const int rc = cand_run_open(c, "candidates_select")) return rc;   // (an insertion needs a selection: the line above has spoken for it)
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
  const auto rearm_then_launch = [&]() -> hipError_t {   // ahead of EVERY launch: the event bytes are zero, the cells' winner words all ones
    hipError_t e = hipMemsetAsync(dq + q.pt_ev, 0, q.end - q.pt_ev, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(b.cell_win, 0xff, N * (size_t)n_cells * sizeof(unsigned int), c->stream);
    return e != hipSuccess ? e : launch_map_select(b, c->stream);
  };
  HIP_TRY_TIMED(c, PLSVO_K_SELECT, rearm_then_launch());
  c->cs_selected = true;
  if (c->ck_live) return keypts_enqueue(c, c->ck_d_upkeep.as<KeyPtsJobDev>());   // removeKeyPoint of the landmarks the selection deleted
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
  Readback rb;
  rb.add(lo, (size_t)(hi - lo));
  if (const int rc = rb.wait(c)) return rc;
  auto H = [&](const void* dev) { return rb.at<char>(0) + (reinterpret_cast<const char*>(dev) - lo); };
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
  if (const int rc = cand_seeds_pending(c, "candidates_pose_optimize")) return rc;
  if (const int rc = cand_run_open(c, "candidates_pose_optimize")) return rc;
  const int n = c->cd_n;
  c->cs_posed = false;
  if (n == 0) { c->cs_posed = true; return PLSVO_OK; }
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t nft = std::max(c->cd_t_opt, (size_t)1) + std::max(2 * c->cd_t_oseg, (size_t)1);
  if (const int rc = c->cs_w.ensure(c, (size_t)n, c->cd_t_opt, 2 * c->cd_t_oseg)) return rc;
  c->cs_w.bind_resident(c->cs_pose, c->cs_b, n);
  const int threads = pose_opt_threads(c, n, (long)nft);   // (selected features <= filed landmarks)
  c->p_refill_frames = 0;                           // (jobs written on the device, as in plsvo_chain_run)
  HIP_TRY_TIMED(c, PLSVO_K_POSEOPT, launch_pose_opt(c->cs_pose, c->cs_w.poses.as<double>(), threads, c->opt_poseopt_select ? 1 : 0, c->stream));
  c->cs_posed = true;
  return PLSVO_OK;
}

extern "C" const double* plsvo_candidates_poses_dev(plsvo_ctx* c) { return (c && c->cd_staged && c->cs_posed) ? c->cs_w.poses.as<double>() : nullptr; }

extern "C" int plsvo_candidates_pose_fetch(plsvo_ctx* c, int n, plsvo_poseopt_out* out) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->cs_selected || !c->cs_posed) return fail(c, PLSVO_E_STATE, "candidates_pose_fetch: no pose optimisation to fetch");
  if (n != c->cd_n || (n > 0 && !out)) return fail(c, PLSVO_E_INVALID, "candidates_pose_fetch: n does not match the staged batch");
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t NP = std::max(c->cd_t_opt, (size_t)1), NS = std::max(2 * c->cd_t_oseg, (size_t)1);
  Readback rb;
  const int r_st = rb.add(c->cs_w.state.p, (size_t)n * sizeof(PoseStateDev)), r_jobs = rb.add(c->cs_b.po_jobs, (size_t)n * sizeof(PoseJobDev)),
            r_pk = rb.add(c->cs_w.ptkeep.p, NP), r_sk = rb.add(c->cs_w.segkeep.p, NS);
  if (const int rc = rb.wait(c)) return rc;
  for (int j = 0; j < n; ++j) {
    const PoseJobDev& J = rb.at<PoseJobDev>(r_jobs)[j];
    plsvo_poseopt_out& o = out[j];
    pose_state_to_out(rb.at<PoseStateDev>(r_st)[j], o);
    if (o.pt_keep && J.n_pts > 0) memcpy(o.pt_keep, rb.at<uint8_t>(r_pk) + J.pt_off, (size_t)J.n_pts);
    if (o.seg_keep && J.n_seg > 0) memcpy(o.seg_keep, rb.at<uint8_t>(r_sk) + J.seg_off, (size_t)J.n_seg);
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
  if (const int rc = cand_seeds_pending(c, "candidates_insert_keyframe")) return rc;
  if (c->ci_inserted) return fail(c, PLSVO_E_STATE, "candidates_insert_keyframe: this run's frame was inserted already");
  if (const int rc = cand_run_open(c, "candidates_insert_keyframe")) return rc;
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
    if (in[s].is_kf && c->cd_maps[(size_t)s].n_kf + 1 - (in[s].remove_kf >= 0 ? 1 : 0) > c->cd_host[(size_t)s].cap_kf)
      return fail(c, PLSVO_E_CAPACITY, "candidates_insert_keyframe: no room for another keyframe (plsvo_candidates_reserve)");
  const size_t N = (size_t)n;
  c->ci_last.assign(N, InsertPlanDev{});
  for (int s = 0; s < n; ++s) {
    InsertPlanDev& O = c->ci_last[(size_t)s]; const CandMapDev& M = c->cd_maps[(size_t)s]; const CandStreamHost& H = c->cd_host[(size_t)s];
    O.n_kf = M.n_kf; O.new_kf = -1; O.n_kf_pt = H.n_kf_pt; O.n_kf_seg = H.n_kf_seg; O.n_pt_obs = H.n_pt_obs; O.n_seg_obs = H.n_seg_obs; O.n_pt_cand = M.n_pt_cand; O.n_seg_cand = M.n_seg_cand;
  }
  if (!any) { c->ci_have_out = true; return PLSVO_OK; }
  HIP_TRY(c, hipSetDevice(c->device));
  // -- the records and the caller's masks, laid out like the resident masks (feature rows from opt_off / 2 * oseg_off)
  Readback rb_sc;   // (consumed into the blob below, ahead of the plan's fetch)
  if (host_masks) rb_sc.add(c->cs_b.scalars, N * 3 * sizeof(int));
  if (const int rc = host_masks ? rb_sc.wait(c) : PLSVO_OK) return rc;
  const int* const sc = host_masks ? rb_sc.at<int>(0) : nullptr;
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
    J.d_T = I.pose_source == PLSVO_INSERT_POSE_DEV ? I.d_T_f_w : I.pose_source == PLSVO_INSERT_POSE_RESIDENT ? c->cs_w.poses.as<double>() + 7 * (size_t)s : nullptr;
    J.pt_keep = c->cs_w.ptkeep.as<uint8_t>(); J.seg_keep = c->cs_w.segkeep.as<uint8_t>();
    if (I.pt_keep) { J.pt_keep = din + b_pk; if (sc[3 * (size_t)s] > 0) memcpy(blob.at<uint8_t>(b_pk) + M.opt_off, I.pt_keep, (size_t)sc[3 * (size_t)s]); }
    if (I.seg_keep) { J.seg_keep = din + b_sk; if (sc[3 * (size_t)s + 1] > 0) memcpy(blob.at<uint8_t>(b_sk) + 2 * M.oseg_off, I.seg_keep, (size_t)sc[3 * (size_t)s + 1]); }
  }
  int rc;
  if ((rc = upload_blob(c, c->ci_d_in, blob))) return rc;
  // -- scratch per landmark, per candidate entry and per new feature; staging rows of the arrays that shift
  Carver w;
  InsertBatchDev b{};
  struct { size_t f0, f1, cnt, len, erase, cand_kf, new_lm, kf_off2, kf_lm2, obs_off2, obs_kf2, obs_level2, obs_a2, obs_b2, obs_c2, obs_d2, obs_type2; } o_k[2];   // InsertKindDev's arrays
  for (int k = 0; k < 2; ++k) {
    const size_t lm = k ? c->cd_t_seg : c->cd_t_pt, cnd = k ? c->cd_t_segc : c->cd_t_ptc, ftr = k ? 2 * c->cd_t_oseg : c->cd_t_opt;
    const size_t kfl = k ? c->ci_t_kfseg : c->ci_t_kfpt, obs = k ? c->ci_t_segobs : c->ci_t_ptobs;
    const InsertKindDev& K = k ? b.seg : b.pt; auto& o = o_k[k];
    auto take = [&](auto* field, size_t n) { return w.take<std::remove_pointer_t<decltype(field)>>(n); };   // (n elements of the field's own type: `at` below casts to the same)
    o.f0 = take(K.f0, lm); o.f1 = take(K.f1, lm); o.cnt = take(K.cnt, lm); o.len = take(K.len, lm); o.erase = take(K.erase, lm);
    o.cand_kf = take(K.cand_kf, cnd); o.new_lm = take(K.new_lm, ftr); o.kf_off2 = take(K.kf_off2, c->ci_t_kf + N); o.kf_lm2 = take(K.kf_lm2, kfl); o.obs_off2 = take(K.obs_off2, lm + N);
    o.obs_kf2 = take(K.obs_kf2, obs); o.obs_level2 = take(K.obs_level2, obs); o.obs_a2 = take(K.obs_a2, obs * 2); o.obs_b2 = take(K.obs_b2, obs * (k ? 2 : 3));
    o.obs_c2 = take(K.obs_c2, obs * (k ? 3 : 2)); o.obs_d2 = take(K.obs_d2, k ? obs * 3 : 1); o.obs_type2 = take(K.obs_type2, k ? 1 : obs);
  }
  HIP_TRY(c, c->ci_d_work.ensure(w.off + 256));
  char* dw = reinterpret_cast<char*>(c->ci_d_work.p);
  for (int k = 0; k < 2; ++k) {
    InsertKindDev& K = k ? b.seg : b.pt; const auto& o = o_k[k];
    auto at = [&](auto*& field, size_t off) { field = reinterpret_cast<std::remove_reference_t<decltype(field)>>(dw + off); };   // (the array's type is the field's)
    at(K.f0, o.f0); at(K.f1, o.f1); at(K.cnt, o.cnt); at(K.len, o.len); at(K.erase, o.erase); at(K.cand_kf, o.cand_kf); at(K.new_lm, o.new_lm); at(K.kf_off2, o.kf_off2);
    at(K.kf_lm2, o.kf_lm2); at(K.obs_off2, o.obs_off2); at(K.obs_kf2, o.obs_kf2); at(K.obs_level2, o.obs_level2); at(K.obs_a2, o.obs_a2); at(K.obs_b2, o.obs_b2);
    at(K.obs_c2, o.obs_c2); at(K.obs_d2, o.obs_d2); at(K.obs_type2, o.obs_type2);
  }
  b.s = c->cs_b;
  b.jobs = reinterpret_cast<const InsertJobDev*>(din + b_jobs); b.plan = c->ci_d_plan.as<InsertPlanDev>();
  // -- the plan: decisions and counts in scratch; capacity is decided before anything is changed
  HIP_TRY(c, launch_map_insert_plan(b, c->stream));
  Readback rb;
  rb.add(b.plan, N * sizeof(InsertPlanDev));
  if ((rc = rb.wait(c))) return rc;
  const InsertPlanDev* const plan = rb.at<InsertPlanDev>(0);
  for (int s = 0; s < n; ++s) {
    if (!in[s].is_kf) continue;
    const InsertPlanDev& P = plan[(size_t)s]; const CandStreamHost& H = c->cd_host[(size_t)s];
    if (P.n_kf > H.cap_kf || P.n_kf_pt > H.cap_kf_pt || P.n_kf_seg > H.cap_kf_seg || P.n_pt_obs > H.cap_pt_obs || P.n_seg_obs > H.cap_seg_obs)
      return fail(c, PLSVO_E_CAPACITY, "candidates_insert_keyframe: a stream's new sizes exceed its room (plsvo_candidates_reserve); nothing was changed");
  }
  HIP_TRY_TIMED(c, PLSVO_K_INSERT, launch_map_insert(b, c->stream));
  if (c->ck_live) {                                 // the key-point table follows: rows close up, removeKeyPoint, the new keyframe's row
    Blob kb;
    const size_t b_kp = kb.reserve<KeyPtsJobDev>(N);
    for (int s = 0; s < n; ++s) kb.at<KeyPtsJobDev>(b_kp)[s] = in[s].is_kf ? KeyPtsJobDev{ kKeyPtsUpkeep, in[s].remove_kf, (c->ck_decided && c->ck_dec_active[(size_t)s]) ? kKeyPtsRowDecided : kKeyPtsRowFresh, 0 } : KeyPtsJobDev{ kKeyPtsStandBy, -1, kKeyPtsRowOld, 0 };
    if ((rc = upload_blob(c, c->ck_d_in, kb))) return rc;
    if ((rc = keypts_enqueue(c, Blob::dev<KeyPtsJobDev>(c->ck_d_in, b_kp)))) return rc;
  }
  // -- the host mirrors describe the new tables
  for (int s = 0; s < n; ++s) {
    if (!in[s].is_kf) { c->ci_last[(size_t)s] = plan[(size_t)s]; continue; }
    const InsertPlanDev& P = plan[(size_t)s];
    CandMapDev& M = c->cd_maps[(size_t)s]; CandStreamHost& H = c->cd_host[(size_t)s];
    int* slot = c->cd_kf_slot.data() + M.kf_off;
    if (in[s].remove_kf >= 0) for (int k = in[s].remove_kf; k + 1 < M.n_kf; ++k) slot[k] = slot[k + 1];
    slot[P.new_kf] = in[s].kf_slot;
    for (int k = P.n_kf; k < H.cap_kf; ++k) slot[k] = 0;
    M.n_kf = P.n_kf; M.n_pt_cand = P.n_pt_cand; M.n_seg_cand = P.n_seg_cand;
    H.fetch_pt_cand = P.n_pt_cand; H.fetch_seg_cand = P.n_seg_cand;
    H.n_kf_pt = P.n_kf_pt; H.n_kf_seg = P.n_kf_seg; H.n_pt_obs = P.n_pt_obs; H.n_seg_obs = P.n_seg_obs;
    c->ci_last[(size_t)s] = P;
  }
  c->cd_max_level = std::max(c->cd_max_level, c->cd_params.n_pyr_levels - 1);   // the new observations' levels are the matcher's search levels
  c->ci_inserted = true; c->ci_have_out = true; c->cc_have_out = false;   // (a compaction's report describes the tables before this)
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_capacity(plsvo_ctx* c, int n, plsvo_cand_reserve* out) {
  CTX_CHECK(c);
  if (!c->cd_staged) return fail(c, PLSVO_E_STATE, "candidates_capacity: no staged map tables");
  if (n != c->cd_n || (n > 0 && !out)) return fail(c, PLSVO_E_INVALID, "candidates_capacity: n does not match the staged batch");
  for (int s = 0; s < n; ++s) {
    const CandStreamHost& H = c->cd_host[(size_t)s];
    out[s].extra_kf = H.cap_kf; out[s].extra_kf_pt = H.cap_kf_pt; out[s].extra_kf_seg = H.cap_kf_seg; out[s].extra_pt_obs = H.cap_pt_obs; out[s].extra_seg_obs = H.cap_seg_obs; out[s].reserved0 = 0;
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
  if (const int rc = cand_seeds_pending(c, "candidates_fetch_map")) return rc;
  if (n != c->cd_n || (n > 0 && !out)) return fail(c, PLSVO_E_INVALID, "candidates_fetch_map: n does not match the staged batch");
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  Readback rb;                                     // the tables are one allocation: one range
  rb.add(c->cd_d_blob.p, c->cd_blob_bytes);
  if (const int rc = rb.wait(c)) return rc;
  const CandBatchDev& b = c->cd_b;
  const char* base = reinterpret_cast<const char*>(c->cd_d_blob.p);
  auto H = [&](const void* dev) { return rb.at<char>(0) + (reinterpret_cast<const char*>(dev) - base); };
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
  if (const int rc = cand_seeds_pending(c, "candidates_set_positions")) return rc;
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

// ---- structure optimisation on the resident map tables (structsel_device.hpp) ---------------------------------------------
extern "C" int plsvo_candidates_optimize_structure(plsvo_ctx* c, int n, const plsvo_cand_structopt* in, const plsvo_cand_structopt_params* pr) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->cd_ran || !c->cs_selected) return fail(c, PLSVO_E_STATE, "candidates_optimize_structure: no selection on the last run");
  if (const int rc = cand_seeds_pending(c, "candidates_optimize_structure")) return rc;
  if (c->co_done) return fail(c, PLSVO_E_STATE, "candidates_optimize_structure: this run's structure was optimised already (the keys have moved on)");
  if (const int rc = cand_run_open(c, "candidates_optimize_structure")) return rc;
  if (!pr || (n > 0 && !in)) return fail(c, PLSVO_E_INVALID, "candidates_optimize_structure: bad arguments");
  if (n != c->cd_n) return fail(c, PLSVO_E_INVALID, "candidates_optimize_structure: n does not match the staged batch");
  if (pr->max_n_pts < 0 || pr->n_iter_pts < 0 || pr->max_n_segs < 0 || pr->n_iter_segs < 0) return fail(c, PLSVO_E_INVALID, "candidates_optimize_structure: negative cap or iteration count");
  bool host_masks = false;
  for (int s = 0; s < n; ++s) {
    if (!in[s].active) continue;
    if ((!in[s].pt_keep || !in[s].seg_keep) && !c->cs_posed) return fail(c, PLSVO_E_STATE, "candidates_optimize_structure: no resident pose optimisation for the masks");
    if (in[s].pt_keep || in[s].seg_keep) host_masks = true;
  }
  if (n == 0) { c->co_done = c->co_have_out = true; c->co_b = StructSelBatchDev{}; return PLSVO_OK; }
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t N = (size_t)n;
  // -- the report's rows per stream: the caps, no more than a stream can select
  int cap_pt = 0, cap_seg = 0;
  for (const CandMapDev& M : c->cd_maps) { cap_pt = std::max(cap_pt, M.cap_pt); cap_seg = std::max(cap_seg, (int)std::min<long long>(2ll * M.cap_seg, INT32_MAX)); }
  const int max_pts = std::min(pr->max_n_pts, cap_pt), max_segs = std::min(pr->max_n_segs, cap_seg);
  // -- the records and the caller's masks, laid out like the resident masks (feature rows from opt_off / 2 * oseg_off)
  Readback rb_sc;
  if (host_masks) rb_sc.add(c->cs_b.scalars, N * 3 * sizeof(int));
  if (const int rc = host_masks ? rb_sc.wait(c) : PLSVO_OK) return rc;
  const int* const sc = host_masks ? rb_sc.at<int>(0) : nullptr;
  Blob blob;
  const size_t b_jobs = blob.reserve<StructSelJobDev>(N);
  const size_t b_pk = host_masks ? blob.reserve<uint8_t>(c->cd_t_opt) : 0, b_sk = host_masks ? blob.reserve<uint8_t>(2 * c->cd_t_oseg) : 0;
  HIP_TRY(c, c->co_d_in.ensure(std::max(blob.host.size(), (size_t)256)));
  const uint8_t* din = c->co_d_in.as<uint8_t>();
  StructSelJobDev* jobs = blob.at<StructSelJobDev>(b_jobs);
  for (int s = 0; s < n; ++s) {
    const plsvo_cand_structopt& I = in[s]; const CandMapDev& M = c->cd_maps[(size_t)s];
    StructSelJobDev& J = jobs[s];
    memset(&J, 0, sizeof(J));
    J.active = I.active ? 1 : 0; J.frame_id = I.frame_id;
    if (!J.active) continue;
    J.pt_keep = c->cs_w.ptkeep.as<uint8_t>(); J.seg_keep = c->cs_w.segkeep.as<uint8_t>();
    if (I.pt_keep) { J.pt_keep = din + b_pk; if (sc[3 * (size_t)s] > 0) memcpy(blob.at<uint8_t>(b_pk) + M.opt_off, I.pt_keep, (size_t)sc[3 * (size_t)s]); }
    if (I.seg_keep) { J.seg_keep = din + b_sk; if (sc[3 * (size_t)s + 1] > 0) memcpy(blob.at<uint8_t>(b_sk) + 2 * M.oseg_off, I.seg_keep, (size_t)sc[3 * (size_t)s + 1]); }
  }
  int rc;
  if ((rc = upload_blob(c, c->co_d_in, blob))) return rc;
  Carver w;
  const size_t w_cnt = w.take<int>(N * 2), w_plm = w.take<int>(N * (size_t)max_pts), w_pit = w.take<int>(N * (size_t)max_pts), w_ppos = w.take<double>(N * (size_t)max_pts * 3),
               w_slm = w.take<int>(N * (size_t)max_segs), w_sit = w.take<int>(N * (size_t)max_segs), w_ss = w.take<double>(N * (size_t)max_segs * 3),
               w_se = w.take<double>(N * (size_t)max_segs * 3);
  HIP_TRY(c, c->co_d_rep.ensure(w.off + 256));
  StructSelBatchDev b{};
  b.s = c->cs_b;
  b.jobs = reinterpret_cast<const StructSelJobDev*>(din + b_jobs);
  b.pt_last_optim = c->co_d_key.as<int>(); b.seg_last_optim = c->co_d_key.as<int>() + c->cd_t_pt;
  b.max_n_pts = max_pts; b.n_iter_pts = pr->n_iter_pts; b.max_n_segs = max_segs; b.n_iter_segs = pr->n_iter_segs;
  b.r_counts = Carver::dev<int>(c->co_d_rep, w_cnt); b.r_pt_lm = Carver::dev<int>(c->co_d_rep, w_plm); b.r_pt_iters = Carver::dev<int>(c->co_d_rep, w_pit);
  b.r_pt_pos = Carver::dev<double>(c->co_d_rep, w_ppos); b.r_seg_lm = Carver::dev<int>(c->co_d_rep, w_slm); b.r_seg_iters = Carver::dev<int>(c->co_d_rep, w_sit);
  b.r_seg_spos = Carver::dev<double>(c->co_d_rep, w_ss); b.r_seg_epos = Carver::dev<double>(c->co_d_rep, w_se);
  HIP_TRY_TIMED(c, PLSVO_K_STRUCTOPT, launch_map_optimize_structure(b, c->stream));
  c->co_b = b; c->co_rep_bytes = w.off;
  c->co_done = c->co_have_out = true;
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_structure_fetch(plsvo_ctx* c, int n, plsvo_cand_structopt_out* out) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->co_have_out) return fail(c, PLSVO_E_STATE, "candidates_structure_fetch: no structure optimisation since the tables were staged");
  if (n > 0 && !out) return fail(c, PLSVO_E_INVALID, "candidates_structure_fetch: bad arguments");
  if (n != c->cd_n) return fail(c, PLSVO_E_INVALID, "candidates_structure_fetch: n does not match the staged batch");
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const StructSelBatchDev& b = c->co_b;
  Readback rb;                                     // the report is one allocation: one range
  rb.add(c->co_d_rep.p, c->co_rep_bytes);
  if (const int rc = rb.wait(c)) return rc;
  const char* base = reinterpret_cast<const char*>(c->co_d_rep.p);
  auto H = [&](const void* dev) { return rb.at<char>(0) + (reinterpret_cast<const char*>(dev) - base); };
  auto cp = [&](void* dst, const void* dev, size_t at, size_t count, size_t elem) { if (dst && count) memcpy(dst, H(dev) + at * elem, count * elem); };
  const int* cnt = reinterpret_cast<const int*>(H(b.r_counts));
  bool fits = true;                                // the counts first, for every stream: no buffer is written unless all of them hold their entries
  for (int s = 0; s < n; ++s) {
    plsvo_cand_structopt_out& O = out[s];
    O.n_sel_pt = cnt[2 * s]; O.n_sel_seg = cnt[2 * s + 1];
    if ((O.pt_lm || O.pt_iters || O.pt_pos) && O.n_sel_pt > O.cap_pt) fits = false;
    if ((O.seg_lm || O.seg_iters || O.seg_spos || O.seg_epos) && O.n_sel_seg > O.cap_seg) fits = false;
  }
  if (!fits) return fail(c, PLSVO_E_INVALID, "candidates_structure_fetch: a stream selected more entries than its buffers' cap_pt / cap_seg hold; nothing was copied");
  for (int s = 0; s < n; ++s) {
    plsvo_cand_structopt_out& O = out[s];
    const size_t np = (size_t)O.n_sel_pt, ns = (size_t)O.n_sel_seg, po = (size_t)s * (size_t)b.max_n_pts, so = (size_t)s * (size_t)b.max_n_segs;
    cp(O.pt_lm, b.r_pt_lm, po, np, sizeof(int)); cp(O.pt_iters, b.r_pt_iters, po, np, sizeof(int)); cp(O.pt_pos, b.r_pt_pos, po * 3, np * 3, sizeof(double));
    cp(O.seg_lm, b.r_seg_lm, so, ns, sizeof(int)); cp(O.seg_iters, b.r_seg_iters, so, ns, sizeof(int));
    cp(O.seg_spos, b.r_seg_spos, so * 3, ns * 3, sizeof(double)); cp(O.seg_epos, b.r_seg_epos, so * 3, ns * 3, sizeof(double));
  }
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_set_last_optim(plsvo_ctx* c, int n, const plsvo_cand_last_optim_in* in) {
  CTX_CHECK(c);
  if (!c->cd_staged) return fail(c, PLSVO_E_STATE, "candidates_set_last_optim: no staged map tables");
  if (const int rc = cand_seeds_pending(c, "candidates_set_last_optim")) return rc;
  if (n != c->cd_n || (n > 0 && !in)) return fail(c, PLSVO_E_INVALID, "candidates_set_last_optim: n does not match the staged batch");
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  int* d = c->co_d_key.as<int>();
  for (int s = 0; s < n; ++s) {
    const CandMapDev& M = c->cd_maps[(size_t)s];
    if (in[s].pt_last_optim && M.n_pt) HIP_TRY(c, hipMemcpyAsync(d + M.pt_off, in[s].pt_last_optim, (size_t)M.n_pt * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (in[s].seg_last_optim && M.n_seg) HIP_TRY(c, hipMemcpyAsync(d + c->cd_t_pt + M.seg_off, in[s].seg_last_optim, (size_t)M.n_seg * sizeof(int), hipMemcpyHostToDevice, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // the caller's arrays are free again
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_fetch_last_optim(plsvo_ctx* c, int n, plsvo_cand_last_optim_out* out) {
  CTX_CHECK(c);
  if (!c->cd_staged) return fail(c, PLSVO_E_STATE, "candidates_fetch_last_optim: no staged map tables");
  if (const int rc = cand_seeds_pending(c, "candidates_fetch_last_optim")) return rc;
  if (n != c->cd_n || (n > 0 && !out)) return fail(c, PLSVO_E_INVALID, "candidates_fetch_last_optim: n does not match the staged batch");
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  Readback rb;
  rb.add(c->co_d_key.p, (c->cd_t_pt + c->cd_t_seg) * sizeof(int));
  if (const int rc = rb.wait(c)) return rc;
  const int* h = rb.at<int>(0);
  for (int s = 0; s < n; ++s) {
    const CandMapDev& M = c->cd_maps[(size_t)s];
    if (out[s].pt_last_optim && M.n_pt) memcpy(out[s].pt_last_optim, h + M.pt_off, (size_t)M.n_pt * sizeof(int));
    if (out[s].seg_last_optim && M.n_seg) memcpy(out[s].seg_last_optim, h + c->cd_t_pt + M.seg_off, (size_t)M.n_seg * sizeof(int));
  }
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
  for (int s = 0; s < n; ++s) { out[s].extra_pt = c->cd_host[(size_t)s].rows_pt; out[s].extra_seg = c->cd_host[(size_t)s].rows_seg; }
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_add(plsvo_ctx* c, int n, const plsvo_cand_new* in) {
  CTX_CHECK(c);
  if (!c->cd_staged) return fail(c, PLSVO_E_STATE, "candidates_add: no staged map tables");
  if (const int rc = cand_seeds_pending(c, "candidates_add")) return rc;
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
    const CandStreamHost& H = c->cd_host[(size_t)s];
    if ((long long)M.n_pt + I.n_pt > H.rows_pt || (long long)M.n_seg + I.n_seg > H.rows_seg)
      return fail(c, PLSVO_E_CAPACITY, "candidates_add: a stream lacks landmark rows (plsvo_candidates_reserve_landmarks); nothing was changed");
    // (implied by the landmark rows until a compaction frees rows of landmarks that had left the candidate list)
    if ((long long)M.n_pt_cand + I.n_pt > H.rows_pt_cand || (long long)M.n_seg_cand + I.n_seg > H.rows_seg_cand)
      return fail(c, PLSVO_E_CAPACITY, "candidates_add: a stream lacks candidate-list rows (plsvo_candidates_reserve_landmarks); nothing was changed");
    if ((long long)H.n_pt_obs + I.n_pt > H.cap_pt_obs || (long long)H.n_seg_obs + I.n_seg > H.cap_seg_obs)
      return fail(c, PLSVO_E_CAPACITY, "candidates_add: a stream lacks observation entries (plsvo_candidates_reserve); nothing was changed");
  }
  const size_t N = (size_t)n;
  c->cn_last.assign(N, plsvo_cand_add_out{});
  for (int s = 0; s < n; ++s) {
    const plsvo_cand_new& I = in[s]; const CandMapDev& M = c->cd_maps[(size_t)s];
    plsvo_cand_add_out& O = c->cn_last[(size_t)s];
    O.first_pt = I.n_pt ? M.n_pt : -1; O.first_seg = I.n_seg ? M.n_seg : -1; O.n_added_pt = I.n_pt; O.n_added_seg = I.n_seg;
  }
  c->cc_have_out = false;
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
  HIP_TRY_TIMED(c, PLSVO_K_NEWCAND, launch_map_add_candidates(b, c->stream));
  // -- the host mirrors describe the new tables (the candidate counts are upper bounds: the selection shortens the lists on the device)
  for (int s = 0; s < n; ++s) {
    CandMapDev& M = c->cd_maps[(size_t)s]; CandStreamHost& H = c->cd_host[(size_t)s];
    M.n_pt += in[s].n_pt; M.n_seg += in[s].n_seg; M.n_pt_cand += in[s].n_pt; M.n_seg_cand += in[s].n_seg;
    H.n_pt_obs += in[s].n_pt; H.n_seg_obs += in[s].n_seg;
  }
  c->cd_max_level = max_level;
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_add_fetch(plsvo_ctx* c, int n, plsvo_cand_add_out* out) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->cn_have_out) return fail(c, PLSVO_E_STATE, "candidates_add_fetch: no add since the tables were staged");
  if (const int rc = cand_seeds_pending(c, "candidates_add_fetch")) return rc;
  if (n != c->cd_n || (n > 0 && !out)) return fail(c, PLSVO_E_INVALID, "candidates_add_fetch: n does not match the staged batch");
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  Readback rb;                                     // the candidate counts as they stand are the device's
  rb.add(c->cd_b.maps, (size_t)n * sizeof(CandMapDev));
  if (const int rc = rb.wait(c)) return rc;
  for (int s = 0; s < n; ++s) {
    const CandMapDev& M = rb.at<CandMapDev>(0)[s]; const CandStreamHost& H = c->cd_host[(size_t)s];
    out[s] = c->cn_last[(size_t)s];
    out[s].n_pt = M.n_pt; out[s].n_seg = M.n_seg; out[s].n_pt_cand = M.n_pt_cand; out[s].n_seg_cand = M.n_seg_cand; out[s].n_pt_obs = H.n_pt_obs; out[s].n_seg_obs = H.n_seg_obs;
  }
  return PLSVO_OK;
}

// ---- compaction of the resident map tables over their deleted landmark rows (compact_device.hpp) ------------------------------
extern "C" int plsvo_candidates_compact(plsvo_ctx* c, int n, const plsvo_cand_compact* in) {
  CTX_CHECK(c);
  if (!c->cd_staged) return fail(c, PLSVO_E_STATE, "candidates_compact: no staged map tables");
  if (const int rc = cand_seeds_pending(c, "candidates_compact")) return rc;
  if (n != c->cd_n || (n > 0 && !in)) return fail(c, PLSVO_E_INVALID, "candidates_compact: n does not match the staged batch");
  for (int s = 0; s < n; ++s) {
    if (in[s].mode < PLSVO_COMPACT_STANDBY || in[s].mode > PLSVO_COMPACT_ROOM) return fail(c, PLSVO_E_INVALID, "candidates_compact: unknown mode");
    if (in[s].min_room_pt < 0 || in[s].min_room_seg < 0) return fail(c, PLSVO_E_INVALID, "candidates_compact: negative threshold");
  }
  const size_t N = (size_t)n;
  c->cc_closed = true; c->cc_have_out = false;      // (a compaction of nothing ends the run too: the rule does not depend on the modes)
  c->cc_last.assign(N, CompactReportDev{});
  if (n == 0) { c->cc_have_out = true; return PLSVO_OK; }
  HIP_TRY(c, hipSetDevice(c->device));
  Blob blob;
  const size_t b_jobs = blob.reserve<CompactJobDev>(N);
  for (int s = 0; s < n; ++s) {
    CompactJobDev& J = blob.at<CompactJobDev>(b_jobs)[s]; const CandStreamHost& H = c->cd_host[(size_t)s];
    J.mode = in[s].mode; J.min_room_pt = in[s].min_room_pt; J.min_room_seg = in[s].min_room_seg; J.rows_pt = H.rows_pt; J.rows_seg = H.rows_seg; J.reserved0 = 0;
  }
  int rc;
  if ((rc = upload_blob(c, c->cc_d_in, blob))) return rc;
  Carver w;
  const size_t w_rep = w.take<CompactReportDev>(N), w_pt = w.take<int>(c->cd_t_pt), w_seg = w.take<int>(c->cd_t_seg);
  HIP_TRY(c, c->cc_d_work.ensure(w.off + 256));
  c->cc_remap_off = w_pt; c->cc_remap_seg = w_seg; c->cc_work_end = w.off;
  const QualitySections q = quality_sections(c);
  char* dq = reinterpret_cast<char*>(c->cs_d_q.p);
  CompactBatchDev b{};
  b.c = c->cd_b;
  b.pt_nfail = reinterpret_cast<int*>(dq + q.pt_nf); b.pt_nsucc = reinterpret_cast<int*>(dq + q.pt_ns);
  b.seg_nfail = reinterpret_cast<int*>(dq + q.seg_nf); b.seg_nsucc = reinterpret_cast<int*>(dq + q.seg_ns);
  b.pt_event = reinterpret_cast<uint8_t*>(dq + q.pt_ev); b.seg_event = reinterpret_cast<uint8_t*>(dq + q.seg_ev);
  b.pt_key = c->co_d_key.as<int>(); b.seg_key = c->co_d_key.as<int>() + c->cd_t_pt;
  b.jobs = Blob::dev<CompactJobDev>(c->cc_d_in, b_jobs); b.report = Carver::dev<CompactReportDev>(c->cc_d_work, w_rep);
  b.pt_remap = Carver::dev<int>(c->cc_d_work, w_pt); b.seg_remap = Carver::dev<int>(c->cc_d_work, w_seg);
  HIP_TRY_TIMED(c, PLSVO_K_INSERT, launch_map_compact(b, c->stream));
  Readback rb;
  rb.add(b.report, N * sizeof(CompactReportDev));
  if ((rc = rb.wait(c))) return rc;
  c->cc_last.assign(rb.at<CompactReportDev>(0), rb.at<CompactReportDev>(0) + n);
  // -- the host mirrors describe the new tables
  for (int s = 0; s < n; ++s) {
    const CompactReportDev& R = c->cc_last[(size_t)s];
    CandMapDev& M = c->cd_maps[(size_t)s]; CandStreamHost& H = c->cd_host[(size_t)s];
    M.n_pt = R.n_pt_after; M.n_seg = R.n_seg_after; M.n_pt_cand = R.n_pt_cand_after; M.n_seg_cand = R.n_seg_cand_after;
    H.n_pt_obs = R.n_pt_obs_after; H.n_seg_obs = R.n_seg_obs_after;
  }
  c->cc_have_out = true;
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_compact_fetch(plsvo_ctx* c, int n, plsvo_cand_compact_out* out) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->cc_have_out) return fail(c, PLSVO_E_STATE, "candidates_compact_fetch: no compaction, or the tables have moved since the last one");
  if (n != c->cd_n || (n > 0 && !out)) return fail(c, PLSVO_E_INVALID, "candidates_compact_fetch: n does not match the staged batch");
  bool remaps = false;
  for (int s = 0; s < n; ++s) {
    const CompactReportDev& R = c->cc_last[(size_t)s]; plsvo_cand_compact_out& O = out[s];
    static_assert(sizeof(CompactReportDev) == 18 * sizeof(int32_t) && offsetof(plsvo_cand_compact_out, pt_remap) >= sizeof(CompactReportDev), "the device's report is the head of the public one");
    memcpy(&O, &R, sizeof(R));
    if ((O.pt_remap && R.ran_pt) || (O.seg_remap && R.ran_seg)) remaps = true;
  }
  Readback rb;
  if (remaps) {
    HIP_TRY(c, hipSetDevice(c->device));
    rb.add(Carver::dev<char>(c->cc_d_work, c->cc_remap_off), c->cc_work_end - c->cc_remap_off);   // both remaps are one range
    if (const int rc = rb.wait(c)) return rc;
  }
  for (int s = 0; s < n; ++s) {
    const CompactReportDev& R = c->cc_last[(size_t)s]; plsvo_cand_compact_out& O = out[s]; const CandMapDev& M = c->cd_maps[(size_t)s];
    const int* const hp = remaps ? rb.at<int>(0) + M.pt_off : nullptr;
    const int* const hs = remaps ? reinterpret_cast<const int*>(rb.at<char>(0) + (c->cc_remap_seg - c->cc_remap_off)) + M.seg_off : nullptr;
    if (O.pt_remap) for (int k = 0; k < R.n_pt_before; ++k) O.pt_remap[k] = R.ran_pt ? hp[k] : k;
    if (O.seg_remap) for (int k = 0; k < R.n_seg_before; ++k) O.seg_remap[k] = R.ran_seg ? hs[k] : k;
  }
  return PLSVO_OK;
}

// ---- the next frame's alignment job from the resident selection (alignjob_device.hpp) ------------------------------------------
namespace {
// the sections of aj_d_batch (the resident alignment batch, rows by capacity) and of aj_d_out (reports, reference poses, composed poses)
struct AlignJobSections { size_t jobs, T0, pt_px, pt_xyz, spx, epx, len, sp, sq, alive, slot, rank, obs, end, o_report, o_tref, o_poses, o_key, o_end; };
static AlignJobSections align_job_sections(size_t n, const plsvo_cand_align_cfg& g) {
  const size_t np = n * (size_t)g.cap_pts, ns = n * (size_t)g.cap_seg, nl = (size_t)(g.max_level - g.min_level + 1);
  Carver w; AlignJobSections o;
  o.jobs = w.take<AlignJobDev>(n); o.T0 = w.take<double>(n * 7); o.pt_px = w.take<double>(np * 2); o.pt_xyz = w.take<double>(np * 3);
  o.spx = w.take<double>(ns * 2); o.epx = w.take<double>(ns * 2); o.len = w.take<double>(ns); o.sp = w.take<double>(ns * 3); o.sq = w.take<double>(ns * 3);
  o.alive = w.take<uint8_t>(ns); o.slot = w.take<int>(nl * ns); o.rank = w.take<int>(ns); o.obs = w.take<int>(ns); o.end = w.off;   // (obs: a keyframe build's scratch, behind the codes' 0xff fill)
  Carver v;
  o.o_report = v.take<AlignBuildReportDev>(n); o.o_tref = v.take<double>(n * 7); o.o_poses = v.take<double>(n * 7); o.o_key = v.take<int>(n); o.o_end = v.off;   // (o_key: the patch count of every stream's last build, the launch-order key)
  return o;
}
static int align_patch_cap(const plsvo_cand_align_cfg& g) { return (g.slot_cap + 3) & ~3; }
// the work buffers of the alignment launch for a batch of n streams of the reserved capacities (plsvo_align_stage sizes the same ones: none shrinks)
static int align_job_work(plsvo_ctx* c, size_t n, const plsvo_cand_align_cfg& g) {
  const size_t pt = std::max(n * (size_t)align_patch_cap(g), (size_t)4), npt_total = n * (size_t)g.cap_pts + 32;
  HIP_TRY(c, c->a_d_alive.ensure(std::max(n * (size_t)g.cap_seg, (size_t)1)));
  HIP_TRY(c, c->a_d_state.ensure(n * sizeof(AlignStateDev)));
  HIP_TRY(c, c->a_d_poses.ensure(n * 7 * sizeof(double)));
  HIP_TRY(c, c->a_d_pxyz.ensure(pt * 3 * sizeof(double)));
  HIP_TRY(c, c->a_d_puv.ensure(pt * 2 * sizeof(float)));
  HIP_TRY(c, c->a_d_cref.ensure(pt * 64));
  HIP_TRY(c, c->a_d_chi.ensure(2 * npt_total * 16 * sizeof(float)));
  if (c->a_trace_cap > 0) HIP_TRY(c, c->a_d_log.ensure(n * (size_t)c->a_trace_cap * sizeof(plsvo_align_iterlog)));
  return PLSVO_OK;
}
// behind a build's launch: its launch order, and the built batch becomes the context's staged alignment batch (the host's view of it
// holds the capacities; aj_slots: per stream the pyramid slots of its last build)
static int align_job_adopt(plsvo_ctx* c, const AlignBuildBatchDev& b, int n, int seg_align) {
  const plsvo_cand_align_cfg& g = c->aj_cfg;
  const size_t N = (size_t)n;
  // launch order: most patches (summed over the levels) first, by the counting sort that re-orders a re-run batch (bins of four patches),
  // on the build's own key -- a stream that sat the build out keeps its last count -- into a buffer no later launch's re-ordering writes
  const int* order = nullptr;
  if (!c->env_align_no_lpt) {
    HIP_TRY(c, launch_align_reorder(b.work_key, n, c->aj_d_order.as<int>(), 2, c->stream));
    order = c->aj_d_order.as<int>();
  }
  // -- the built batch is the context's staged alignment batch; the host's view of it holds the capacities
  const int patch_cap = b.patch_cap;
  c->a_jobs.assign(N, AlignJobDev{});
  for (int j = 0; j < n; ++j) {
    AlignJobDev& J = c->a_jobs[(size_t)j];
    J.ref_slot = c->aj_slots[2 * (size_t)j]; J.cur_slot = c->aj_slots[2 * (size_t)j + 1];
    J.max_level = g.max_level; J.min_level = g.min_level; J.n_iter = g.n_iter; J.eps = g.eps;
    J.pt_off = j * g.cap_pts; J.n_pts = g.cap_pts; J.seg_off = j * g.cap_seg; J.n_seg = g.cap_seg; J.patch_off = j * patch_cap; J.patch_cap = patch_cap;
  }
  AlignBatchDev& a = c->a_b;
  a.jobs = b.a_jobs; a.state = c->a_d_state.as<AlignStateDev>(); a.T0 = b.T0;
  a.pt_px = b.pt_px; a.pt_xyz = b.pt_xyz; a.seg_spx = b.seg_spx; a.seg_epx = b.seg_epx; a.seg_len = b.seg_len; a.seg_p = b.seg_p; a.seg_q = b.seg_q;
  a.seg_alive_in = b.seg_alive_in; a.seg_alive = c->a_d_alive.as<uint8_t>();
  a.patch_xyz = c->a_d_pxyz.as<double>(); a.patch_uvref = c->a_d_puv.as<float>(); a.cache_ref = c->a_d_cref.as<float>();
  a.chi_terms = c->a_d_chi.as<float>(); a.chi_plane = (unsigned long long)(N * (size_t)g.cap_pts + 32) * 16;
  a.seg_slot = b.seg_slot; a.slot_level0 = g.min_level; a.slot_stride = n * g.cap_seg;
  a.poses = c->a_d_poses.as<double>();
  a.pyr = c->pyr;
  a.log = c->a_trace_cap > 0 ? c->a_d_log.as<plsvo_align_iterlog>() : nullptr;
  a.log_cap = c->a_trace_cap;
  a.n_jobs = n;
  a.pair = 0; a.xseq0 = 0; a.xbuf = nullptr; a.work_key = nullptr; a.tail_n = 0; a.static_solve = 1; a.tail_flag = nullptr; a.seg_alive_tail = nullptr;   // (plsvo_align_run decides)
  a.order = order;
  c->a_stage_order = order;
  c->a_patch_total = std::max(N * (size_t)patch_cap, (size_t)4);
  c->a_n = n; c->a_total_seg = n * g.cap_seg; c->a_gmax = g.max_level; c->a_gmin = g.min_level;
  for (int l = 0; l < PLSVO_MAX_LEVELS; ++l) c->a_cap[l] = (l >= g.min_level && l <= g.max_level) ? patch_cap : 0;
  c->a_scap = std::max(4, g.cap_seg);
  c->a_seg_align = seg_align;
  c->a_staged = true; c->a_run_seq = 0;
  c->aj_built = true; c->aj_composed = false;
  return PLSVO_OK;
}
}  // namespace

extern "C" int plsvo_candidates_align_reserve(plsvo_ctx* c, const plsvo_cand_align_cfg* g) {
  CTX_CHECK(c);
  if (!g) return fail(c, PLSVO_E_INVALID, "candidates_align_reserve: bad arguments");
  if (!c->cd_staged) return fail(c, PLSVO_E_STATE, "candidates_align_reserve: no staged map tables");
  if (!c->pyr.base) return fail(c, PLSVO_E_STATE, "candidates_align_reserve: pyramids not configured");
  if (g->max_level < g->min_level || g->min_level < 0 || g->max_level >= c->pyr.n_levels || g->n_iter < 0)
    return fail(c, PLSVO_E_INVALID, "candidates_align_reserve: bad parameters (levels must exist in the configured pyramid)");
  if (g->cap_pts <= 0 || g->cap_seg <= 0 || g->slot_cap <= 0) return fail(c, PLSVO_E_INVALID, "candidates_align_reserve: non-positive capacity");
  if (c->cd_b.cam_width != c->pyr.w[0] || c->cd_b.cam_height != c->pyr.h[0])
    return fail(c, PLSVO_E_INVALID, "candidates_align_reserve: the staged camera's size does not match the configured pyramid");
  const int n = c->cd_n, patch_cap = align_patch_cap(*g), scap = (std::max(g->cap_seg, 4) + 3) & ~3;
  // the shape plsvo_align_run launches a batch of this many streams with: few streams get many threads, and more LDS per slot
  int run_threads = 64, run_chi = 0; size_t run_lds = 0;
  pick_align_config(c, std::max(n, 1), std::max(patch_cap, 4), scap, g->cap_pts, &run_threads, &run_lds, &run_chi);
  if (g->slot_cap > kAlignJobMaxSlotCap || g->cap_seg >= (1 << 20) || run_lds > c->lds_per_block)
    return fail(c, PLSVO_E_CAPACITY, "candidates_align_reserve: slot tables of these capacities do not fit a workgroup's LDS at " + std::to_string(run_threads) + " threads per frame");
  const long long rows = std::max<long long>(std::max(g->cap_pts, g->cap_seg), patch_cap);
  if ((long long)std::max(n, 1) * rows * (g->max_level - g->min_level + 1) > (long long)0x7fffffff / 16)
    return fail(c, PLSVO_E_CAPACITY, "candidates_align_reserve: batch too large (row index overflow)");
  HIP_TRY(c, hipSetDevice(c->device));
  if (c->aj_built) c->a_staged = false;             // the built batch's rows are laid out anew
  c->aj_reserved = c->aj_built = c->aj_composed = false;
  const size_t N = (size_t)n;
  const AlignJobSections o = align_job_sections(N, *g);
  HIP_TRY(c, c->aj_d_batch.ensure(o.end + 256));
  HIP_TRY(c, c->aj_d_out.ensure(o.o_end + 256));
  if (const int rc = align_job_work(c, N, *g)) return rc;
  // every stream starts with an empty job (skip) at the identity; codes -1, reports zero
  std::vector<AlignJobDev> jobs(N);
  std::vector<double> ident(N * 7, 0.0);
  for (int j = 0; j < n; ++j) {
    AlignJobDev& J = jobs[(size_t)j];
    memset(&J, 0, sizeof(J));
    J.fx = c->cd_b.fx; J.fy = c->cd_b.fy; J.cx = c->cd_b.cx; J.cy = c->cd_b.cy; J.width = c->cd_b.cam_width; J.height = c->cd_b.cam_height;
    J.max_level = g->max_level; J.min_level = g->min_level; J.n_iter = g->n_iter; J.skip = 1; J.eps = g->eps;
    J.pt_off = j * g->cap_pts; J.seg_off = j * g->cap_seg; J.patch_off = j * patch_cap; J.patch_cap = patch_cap; J.ldlt_flavour = c->ldlt_flavour;
    ident[(size_t)j * 7 + 3] = 1.0;
  }
  char* db = c->aj_d_batch.as<char>(); char* dout = c->aj_d_out.as<char>();
  HIP_TRY(c, hipMemsetAsync(db, 0, o.end, c->stream));
  HIP_TRY(c, hipMemsetAsync(db + o.slot, 0xff, o.rank - o.slot, c->stream));
  HIP_TRY(c, hipMemsetAsync(dout, 0, o.o_end, c->stream));
  HIP_TRY(c, hipMemsetAsync(c->a_d_alive.p, 0, c->a_d_alive.cap, c->stream));
  if (n > 0) {
    HIP_TRY(c, hipMemcpyAsync(db + o.jobs, jobs.data(), N * sizeof(AlignJobDev), hipMemcpyHostToDevice, c->stream));
    for (char* dst : { db + o.T0, dout + o.o_tref, dout + o.o_poses })
      HIP_TRY(c, hipMemcpyAsync(dst, ident.data(), N * 7 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the host vectors above are read by the copies)
  AlignBuildBatchDev& b = c->aj_b;
  b = AlignBuildBatchDev{};
  b.report = reinterpret_cast<AlignBuildReportDev*>(dout + o.o_report);
  b.a_jobs = reinterpret_cast<AlignJobDev*>(db + o.jobs); b.T0 = reinterpret_cast<double*>(db + o.T0); b.T_ref = reinterpret_cast<double*>(dout + o.o_tref);
  b.pt_px = reinterpret_cast<double*>(db + o.pt_px); b.pt_xyz = reinterpret_cast<double*>(db + o.pt_xyz);
  b.seg_spx = reinterpret_cast<double*>(db + o.spx); b.seg_epx = reinterpret_cast<double*>(db + o.epx); b.seg_len = reinterpret_cast<double*>(db + o.len);
  b.seg_p = reinterpret_cast<double*>(db + o.sp); b.seg_q = reinterpret_cast<double*>(db + o.sq); b.seg_alive_in = reinterpret_cast<uint8_t*>(db + o.alive);
  b.seg_slot = reinterpret_cast<int*>(db + o.slot); b.seg_rank = reinterpret_cast<int*>(db + o.rank);
  b.work_key = reinterpret_cast<int*>(dout + o.o_key);
  b.cap_pts = g->cap_pts; b.cap_seg = g->cap_seg; b.slot_cap = g->slot_cap; b.patch_cap = patch_cap;
  b.max_level = g->max_level; b.min_level = g->min_level; b.n_iter = g->n_iter; b.eps = g->eps;
  c->aj_pose = AlignPoseBatchDev{ nullptr, b.T_ref, reinterpret_cast<double*>(dout + o.o_poses), n };
  c->aj_seg_obs = reinterpret_cast<int*>(db + o.obs);
  c->aj_cfg = *g; c->aj_n = n; c->aj_slots.assign(2 * N, 0); c->aj_kf_slots.assign(N, std::vector<int>());
  c->aj_reserved = true;
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_align_build(plsvo_ctx* c, int n, const plsvo_cand_align_job* in) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->aj_reserved || c->aj_n != c->cd_n) return fail(c, PLSVO_E_STATE, "candidates_align_build: no alignment batch reserved for the staged streams (plsvo_candidates_align_reserve)");
  if (!c->cd_ran || !c->cs_selected) return fail(c, PLSVO_E_STATE, "candidates_align_build: no selection on the last run");
  if (const int rc = cand_seeds_pending(c, "candidates_align_build")) return rc;
  if (c->cc_closed) return fail(c, PLSVO_E_STATE, "candidates_align_build: the tables were compacted behind this run (the selection's rows have been renumbered); build ahead of the compaction");
  if (n != c->cd_n || (n > 0 && !in)) return fail(c, PLSVO_E_INVALID, "candidates_align_build: n does not match the staged batch");
  const plsvo_cand_align_cfg& g = c->aj_cfg;
  if (!c->pyr.base || g.max_level >= c->pyr.n_levels || c->cd_b.cam_width != c->pyr.w[0] || c->cd_b.cam_height != c->pyr.h[0])
    return fail(c, PLSVO_E_STATE, "candidates_align_build: the pyramids or the camera changed since the reserve");
  bool host_masks = false;
  for (int s = 0; s < n; ++s) {
    const plsvo_cand_align_job& I = in[s];
    if (!I.active) continue;
    if (I.ref_slot < 0 || I.ref_slot >= c->pyr.n_slots || I.cur_slot < 0 || I.cur_slot >= c->pyr.n_slots) return fail(c, PLSVO_E_INVALID, "candidates_align_build: pyramid slot out of range");
    if (I.pose_source < PLSVO_INSERT_POSE_HOST || I.pose_source > PLSVO_INSERT_POSE_RESIDENT || (I.pose_source == PLSVO_INSERT_POSE_DEV && !I.d_T_f_w))
      return fail(c, PLSVO_E_INVALID, "candidates_align_build: bad pose source");
    if (I.pt_keep || I.seg_keep) host_masks = true;
  }
  for (int s = 0; s < n; ++s)
    if (in[s].active && (!in[s].pt_keep || !in[s].seg_keep || in[s].pose_source == PLSVO_INSERT_POSE_RESIDENT) && !c->cs_posed)
      return fail(c, PLSVO_E_STATE, "candidates_align_build: no resident pose optimisation for the masks or the pose");
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t N = (size_t)n;
  // -- the records and the caller's masks, laid out like the resident masks (feature rows from opt_off / 2 * oseg_off)
  Readback rb_sc;
  if (host_masks) rb_sc.add(c->cs_b.scalars, N * 3 * sizeof(int));
  if (const int rc = host_masks ? rb_sc.wait(c) : PLSVO_OK) return rc;
  const int* const sc = host_masks ? rb_sc.at<int>(0) : nullptr;
  Blob blob;
  const size_t b_jobs = blob.reserve<AlignBuildJobDev>(N);
  const size_t b_pk = host_masks ? blob.reserve<uint8_t>(c->cd_t_opt) : 0, b_sk = host_masks ? blob.reserve<uint8_t>(2 * c->cd_t_oseg) : 0;
  HIP_TRY(c, c->aj_d_in.ensure(std::max(blob.host.size(), (size_t)256)));
  const uint8_t* din = c->aj_d_in.as<uint8_t>();
  AlignBuildJobDev* jobs = blob.at<AlignBuildJobDev>(b_jobs);
  for (int s = 0; s < n; ++s) {
    const plsvo_cand_align_job& I = in[s]; const CandMapDev& M = c->cd_maps[(size_t)s];
    AlignBuildJobDev& J = jobs[s];
    memset(&J, 0, sizeof(J));
    J.active = I.active ? 1 : 0;
    if (!J.active) continue;
    J.ref_slot = I.ref_slot; J.cur_slot = I.cur_slot;
    memcpy(J.T, I.T_f_w, sizeof(J.T));
    J.d_T = I.pose_source == PLSVO_INSERT_POSE_DEV ? I.d_T_f_w : I.pose_source == PLSVO_INSERT_POSE_RESIDENT ? c->cs_w.poses.as<double>() + 7 * (size_t)s : nullptr;
    J.pt_keep = c->cs_w.ptkeep.as<uint8_t>(); J.seg_keep = c->cs_w.segkeep.as<uint8_t>();
    if (I.pt_keep) { J.pt_keep = din + b_pk; if (sc[3 * (size_t)s] > 0) memcpy(blob.at<uint8_t>(b_pk) + M.opt_off, I.pt_keep, (size_t)sc[3 * (size_t)s]); }
    if (I.seg_keep) { J.seg_keep = din + b_sk; if (sc[3 * (size_t)s + 1] > 0) memcpy(blob.at<uint8_t>(b_sk) + 2 * M.oseg_off, I.seg_keep, (size_t)sc[3 * (size_t)s + 1]); }
  }
  int rc;
  if ((rc = align_job_work(c, N, g))) return rc;
  HIP_TRY(c, c->aj_d_order.ensure(N * sizeof(int)));
  if ((rc = upload_blob(c, c->aj_d_in, blob))) return rc;
  // small batches may run two workgroups per frame (plsvo_align_run decides from the launch shape): their segments start at a multiple of 64 slots
  const int cus = c->cu_count > 0 ? c->cu_count : 256;
  const int seg_align = (2 * n <= cus) ? 64 : 32;
  AlignBuildBatchDev b = c->aj_b;
  b.s = c->cs_b;
  b.jobs = Blob::dev<AlignBuildJobDev>(c->aj_d_in, b_jobs);
  b.seg_align = seg_align; b.ldlt_flavour = c->ldlt_flavour;
  c->a_staged = false; c->aj_built = false;
  c->ch_staged = false;                             // a resident frame step is built on the staged alignment batch: building another one invalidates it
  HIP_TRY_TIMED(c, PLSVO_K_ALIGN_INIT, launch_map_align_job(b, c->stream));
  for (int s = 0; s < n; ++s) if (in[s].active) { c->aj_slots[2 * (size_t)s] = in[s].ref_slot; c->aj_slots[2 * (size_t)s + 1] = in[s].cur_slot; c->aj_kf_slots[(size_t)s].clear(); }
  return align_job_adopt(c, b, n, seg_align);
}

// relocalizeFrame's and the first frame's job: a keyframe row of the resident tables as the reference frame (map_align_kf_job_kernel)
extern "C" int plsvo_candidates_align_build_kf(plsvo_ctx* c, int n, const plsvo_cand_align_kf_job* in) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->aj_reserved || c->aj_n != c->cd_n) return fail(c, PLSVO_E_STATE, "candidates_align_build_kf: no alignment batch reserved for the staged streams (plsvo_candidates_align_reserve)");
  if (const int rc = cand_seeds_pending(c, "candidates_align_build_kf")) return rc;
  if (n != c->cd_n || (n > 0 && !in)) return fail(c, PLSVO_E_INVALID, "candidates_align_build_kf: n does not match the staged batch");
  const plsvo_cand_align_cfg& g = c->aj_cfg;
  if (!c->pyr.base || g.max_level >= c->pyr.n_levels || c->cd_b.cam_width != c->pyr.w[0] || c->cd_b.cam_height != c->pyr.h[0])
    return fail(c, PLSVO_E_STATE, "candidates_align_build_kf: the pyramids or the camera changed since the reserve");
  bool closest = false;
  for (int s = 0; s < n; ++s) {
    const plsvo_cand_align_kf_job& I = in[s];
    if (!I.active) continue;
    const CandMapDev& M = c->cd_maps[(size_t)s];
    if (I.ref_kf != PLSVO_ALIGN_REF_CLOSEST && (I.ref_kf < 0 || I.ref_kf >= M.n_kf)) return fail(c, PLSVO_E_INVALID, "candidates_align_build_kf: no such keyframe row");
    if (I.cur_slot < 0 || I.cur_slot >= c->pyr.n_slots) return fail(c, PLSVO_E_INVALID, "candidates_align_build_kf: pyramid slot out of range");
    for (int k = 0; k < M.n_kf; ++k)
      if ((I.ref_kf == PLSVO_ALIGN_REF_CLOSEST || I.ref_kf == k) && (c->cd_kf_slot[(size_t)M.kf_off + (size_t)k] < 0 || c->cd_kf_slot[(size_t)M.kf_off + (size_t)k] >= c->pyr.n_slots))
        return fail(c, PLSVO_E_INVALID, "candidates_align_build_kf: a keyframe's pyramid slot is out of range");
    if (I.init_source < PLSVO_ALIGN_INIT_HOST || I.init_source > PLSVO_ALIGN_INIT_KEYFRAME || (I.init_source == PLSVO_ALIGN_INIT_DEV && !I.d_T_init))
      return fail(c, PLSVO_E_INVALID, "candidates_align_build_kf: bad source of the initial pose");
    if (I.ref_kf == PLSVO_ALIGN_REF_CLOSEST) {
      if ((I.last_source != PLSVO_INSERT_POSE_HOST && I.last_source != PLSVO_INSERT_POSE_DEV) || (I.last_source == PLSVO_INSERT_POSE_DEV && !I.d_T_last))
        return fail(c, PLSVO_E_INVALID, "candidates_align_build_kf: bad source of the last frame's pose");
      if (I.self_kf < -1 || I.self_kf >= M.n_kf) return fail(c, PLSVO_E_INVALID, "candidates_align_build_kf: self_kf is no keyframe row");
      closest = true;
    }
  }
  if (closest && !c->ck_live) return fail(c, PLSVO_E_STATE, "candidates_align_build_kf: the closest keyframe needs a live key-point table (plsvo_candidates_set_keypts)");
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t N = (size_t)n;
  Blob blob;
  const size_t b_jobs = blob.reserve<AlignKfJobDev>(N);
  for (int s = 0; s < n; ++s) {
    const plsvo_cand_align_kf_job& I = in[s];
    AlignKfJobDev& J = blob.at<AlignKfJobDev>(b_jobs)[s];
    memset(&J, 0, sizeof(J));
    J.active = I.active ? 1 : 0;
    if (!J.active) continue;
    J.ref_kf = I.ref_kf; J.self_kf = I.ref_kf == PLSVO_ALIGN_REF_CLOSEST ? I.self_kf : -1; J.init_source = I.init_source; J.cur_slot = I.cur_slot;
    memcpy(J.T_init, I.T_init, sizeof(J.T_init)); J.d_T_init = I.init_source == PLSVO_ALIGN_INIT_DEV ? I.d_T_init : nullptr;
    if (I.ref_kf == PLSVO_ALIGN_REF_CLOSEST) { memcpy(J.T_last, I.T_last, sizeof(J.T_last)); J.d_T_last = I.last_source == PLSVO_INSERT_POSE_DEV ? I.d_T_last : nullptr; }
  }
  int rc;
  if ((rc = align_job_work(c, N, g))) return rc;
  HIP_TRY(c, c->aj_d_order.ensure(N * sizeof(int)));
  if ((rc = upload_blob(c, c->aj_d_kf_in, blob))) return rc;
  const int cus = c->cu_count > 0 ? c->cu_count : 256;
  const int seg_align = (2 * n <= cus) ? 64 : 32;   // as plsvo_candidates_align_build lays out: the two compose on one batch
  AlignKfBatchDev k{};
  k.a = c->aj_b;
  k.a.s = SelectBatchDev{}; k.a.s.c = c->cd_b;      // the tables alone: no selection is read
  k.a.seg_align = seg_align; k.a.ldlt_flavour = c->ldlt_flavour;
  k.jobs = Blob::dev<AlignKfJobDev>(c->aj_d_kf_in, b_jobs);
  k.keypts = c->ck_live ? c->ck_d_keypts.as<int>() : nullptr;
  k.seg_obs = c->aj_seg_obs;
  c->a_staged = false; c->aj_built = false;
  c->ch_staged = false;                             // (as plsvo_candidates_align_build)
  HIP_TRY_TIMED(c, PLSVO_K_ALIGN_INIT, launch_map_align_kf_job(k, c->stream));
  for (int s = 0; s < n; ++s) {
    const plsvo_cand_align_kf_job& I = in[s];
    if (!I.active) continue;
    const CandMapDev& M = c->cd_maps[(size_t)s];
    const int* slot = c->cd_kf_slot.data() + M.kf_off;
    std::vector<int>& may = c->aj_kf_slots[(size_t)s];
    may.clear();
    if (I.ref_kf == PLSVO_ALIGN_REF_CLOSEST) may.assign(slot, slot + M.n_kf);   // the device picks the row: the launch may read any of them
    c->aj_slots[2 * (size_t)s] = I.ref_kf == PLSVO_ALIGN_REF_CLOSEST ? I.cur_slot : slot[I.ref_kf]; c->aj_slots[2 * (size_t)s + 1] = I.cur_slot;
  }
  return align_job_adopt(c, k.a, n, seg_align);
}

extern "C" int plsvo_candidates_align_compose(plsvo_ctx* c) {
  CTX_CHECK(c);
  if (!c->aj_reserved || !c->aj_built || !c->a_staged || c->a_run_seq == 0) return fail(c, PLSVO_E_STATE, "candidates_align_compose: the built alignment batch has not run");
  HIP_TRY(c, hipSetDevice(c->device));
  AlignPoseBatchDev b = c->aj_pose;
  b.align_poses = c->a_d_poses.as<double>(); b.n_jobs = c->a_n;
  HIP_TRY_TIMED(c, PLSVO_K_ALIGN_INIT, launch_map_align_pose(b, c->stream));
  c->aj_composed = true;
  return PLSVO_OK;
}

extern "C" const double* plsvo_candidates_align_poses_dev(plsvo_ctx* c) { return (c && c->aj_reserved && c->aj_composed) ? c->aj_pose.out : nullptr; }

extern "C" int plsvo_candidates_align_fetch(plsvo_ctx* c, int n, plsvo_cand_align_report* out) {
  CTX_CHECK(c);
  if (!c->aj_reserved) return fail(c, PLSVO_E_STATE, "candidates_align_fetch: no alignment batch reserved");
  if (n != c->aj_n || (n > 0 && !out)) return fail(c, PLSVO_E_INVALID, "candidates_align_fetch: n does not match the reserved batch");
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  static_assert(sizeof(AlignBuildReportDev) == sizeof(plsvo_cand_align_report) && sizeof(plsvo_cand_align_report) == 32, "the device's report is the public one");
  Readback rb;
  rb.add(c->aj_b.report, (size_t)n * sizeof(AlignBuildReportDev));
  if (const int rc = rb.wait(c)) return rc;
  memcpy(out, rb.at<AlignBuildReportDev>(0), (size_t)n * sizeof(AlignBuildReportDev));
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_align_fetch_job(plsvo_ctx* c, int stream, plsvo_cand_align_job_out* O) {
  CTX_CHECK(c);
  if (!c->aj_reserved) return fail(c, PLSVO_E_STATE, "candidates_align_fetch_job: no alignment batch reserved");
  if (stream < 0 || stream >= c->aj_n || !O) return fail(c, PLSVO_E_INVALID, "candidates_align_fetch_job: bad arguments");
  HIP_TRY(c, hipSetDevice(c->device));
  const AlignBuildBatchDev& b = c->aj_b; const plsvo_cand_align_cfg& g = c->aj_cfg;
  const size_t s = (size_t)stream, np = (size_t)g.cap_pts, ns = (size_t)g.cap_seg, nl = (size_t)(g.max_level - g.min_level + 1), stride = (size_t)c->aj_n * ns;
  Readback rb;
  const int r_job = rb.add(b.a_jobs + s, sizeof(AlignJobDev)), r_T0 = rb.add(b.T0 + 7 * s, 7 * sizeof(double)), r_Tr = rb.add(b.T_ref + 7 * s, 7 * sizeof(double));
  const int r_Tc = rb.add(c->aj_pose.out + 7 * s, 7 * sizeof(double));
  const int r_key = rb.add(b.work_key + s, sizeof(int));
  const int r_ppx = rb.add(b.pt_px + 2 * s * np, 2 * np * sizeof(double)), r_pxyz = rb.add(b.pt_xyz + 3 * s * np, 3 * np * sizeof(double));
  const int r_spx = rb.add(b.seg_spx + 2 * s * ns, 2 * ns * sizeof(double)), r_epx = rb.add(b.seg_epx + 2 * s * ns, 2 * ns * sizeof(double));
  const int r_len = rb.add(b.seg_len + s * ns, ns * sizeof(double)), r_sp = rb.add(b.seg_p + 3 * s * ns, 3 * ns * sizeof(double)), r_sq = rb.add(b.seg_q + 3 * s * ns, 3 * ns * sizeof(double));
  const int r_al = rb.add(b.seg_alive_in + s * ns, ns);
  std::vector<int> r_code(nl);
  for (size_t l = 0; l < nl; ++l) r_code[l] = rb.add(b.seg_slot + l * stride + s * ns, ns * sizeof(int));
  if (const int rc = rb.wait(c)) return rc;
  const AlignJobDev& J = *rb.at<AlignJobDev>(r_job);
  if (J.n_pts < 0 || J.n_pts > g.cap_pts || J.n_seg < 0 || J.n_seg > g.cap_seg) return fail(c, PLSVO_E_HIP, "candidates_align_fetch_job: corrupt job");
  O->n_pts = J.n_pts; O->n_seg = J.n_seg; O->skip = J.skip; O->long_mask = J.long_mask;
  for (int l = 0; l < PLSVO_MAX_LEVELS; ++l) O->n_slots[l] = J.n_slots[l];
  O->ref_slot = J.ref_slot; O->cur_slot = J.cur_slot; O->n_patches = *rb.at<int>(r_key); O->reserved0 = 0;
  memcpy(O->T0, rb.at<double>(r_T0), sizeof(O->T0)); memcpy(O->T_ref, rb.at<double>(r_Tr), sizeof(O->T_ref)); memcpy(O->T_f_w, rb.at<double>(r_Tc), sizeof(O->T_f_w));
  auto cp = [&](void* dst, int r, size_t count, size_t elem) { if (dst && count) memcpy(dst, rb.at<char>(r), count * elem); };
  const size_t kp = (size_t)J.n_pts, ks = (size_t)J.n_seg;
  cp(O->pt_px, r_ppx, 2 * kp, sizeof(double)); cp(O->pt_xyz_ref, r_pxyz, 3 * kp, sizeof(double));
  cp(O->seg_spx, r_spx, 2 * ks, sizeof(double)); cp(O->seg_epx, r_epx, 2 * ks, sizeof(double)); cp(O->seg_len, r_len, ks, sizeof(double));
  cp(O->seg_p_ref, r_sp, 3 * ks, sizeof(double)); cp(O->seg_q_ref, r_sq, 3 * ks, sizeof(double)); cp(O->seg_alive_in, r_al, ks, 1);
  if (O->seg_code) for (size_t l = 0; l < nl; ++l) cp(O->seg_code + l * ns, r_code[l], ks, sizeof(int));
  return PLSVO_OK;
}

// ---- the tracking gates behind the pose optimisation (alignjob_device.hpp map_track_gate_kernel) ------------------------------
namespace {
// the sections of tg_d_out: the records, the carried poses, num_obs_last_pt / _ls
struct GateSections { size_t out, carried, last, end; };
static GateSections gate_sections(size_t n) {
  Carver w; GateSections o;
  o.out = w.take<TrackGateOutDev>(n); o.carried = w.take<double>(n * 7); o.last = w.take<int>(n * 2); o.end = w.off;
  return o;
}
}  // namespace

extern "C" int plsvo_candidates_track_gate(plsvo_ctx* c, int n, const plsvo_cand_gate* in) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->cd_ran || !c->cs_selected || !c->cs_posed) return fail(c, PLSVO_E_STATE, "candidates_track_gate: no resident pose optimisation on the last run");
  if (const int rc = cand_seeds_pending(c, "candidates_track_gate")) return rc;
  if (n != c->cd_n || (n > 0 && !in)) return fail(c, PLSVO_E_INVALID, "candidates_track_gate: n does not match the staged batch");
  const bool have = c->tg_have && c->tg_n == n;   // (tg_have is cleared by every stage and n is the staged count: `have` means a gate since THIS stage)
  bool resident = false;
  for (int s = 0; s < n; ++s) {
    const plsvo_cand_gate& I = in[s];
    if (!I.active) continue;
    if (I.mode != PLSVO_GATE_TRACK && I.mode != PLSVO_GATE_RELOC) return fail(c, PLSVO_E_INVALID, "candidates_track_gate: unknown mode");
    if (I.last_source != PLSVO_GATE_LAST_HOST && I.last_source != PLSVO_GATE_LAST_RESIDENT) return fail(c, PLSVO_E_INVALID, "candidates_track_gate: unknown source of num_obs_last");
    if ((I.reset_source != PLSVO_INSERT_POSE_HOST && I.reset_source != PLSVO_INSERT_POSE_DEV) || (I.reset_source == PLSVO_INSERT_POSE_DEV && !I.d_T_reset))
      return fail(c, PLSVO_E_INVALID, "candidates_track_gate: bad pose source");
    if (I.quality_min_fts < 0 || I.quality_max_drop_fts < 0 || I.max_fts < 0 || I.max_fts_segs < 0 ||
        (I.last_source == PLSVO_GATE_LAST_HOST && (I.num_obs_last_pt < 0 || I.num_obs_last_ls < 0)))
      return fail(c, PLSVO_E_INVALID, "candidates_track_gate: negative threshold, clamp or count");
    resident = resident || I.last_source == PLSVO_GATE_LAST_RESIDENT;
  }
  if (resident && !have) return fail(c, PLSVO_E_STATE, "candidates_track_gate: no resident num_obs_last (no gate since the stage)");
  if (n == 0) { c->tg_have = true; c->tg_n = 0; return PLSVO_OK; }
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t N = (size_t)n;
  Blob blob;
  const size_t b_jobs = blob.reserve<TrackGateJobDev>(N);
  for (int s = 0; s < n; ++s) {
    const plsvo_cand_gate& I = in[s];
    TrackGateJobDev& J = blob.at<TrackGateJobDev>(b_jobs)[s];
    memset(&J, 0, sizeof(J));
    J.active = I.active ? 1 : 0;
    if (!J.active) continue;
    memcpy(J.T_reset, I.T_reset, sizeof(J.T_reset)); J.d_T_reset = I.reset_source == PLSVO_INSERT_POSE_DEV ? I.d_T_reset : nullptr;
    J.mode = I.mode; J.quality_min_fts = I.quality_min_fts; J.quality_max_drop_fts = I.quality_max_drop_fts; J.max_fts = I.max_fts; J.max_fts_segs = I.max_fts_segs;
    J.last_resident = I.last_source == PLSVO_GATE_LAST_RESIDENT ? 1 : 0; J.num_obs_last_pt = I.num_obs_last_pt; J.num_obs_last_ls = I.num_obs_last_ls;
  }
  int rc;
  if ((rc = upload_blob(c, c->tg_d_in, blob))) return rc;
  const GateSections o = gate_sections(N);
  if (!have) {                                      // the first gate behind a stage: a stream that sits it out reads as zeros
    c->tg_have = false;
    HIP_TRY(c, c->tg_d_out.ensure(o.end + 256));
    HIP_TRY(c, hipMemsetAsync(c->tg_d_out.p, 0, o.end, c->stream));
  }
  TrackGateBatchDev b{};
  b.jobs = Blob::dev<TrackGateJobDev>(c->tg_d_in, b_jobs); b.out = Carver::dev<TrackGateOutDev>(c->tg_d_out, o.out);
  b.scalars = c->cs_b.scalars; b.state = c->cs_w.state.as<PoseStateDev>(); b.poses = c->cs_w.poses.as<double>();
  b.carried = Carver::dev<double>(c->tg_d_out, o.carried); b.obs_last = Carver::dev<int>(c->tg_d_out, o.last); b.n_jobs = n;
  HIP_TRY_TIMED(c, PLSVO_K_KEYFRAME, launch_map_track_gate(b, c->stream));
  c->tg_b = b; c->tg_have = true; c->tg_n = n;
  return PLSVO_OK;
}

extern "C" int plsvo_candidates_gate_fetch(plsvo_ctx* c, int n, plsvo_cand_gate_out* out, double* poses) {
  CTX_CHECK(c);
  if (!c->cd_staged || !c->tg_have || c->tg_n != c->cd_n) return fail(c, PLSVO_E_STATE, "candidates_gate_fetch: no gate since the stage");
  if (n != c->cd_n || (n > 0 && !out)) return fail(c, PLSVO_E_INVALID, "candidates_gate_fetch: n does not match the staged batch");
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  static_assert(sizeof(TrackGateOutDev) == sizeof(plsvo_cand_gate_out) && sizeof(plsvo_cand_gate_out) == 32, "the device's record is the public one");
  Readback rb;
  const int r_out = rb.add(c->tg_b.out, (size_t)n * sizeof(TrackGateOutDev));
  const int r_T = poses ? rb.add(c->tg_b.carried, (size_t)n * 7 * sizeof(double)) : -1;
  if (const int rc = rb.wait(c)) return rc;
  memcpy(out, rb.at<TrackGateOutDev>(r_out), (size_t)n * sizeof(TrackGateOutDev));
  if (poses) memcpy(poses, rb.at<double>(r_T), (size_t)n * 7 * sizeof(double));
  return PLSVO_OK;
}

extern "C" const double* plsvo_candidates_gate_poses_dev(plsvo_ctx* c) { return (c && c->cd_staged && c->tg_have && c->tg_n == c->cd_n && c->tg_n > 0) ? c->tg_b.carried : nullptr; }

// ---- depth-filter seed lists resident beside the map tables (seedlist_device.hpp) -------------------------------------------
namespace {
// the sections of sd_d_work: reports, then the shadow rows (SeedsBatchDev's outputs, one per capacity row)
struct SeedWorkSections { size_t report, p_st, p_a, p_b, p_mu, p_s2, p_xyz, p_px, p_z, s_st, s_a, s_b, s_mus, s_mue, s_s2s, s_s2e, s_xs, s_xe, s_zs, s_ze, end; };
static SeedWorkSections seed_work_sections(size_t n, size_t tp, size_t ts) {
  Carver w; SeedWorkSections o;
  o.report = w.take<SeedReportDev>(n);
  o.p_st = w.take<int>(tp); o.p_a = w.take<float>(tp); o.p_b = w.take<float>(tp); o.p_mu = w.take<float>(tp); o.p_s2 = w.take<float>(tp);
  o.p_xyz = w.take<double>(tp * 3); o.p_px = w.take<double>(tp * 2); o.p_z = w.take<double>(tp);
  o.s_st = w.take<int>(ts); o.s_a = w.take<float>(ts); o.s_b = w.take<float>(ts); o.s_mus = w.take<float>(ts); o.s_mue = w.take<float>(ts);
  o.s_s2s = w.take<float>(ts); o.s_s2e = w.take<float>(ts); o.s_xs = w.take<double>(ts * 3); o.s_xe = w.take<double>(ts * 3); o.s_zs = w.take<double>(ts); o.s_ze = w.take<double>(ts);
  o.end = w.off;
  return o;
}
static int seeds_ready(plsvo_ctx* c, int n, const void* arg, const char* who, bool may_be_pending = false) {
  if (!c->cd_staged || !c->sd_staged) return fail(c, PLSVO_E_STATE, std::string(who) + ": no staged seed tables (a plsvo_candidates_stage drops them: stage both again)");
  if (!may_be_pending && c->sd_pending) return fail(c, PLSVO_E_STATE, std::string(who) + ": a seed update is not fetched yet (plsvo_seeds_update_fetch)");
  if (n != c->sd_n || (n > 0 && !arg)) return fail(c, PLSVO_E_INVALID, std::string(who) + ": n does not match the staged batch");
  return PLSVO_OK;
}
static size_t seed_round(size_t rows) { return (rows + 63) & ~(size_t)63; }   // match_device.hpp's MT: a workgroup of the update serves one stream
// the update's frames travel, then the commit launch; `launch_update`: the per-seed launch in front of it
static int seeds_enqueue(plsvo_ctx* c, int n, const std::vector<SeedFrameDev>& frames, bool launch_update) {
  Blob blob;
  blob.add(frames);
  if (const int rc = upload_blob(c, c->sd_d_in, blob)) return rc;
  SeedListBatchDev b = c->sd_b;
  b.frames = c->sd_d_in.as<SeedFrameDev>();
  b.s.pyr_base = c->pyr.base; b.s.slot_bytes = c->pyr.slot_bytes; b.s.width = c->pyr.w[0]; b.s.height = c->pyr.h[0];
  if (launch_update) HIP_TRY_TIMED(c, PLSVO_K_SEEDS, launch_update_seeds_resident(b, c->stream));
  HIP_TRY_TIMED(c, PLSVO_K_NEWCAND, launch_seeds_commit(b, c->stream));
  c->cd_max_level = std::max(c->cd_max_level, c->sd_max_level);   // a new landmark's observation has its seed's level
  c->cn_closed = true; c->cc_have_out = false;      // the open run is over, as behind plsvo_candidates_add
  c->sd_pending = true; c->sd_have_report = false;
  (void)n;
  return PLSVO_OK;
}
}  // namespace

extern "C" int plsvo_seeds_reserve(plsvo_ctx* c, const plsvo_seed_reserve* r) {
  CTX_CHECK(c);
  if (r && (r->extra_pt < 0 || r->extra_seg < 0)) return fail(c, PLSVO_E_INVALID, "seeds_reserve: negative room");
  c->sd_reserve = r ? *r : plsvo_seed_reserve{};
  return PLSVO_OK;
}

extern "C" int plsvo_seeds_capacity(plsvo_ctx* c, int n, plsvo_seed_reserve* out) {
  CTX_CHECK(c);
  if (const int rc = seeds_ready(c, n, out, "seeds_capacity", true)) return rc;
  for (int s = 0; s < n; ++s) { out[s].extra_pt = c->sd_lim[2 * (size_t)s]; out[s].extra_seg = c->sd_lim[2 * (size_t)s + 1]; }
  return PLSVO_OK;
}

extern "C" int plsvo_seeds_stage(plsvo_ctx* c, int n, const plsvo_seed_params* pr, const plsvo_seed_list* lists) {
  CTX_CHECK(c);
  if (!c->cd_staged || n != c->cd_n) return fail(c, PLSVO_E_STATE, "seeds_stage: no staged candidate tables of the same n");
  if (c->sd_pending) return fail(c, PLSVO_E_STATE, "seeds_stage: a seed update is not fetched yet (plsvo_seeds_update_fetch)");
  if (!c->pyr.base) return fail(c, PLSVO_E_STATE, "seeds_stage: pyramids not configured");
  if (!pr || (n > 0 && !lists)) return fail(c, PLSVO_E_INVALID, "seeds_stage: bad arguments");
  if (pr->n_pyr_levels < 1 || pr->align_max_iter < 0 || pr->max_epi_search_steps < 0 || pr->max_n_kfs < 0 || pr->n_pyr_levels > c->pyr.n_levels)
    return fail(c, PLSVO_E_INVALID, "seeds_stage: bad parameters");
  if (pr->cam.width != c->pyr.w[0] || pr->cam.height != c->pyr.h[0]) return fail(c, PLSVO_E_INVALID, "seeds_stage: camera size does not match the configured pyramid");
  const plsvo_seed_reserve R = c->sd_reserve;
  const size_t N = (size_t)n;
  std::vector<SeedStreamDev> sd(N);
  std::vector<int> lim(2 * N), blk_pt, blk_seg;
  size_t tp = 0, ts = 0;
  int max_level = 0;
  for (int s = 0; s < n; ++s) {
    const plsvo_seed_list& I = lists[s]; const CandMapDev& M = c->cd_maps[(size_t)s]; const CandStreamHost& H = c->cd_host[(size_t)s];
    if (I.n_pt < 0 || I.n_seg < 0) return fail(c, PLSVO_E_INVALID, "seeds_stage: negative count");
    if (I.n_pt > 0 && (!I.pt_ref_kf || !I.pt_batch_id || !I.pt_px || !I.pt_f || !I.pt_level || !I.pt_type || !I.pt_a || !I.pt_b || !I.pt_mu || !I.pt_z_range || !I.pt_sigma2))
      return fail(c, PLSVO_E_INVALID, "seeds_stage: null point-seed array");
    if (I.n_seg > 0 && (!I.seg_ref_kf || !I.seg_batch_id || !I.seg_px || !I.seg_f || !I.seg_sf || !I.seg_ef || !I.seg_spx || !I.seg_epx || !I.seg_level || !I.seg_a || !I.seg_b ||
                        !I.seg_mu_s || !I.seg_mu_e || !I.seg_z_range_s || !I.seg_z_range_e || !I.seg_sigma2_s || !I.seg_sigma2_e))
      return fail(c, PLSVO_E_INVALID, "seeds_stage: null line-seed array");
    if (!cand_idx_ok(I.pt_ref_kf, (size_t)I.n_pt, 0, M.n_kf) || !cand_idx_ok(I.seg_ref_kf, (size_t)I.n_seg, 0, M.n_kf)) return fail(c, PLSVO_E_INVALID, "seeds_stage: ref_kf outside the keyframe table");
    if (!cand_idx_ok(I.pt_level, (size_t)I.n_pt, 0, c->pyr.n_levels) || !cand_idx_ok(I.seg_level, (size_t)I.n_seg, 0, c->pyr.n_levels))
      return fail(c, PLSVO_E_INVALID, "seeds_stage: feature level outside the configured pyramid");
    for (int k = 0; k < I.n_pt; ++k) {
      if (I.pt_type[k] == PLSVO_FTR_EDGELET) { if (pr->edgelet_filtering && !I.pt_grad) return fail(c, PLSVO_E_INVALID, "seeds_stage: edgelets without pt_grad"); }
      else if (I.pt_type[k] != PLSVO_FTR_CORNER) return fail(c, PLSVO_E_INVALID, "seeds_stage: unknown feature type");
      max_level = std::max(max_level, (int)I.pt_level[k]);
    }
    for (int k = 0; k < I.n_seg; ++k) max_level = std::max(max_level, (int)I.seg_level[k]);
    if ((size_t)I.n_pt + (size_t)R.extra_pt > (size_t)INT32_MAX - 64 || (size_t)I.n_seg + (size_t)R.extra_seg > (size_t)INT32_MAX - 64) return fail(c, PLSVO_E_CAPACITY, "seeds_stage: stream too large");
    SeedStreamDev& S = sd[(size_t)s];
    S = SeedStreamDev{};
    S.n_pt = I.n_pt; S.n_seg = I.n_seg; S.batch_counter = I.batch_counter;
    lim[2 * (size_t)s] = I.n_pt + R.extra_pt; lim[2 * (size_t)s + 1] = I.n_seg + R.extra_seg;
    S.cap_pt = (int)seed_round((size_t)lim[2 * (size_t)s]); S.cap_seg = (int)seed_round((size_t)lim[2 * (size_t)s + 1]);
    S.rows_pt = H.rows_pt; S.rows_seg = H.rows_seg; S.rows_pt_cand = H.rows_pt_cand; S.rows_seg_cand = H.rows_seg_cand; S.cap_pt_obs = H.cap_pt_obs; S.cap_seg_obs = H.cap_seg_obs;
    S.pt_off = (long long)tp; S.seg_off = (long long)ts;
    for (int k = 0; k < S.cap_pt / 64; ++k) blk_pt.push_back(s);
    for (int k = 0; k < S.cap_seg / 64; ++k) blk_seg.push_back(s);
    tp += (size_t)S.cap_pt; ts += (size_t)S.cap_seg;
  }
  if (tp / 64 + ts / 64 > (size_t)INT32_MAX) return fail(c, PLSVO_E_CAPACITY, "seeds_stage: batch too large");
  c->sd_staged = false; c->sd_have_report = false; c->sk_have_report = false;
  c->sd_params = *pr; c->sd_n = n; c->sd_host = sd; c->sd_lim = lim; c->sd_max_level = max_level; c->sd_t_pt = tp; c->sd_t_seg = ts;
  if (n == 0) { c->sd_staged = true; c->sd_b = SeedListBatchDev{}; return PLSVO_OK; }
  HIP_TRY(c, hipSetDevice(c->device));
  const int n_blk_pt = (int)blk_pt.size();
  blk_pt.insert(blk_pt.end(), blk_seg.begin(), blk_seg.end());
  Blob blob;
  const size_t b_str = blob.add(sd), b_blk = blob.add(blk_pt);
  const size_t p_kf = blob.reserve<int>(tp), p_bid = blob.reserve<int>(tp), p_px = blob.reserve<double>(tp * 2), p_f = blob.reserve<double>(tp * 3), p_lv = blob.reserve<int>(tp),
               p_ty = blob.reserve<uint8_t>(tp), p_gr = blob.reserve<double>(tp * 2), p_a = blob.reserve<float>(tp), p_b = blob.reserve<float>(tp), p_mu = blob.reserve<float>(tp),
               p_zr = blob.reserve<float>(tp), p_s2 = blob.reserve<float>(tp);
  const size_t s_kf = blob.reserve<int>(ts), s_bid = blob.reserve<int>(ts), s_px = blob.reserve<double>(ts * 2), s_f = blob.reserve<double>(ts * 3), s_sf = blob.reserve<double>(ts * 3),
               s_ef = blob.reserve<double>(ts * 3), s_spx = blob.reserve<double>(ts * 2), s_epx = blob.reserve<double>(ts * 2), s_lv = blob.reserve<int>(ts), s_a = blob.reserve<float>(ts),
               s_b = blob.reserve<float>(ts), s_mus = blob.reserve<float>(ts), s_mue = blob.reserve<float>(ts), s_zrs = blob.reserve<float>(ts), s_zre = blob.reserve<float>(ts),
               s_s2s = blob.reserve<float>(ts), s_s2e = blob.reserve<float>(ts);
  auto put = [&](size_t sec, size_t at, const void* src, size_t count, size_t elem) { if (count && src) memcpy(blob.host.data() + sec + at * elem, src, count * elem); };
  for (int s = 0; s < n; ++s) {
    const plsvo_seed_list& I = lists[s]; const SeedStreamDev& S = sd[(size_t)s];
    const size_t np = (size_t)I.n_pt, ns = (size_t)I.n_seg, po = (size_t)S.pt_off, so = (size_t)S.seg_off;
    put(p_kf, po, I.pt_ref_kf, np, 4); put(p_bid, po, I.pt_batch_id, np, 4); put(p_px, po * 2, I.pt_px, np * 2, 8); put(p_f, po * 3, I.pt_f, np * 3, 8); put(p_lv, po, I.pt_level, np, 4);
    put(p_ty, po, I.pt_type, np, 1); put(p_gr, po * 2, I.pt_grad, np * 2, 8); put(p_a, po, I.pt_a, np, 4); put(p_b, po, I.pt_b, np, 4); put(p_mu, po, I.pt_mu, np, 4);
    put(p_zr, po, I.pt_z_range, np, 4); put(p_s2, po, I.pt_sigma2, np, 4);
    put(s_kf, so, I.seg_ref_kf, ns, 4); put(s_bid, so, I.seg_batch_id, ns, 4); put(s_px, so * 2, I.seg_px, ns * 2, 8); put(s_f, so * 3, I.seg_f, ns * 3, 8); put(s_sf, so * 3, I.seg_sf, ns * 3, 8);
    put(s_ef, so * 3, I.seg_ef, ns * 3, 8); put(s_spx, so * 2, I.seg_spx, ns * 2, 8); put(s_epx, so * 2, I.seg_epx, ns * 2, 8); put(s_lv, so, I.seg_level, ns, 4);
    put(s_a, so, I.seg_a, ns, 4); put(s_b, so, I.seg_b, ns, 4); put(s_mus, so, I.seg_mu_s, ns, 4); put(s_mue, so, I.seg_mu_e, ns, 4); put(s_zrs, so, I.seg_z_range_s, ns, 4);
    put(s_zre, so, I.seg_z_range_e, ns, 4); put(s_s2s, so, I.seg_sigma2_s, ns, 4); put(s_s2e, so, I.seg_sigma2_e, ns, 4);
  }
  if (const int rc = upload_blob(c, c->sd_d_tab, blob)) return rc;
  c->sd_tab_bytes = blob.host.size();
  const SeedWorkSections W = seed_work_sections(N, tp, ts);
  HIP_TRY(c, c->sd_d_work.ensure(W.end + 256));
  HIP_TRY(c, hipMemsetAsync(c->sd_d_work.p, 0, W.end, c->stream));
  HIP_TRY(c, c->sk_d_report.ensure(N * sizeof(SeedStartReportDev)));   // plsvo_seeds_keyframe_detect's reports: all zero until an event touches the stream
  HIP_TRY(c, hipMemsetAsync(c->sk_d_report.p, 0, N * sizeof(SeedStartReportDev), c->stream));
  char* d = reinterpret_cast<char*>(c->sd_d_tab.p); char* w = reinterpret_cast<char*>(c->sd_d_work.p);
  auto D = [&](size_t o) { return reinterpret_cast<double*>(d + o); };
  auto Iv = [&](size_t o) { return reinterpret_cast<int*>(d + o); };
  auto Fv = [&](size_t o) { return reinterpret_cast<float*>(d + o); };
  auto WD = [&](size_t o) { return reinterpret_cast<double*>(w + o); };
  auto WI = [&](size_t o) { return reinterpret_cast<int*>(w + o); };
  auto WF = [&](size_t o) { return reinterpret_cast<float*>(w + o); };
  SeedListBatchDev b{};
  SeedsBatchDev& q = b.s;
  q.fx = pr->cam.fx; q.fy = pr->cam.fy; q.cx = pr->cam.cx; q.cy = pr->cam.cy; q.cam_width = pr->cam.width; q.cam_height = pr->cam.height;
  q.n_pyr_levels = pr->n_pyr_levels; q.align_max_iter = pr->align_max_iter; q.max_epi_search_steps = pr->max_epi_search_steps;
  q.edgelet_filtering = pr->edgelet_filtering; q.edgelet_max_angle = pr->edgelet_max_angle;
  q.px_error_angle = std::atan(pr->px_noise / (2.0 * std::fabs(pr->cam.fx))) * 2.0;   // depth_filter.cpp:279-280 (host libm, as in plsvo_update_seeds)
  q.convergence_sigma2_thresh = pr->convergence_sigma2_thresh;
  q.n_pt = (int)std::min(tp, (size_t)INT32_MAX); q.n_seg = (int)std::min(ts, (size_t)INT32_MAX);
  q.frame_T = c->cd_b.frame_T; q.frame_slot = c->cd_b.frame_slot;
  q.pt_ref_frame = Iv(p_kf); q.pt_px = D(p_px); q.pt_f = D(p_f); q.pt_level = Iv(p_lv); q.pt_type = reinterpret_cast<const uint8_t*>(d + p_ty); q.pt_grad = D(p_gr);
  q.pt_a = Fv(p_a); q.pt_b = Fv(p_b); q.pt_mu = Fv(p_mu); q.pt_z_range = Fv(p_zr); q.pt_sigma2 = Fv(p_s2);
  q.seg_ref_frame = Iv(s_kf); q.seg_px = D(s_px); q.seg_f = D(s_f); q.seg_sf = D(s_sf); q.seg_ef = D(s_ef); q.seg_level = Iv(s_lv);
  q.seg_a = Fv(s_a); q.seg_b = Fv(s_b); q.seg_mu_s = Fv(s_mus); q.seg_mu_e = Fv(s_mue); q.seg_z_range_s = Fv(s_zrs); q.seg_z_range_e = Fv(s_zre);
  q.seg_sigma2_s = Fv(s_s2s); q.seg_sigma2_e = Fv(s_s2e);
  q.o_pt_status = WI(W.p_st); q.o_pt_a = WF(W.p_a); q.o_pt_b = WF(W.p_b); q.o_pt_mu = WF(W.p_mu); q.o_pt_sigma2 = WF(W.p_s2); q.o_pt_xyz = WD(W.p_xyz); q.o_pt_px = WD(W.p_px);
  q.o_pt_depth = WD(W.p_z);
  q.o_seg_status = WI(W.s_st); q.o_seg_a = WF(W.s_a); q.o_seg_b = WF(W.s_b); q.o_seg_mu_s = WF(W.s_mus); q.o_seg_mu_e = WF(W.s_mue); q.o_seg_sigma2_s = WF(W.s_s2s);
  q.o_seg_sigma2_e = WF(W.s_s2e); q.o_seg_xyz_s = WD(W.s_xs); q.o_seg_xyz_e = WD(W.s_xe); q.o_seg_depth_s = WD(W.s_zs); q.o_seg_depth_e = WD(W.s_ze);
  const QualitySections ql = quality_sections(c);
  char* dq = reinterpret_cast<char*>(c->cs_d_q.p);
  b.m.c = c->cd_b;
  b.m.pt_nfail = reinterpret_cast<int*>(dq + ql.pt_nf); b.m.pt_nsucc = reinterpret_cast<int*>(dq + ql.pt_ns); b.m.seg_nfail = reinterpret_cast<int*>(dq + ql.seg_nf);
  b.m.seg_nsucc = reinterpret_cast<int*>(dq + ql.seg_ns); b.m.pt_event = reinterpret_cast<uint8_t*>(dq + ql.pt_ev); b.m.seg_event = reinterpret_cast<uint8_t*>(dq + ql.seg_ev);
  b.streams = reinterpret_cast<SeedStreamDev*>(d + b_str); b.report = reinterpret_cast<SeedReportDev*>(w + W.report); b.blk_stream = Iv(b_blk);
  b.n_blk_pt = n_blk_pt; b.n_blk = (int)blk_pt.size(); b.n_jobs = n; b.max_n_kfs = pr->max_n_kfs;
  b.pt_batch_id = Iv(p_bid); b.seg_batch_id = Iv(s_bid); b.seg_spx = D(s_spx); b.seg_epx = D(s_epx);
  c->sd_b = b;
  c->sd_staged = true;
  return PLSVO_OK;
}

extern "C" int plsvo_seeds_update(plsvo_ctx* c, int n, const plsvo_seed_frame* fr) {
  CTX_CHECK(c);
  if (const int rc = seeds_ready(c, n, fr, "seeds_update")) return rc;
  if (!c->pyr.base || c->pyr.n_levels < c->sd_params.n_pyr_levels || c->sd_max_level >= c->pyr.n_levels || c->sd_params.cam.width != c->pyr.w[0] || c->sd_params.cam.height != c->pyr.h[0])
    return fail(c, PLSVO_E_STATE, "seeds_update: the configured pyramids are not those of the stage");
  for (int s = 0; s < n; ++s) {
    if (!fr[s].active) continue;
    if (fr[s].cur_slot < 0 || fr[s].cur_slot >= c->pyr.n_slots) return fail(c, PLSVO_E_INVALID, "seeds_update: pyramid slot out of range");
    if (fr[s].pose_source < PLSVO_INSERT_POSE_HOST || fr[s].pose_source > PLSVO_INSERT_POSE_RESIDENT || (fr[s].pose_source == PLSVO_INSERT_POSE_DEV && !fr[s].d_T_f_w))
      return fail(c, PLSVO_E_INVALID, "seeds_update: bad pose source");
    if (fr[s].pose_source == PLSVO_INSERT_POSE_RESIDENT && !c->cs_posed) return fail(c, PLSVO_E_STATE, "seeds_update: no resident pose optimisation for the pose");
  }
  for (int s = 0; s < n; ++s) {
    if (!fr[s].active || c->sd_host[(size_t)s].n_pt + c->sd_host[(size_t)s].n_seg == 0) continue;
    const CandMapDev& M = c->cd_maps[(size_t)s];
    for (int k = 0; k < M.n_kf; ++k) if (c->cd_kf_slot[(size_t)M.kf_off + (size_t)k] >= c->pyr.n_slots) return fail(c, PLSVO_E_CAPACITY, "seeds_update: a keyframe's pyramid slot is out of range");
  }
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  std::vector<SeedFrameDev> frames((size_t)n);
  for (int s = 0; s < n; ++s) {
    SeedFrameDev& J = frames[(size_t)s];
    memset(&J, 0, sizeof(J));
    J.active = fr[s].active ? 1 : 0; J.cur_slot = fr[s].cur_slot;
    if (!J.active) continue;
    memcpy(J.T, fr[s].T_f_w, sizeof(J.T));
    J.d_T = fr[s].pose_source == PLSVO_INSERT_POSE_DEV ? fr[s].d_T_f_w : fr[s].pose_source == PLSVO_INSERT_POSE_RESIDENT ? c->cs_w.poses.as<double>() + 7 * (size_t)s : nullptr;
  }
  return seeds_enqueue(c, n, frames, true);
}

extern "C" int plsvo_seeds_commit_rows(plsvo_ctx* c, int n, const plsvo_seed_rows* rows) {
  CTX_CHECK(c);
  if (const int rc = seeds_ready(c, n, rows, "seeds_commit_rows")) return rc;
  for (int s = 0; s < n; ++s) {
    const plsvo_seed_rows& I = rows[s]; const SeedStreamDev& S = c->sd_host[(size_t)s];
    if (!I.active) continue;
    if (I.n_pt != S.n_pt || I.n_seg != S.n_seg) return fail(c, PLSVO_E_INVALID, "seeds_commit_rows: the row counts are not the list lengths");
    if (I.n_pt > 0 && (!I.pt_status || !I.pt_a || !I.pt_b || !I.pt_mu || !I.pt_sigma2 || !I.pt_xyz_world)) return fail(c, PLSVO_E_INVALID, "seeds_commit_rows: null point array");
    if (I.n_seg > 0 && (!I.seg_status || !I.seg_a || !I.seg_b || !I.seg_mu_s || !I.seg_mu_e || !I.seg_sigma2_s || !I.seg_sigma2_e || !I.seg_xyz_world_s || !I.seg_xyz_world_e))
      return fail(c, PLSVO_E_INVALID, "seeds_commit_rows: null segment array");
    if (!cand_idx_ok(I.pt_status, (size_t)I.n_pt, 0, PLSVO_SEED_AGED + 1) || !cand_idx_ok(I.seg_status, (size_t)I.n_seg, 0, PLSVO_SEED_AGED + 1)) return fail(c, PLSVO_E_INVALID, "seeds_commit_rows: unknown status");
  }
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const SeedsBatchDev& q = c->sd_b.s;
  std::vector<SeedFrameDev> frames((size_t)n);
  auto up = [&](void* dst, const void* src, size_t bytes) { return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream) : hipSuccess; };
  for (int s = 0; s < n; ++s) {
    const plsvo_seed_rows& I = rows[s]; const SeedStreamDev& S = c->sd_host[(size_t)s];
    memset(&frames[(size_t)s], 0, sizeof(SeedFrameDev));
    frames[(size_t)s].active = I.active ? 1 : 0;
    if (!I.active) continue;
    const size_t np = (size_t)I.n_pt, ns = (size_t)I.n_seg, po = (size_t)S.pt_off, so = (size_t)S.seg_off;
    HIP_TRY(c, up(q.o_pt_status + po, I.pt_status, np * 4)); HIP_TRY(c, up(q.o_pt_a + po, I.pt_a, np * 4)); HIP_TRY(c, up(q.o_pt_b + po, I.pt_b, np * 4));
    HIP_TRY(c, up(q.o_pt_mu + po, I.pt_mu, np * 4)); HIP_TRY(c, up(q.o_pt_sigma2 + po, I.pt_sigma2, np * 4)); HIP_TRY(c, up(q.o_pt_xyz + 3 * po, I.pt_xyz_world, np * 24));
    HIP_TRY(c, up(q.o_seg_status + so, I.seg_status, ns * 4)); HIP_TRY(c, up(q.o_seg_a + so, I.seg_a, ns * 4)); HIP_TRY(c, up(q.o_seg_b + so, I.seg_b, ns * 4));
    HIP_TRY(c, up(q.o_seg_mu_s + so, I.seg_mu_s, ns * 4)); HIP_TRY(c, up(q.o_seg_mu_e + so, I.seg_mu_e, ns * 4)); HIP_TRY(c, up(q.o_seg_sigma2_s + so, I.seg_sigma2_s, ns * 4));
    HIP_TRY(c, up(q.o_seg_sigma2_e + so, I.seg_sigma2_e, ns * 4)); HIP_TRY(c, up(q.o_seg_xyz_s + 3 * so, I.seg_xyz_world_s, ns * 24)); HIP_TRY(c, up(q.o_seg_xyz_e + 3 * so, I.seg_xyz_world_e, ns * 24));
  }
  if (const int rc = seeds_enqueue(c, n, frames, false)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // the caller's arrays are free again
  return PLSVO_OK;
}

extern "C" int plsvo_seeds_update_fetch(plsvo_ctx* c, int n, plsvo_seed_report* out) {
  CTX_CHECK(c);
  if (const int rc = seeds_ready(c, n, out, "seeds_update_fetch", true)) return rc;
  if (!c->sd_pending && !c->sd_have_report) return fail(c, PLSVO_E_STATE, "seeds_update_fetch: no update since the seed tables were staged");
  static_assert(sizeof(SeedReportDev) == sizeof(plsvo_seed_report), "the device's report is the public one");
  if (c->sd_pending) {
    HIP_TRY(c, hipSetDevice(c->device));
    Readback rb;
    rb.add(c->sd_b.report, (size_t)n * sizeof(SeedReportDev));
    if (const int rc = rb.wait(c)) return rc;
    c->sd_last.assign(rb.at<SeedReportDev>(0), rb.at<SeedReportDev>(0) + n);
    for (int s = 0; s < n; ++s) {                   // the host mirrors describe the tables as they stand
      const SeedReportDev& R = c->sd_last[(size_t)s];
      CandMapDev& M = c->cd_maps[(size_t)s]; CandStreamHost& H = c->cd_host[(size_t)s]; SeedStreamDev& S = c->sd_host[(size_t)s];
      M.n_pt = R.n_pt; M.n_seg = R.n_seg; M.n_pt_cand = R.n_pt_cand; M.n_seg_cand = R.n_seg_cand; H.n_pt_obs = R.n_pt_obs; H.n_seg_obs = R.n_seg_obs;
      S.n_pt = R.n_pt_seeds; S.n_seg = R.n_seg_seeds; S.batch_counter = R.batch_counter;
    }
    c->sd_pending = false; c->sd_have_report = true;
  }
  if (n > 0) memcpy(out, c->sd_last.data(), (size_t)n * sizeof(plsvo_seed_report));
  return PLSVO_OK;
}

extern "C" int plsvo_seeds_keyframe(plsvo_ctx* c, int n, const plsvo_seed_kf* in) {
  CTX_CHECK(c);
  if (const int rc = seeds_ready(c, n, in, "seeds_keyframe")) return rc;
  size_t tp = 0, ts = 0;
  int max_level = c->sd_max_level;
  bool any = false;
  for (int s = 0; s < n; ++s) {
    const plsvo_seed_kf& I = in[s]; const CandMapDev& M = c->cd_maps[(size_t)s];
    if (I.n_pt < 0 || I.n_seg < 0) return fail(c, PLSVO_E_INVALID, "seeds_keyframe: negative count");
    if (I.removed_kf < -1 || I.removed_kf > M.n_kf) return fail(c, PLSVO_E_INVALID, "seeds_keyframe: removed_kf outside the keyframe table as it stood");
    if (I.n_pt + I.n_seg > 0) {
      if (I.new_kf < 0 || I.new_kf >= M.n_kf) return fail(c, PLSVO_E_INVALID, "seeds_keyframe: new_kf outside the keyframe table");
      if (!((float)I.depth_mean > 0.0f) || !((float)I.depth_min > 0.0f)) return fail(c, PLSVO_E_INVALID, "seeds_keyframe: depth not positive");
    }
    if (I.n_pt > 0 && (!I.pt_px || !I.pt_f || !I.pt_level || !I.pt_type)) return fail(c, PLSVO_E_INVALID, "seeds_keyframe: null point array");
    if (I.n_seg > 0 && (!I.seg_px || !I.seg_f || !I.seg_sf || !I.seg_ef || !I.seg_spx || !I.seg_epx || !I.seg_level)) return fail(c, PLSVO_E_INVALID, "seeds_keyframe: null segment array");
    if (!cand_idx_ok(I.pt_level, (size_t)I.n_pt, 0, c->pyr.n_levels) || !cand_idx_ok(I.seg_level, (size_t)I.n_seg, 0, c->pyr.n_levels))
      return fail(c, PLSVO_E_INVALID, "seeds_keyframe: feature level outside the configured pyramid");
    for (int k = 0; k < I.n_pt; ++k) {
      if (I.pt_type[k] == PLSVO_FTR_EDGELET) { if (c->sd_params.edgelet_filtering && !I.pt_grad) return fail(c, PLSVO_E_INVALID, "seeds_keyframe: edgelets without pt_grad"); }
      else if (I.pt_type[k] != PLSVO_FTR_CORNER) return fail(c, PLSVO_E_INVALID, "seeds_keyframe: unknown feature type");
      max_level = std::max(max_level, (int)I.pt_level[k]);
    }
    for (int k = 0; k < I.n_seg; ++k) max_level = std::max(max_level, (int)I.seg_level[k]);
    tp += (size_t)I.n_pt; ts += (size_t)I.n_seg;
    any = any || I.removed_kf >= 0 || I.new_batch || I.n_pt + I.n_seg > 0;
  }
  for (int s = 0; s < n; ++s)                       // room, from the mirrored list lengths
    if ((long long)c->sd_host[(size_t)s].n_pt + in[s].n_pt > c->sd_lim[2 * (size_t)s] || (long long)c->sd_host[(size_t)s].n_seg + in[s].n_seg > c->sd_lim[2 * (size_t)s + 1])
      return fail(c, PLSVO_E_CAPACITY, "seeds_keyframe: a stream's seed list lacks rows (plsvo_seeds_reserve); nothing was changed");
  if (!any) return PLSVO_OK;
  if (tp > (size_t)INT32_MAX || ts > (size_t)INT32_MAX) return fail(c, PLSVO_E_CAPACITY, "seeds_keyframe: batch too large");
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t N = (size_t)n;
  Blob blob;
  const size_t b_jobs = blob.reserve<SeedKfJobDev>(N);
  const size_t p_px = blob.reserve<double>(tp * 2), p_f = blob.reserve<double>(tp * 3), p_lv = blob.reserve<int>(tp), p_ty = blob.reserve<uint8_t>(tp), p_gr = blob.reserve<double>(tp * 2);
  const size_t s_px = blob.reserve<double>(ts * 2), s_f = blob.reserve<double>(ts * 3), s_sf = blob.reserve<double>(ts * 3), s_ef = blob.reserve<double>(ts * 3),
               s_spx = blob.reserve<double>(ts * 2), s_epx = blob.reserve<double>(ts * 2), s_lv = blob.reserve<int>(ts);
  auto put = [&](size_t sec, size_t at, const void* src, size_t count, size_t elem) { if (count && src) memcpy(blob.host.data() + sec + at * elem, src, count * elem); };
  size_t ap = 0, as = 0;
  for (int s = 0; s < n; ++s) {
    const plsvo_seed_kf& I = in[s];
    SeedKfJobDev& J = blob.at<SeedKfJobDev>(b_jobs)[s];
    memset(&J, 0, sizeof(J));
    J.removed_kf = I.removed_kf; J.new_batch = I.new_batch ? 1 : 0; J.new_kf = I.new_kf; J.n_pt = I.n_pt; J.n_seg = I.n_seg; J.pt_at = (long long)ap; J.seg_at = (long long)as;
    if (I.n_pt + I.n_seg > 0) {                     // PointSeed::PointSeed / LineSeed::LineSeed (:53-74): float arguments, float members
      const float depth_mean = (float)I.depth_mean, depth_min = (float)I.depth_min;
      const float mu = 1.0 / depth_mean, z_range = 1.0 / depth_min;
      const float sigma2 = z_range * z_range / 36;
      J.mu = mu; J.z_range = z_range; J.sigma2 = sigma2;
    }
    const size_t np = (size_t)I.n_pt, ns = (size_t)I.n_seg;
    put(p_px, ap * 2, I.pt_px, np * 2, 8); put(p_f, ap * 3, I.pt_f, np * 3, 8); put(p_lv, ap, I.pt_level, np, 4); put(p_ty, ap, I.pt_type, np, 1); put(p_gr, ap * 2, I.pt_grad, np * 2, 8);
    put(s_px, as * 2, I.seg_px, ns * 2, 8); put(s_f, as * 3, I.seg_f, ns * 3, 8); put(s_sf, as * 3, I.seg_sf, ns * 3, 8); put(s_ef, as * 3, I.seg_ef, ns * 3, 8);
    put(s_spx, as * 2, I.seg_spx, ns * 2, 8); put(s_epx, as * 2, I.seg_epx, ns * 2, 8); put(s_lv, as, I.seg_level, ns, 4);
    ap += np; as += ns;
  }
  if (const int rc = upload_blob(c, c->sd_d_in, blob)) return rc;
  const char* d = reinterpret_cast<const char*>(c->sd_d_in.p);
  auto D = [&](size_t o) { return reinterpret_cast<const double*>(d + o); };
  SeedListBatchDev b = c->sd_b;
  b.kf_jobs = reinterpret_cast<const SeedKfJobDev*>(d + b_jobs);
  b.k_pt_px = D(p_px); b.k_pt_f = D(p_f); b.k_pt_level = reinterpret_cast<const int*>(d + p_lv); b.k_pt_type = reinterpret_cast<const uint8_t*>(d + p_ty); b.k_pt_grad = D(p_gr);
  b.k_seg_px = D(s_px); b.k_seg_f = D(s_f); b.k_seg_sf = D(s_sf); b.k_seg_ef = D(s_ef); b.k_seg_spx = D(s_spx); b.k_seg_epx = D(s_epx); b.k_seg_level = reinterpret_cast<const int*>(d + s_lv);
  HIP_TRY_TIMED(c, PLSVO_K_NEWCAND, launch_seeds_keyframe(b, c->stream));
  for (int s = 0; s < n; ++s) {                     // (with a removal the lengths are upper bounds until the next update fetch)
    SeedStreamDev& S = c->sd_host[(size_t)s];
    S.n_pt += in[s].n_pt; S.n_seg += in[s].n_seg; S.batch_counter += in[s].new_batch ? 1 : 0;
  }
  c->sd_max_level = max_level;
  return PLSVO_OK;
}

// DepthFilter::initializeSeeds' creating half (:151-191) on the device: occupancy grids, detection through a slot table, seed start
extern "C" int plsvo_seeds_keyframe_detect(plsvo_ctx* c, int n, const plsvo_detect_params* p, const plsvo_seed_kf_detect* in) {
  CTX_CHECK(c);
  if (const int rc = seeds_ready(c, n, in, "seeds_keyframe_detect")) return rc;
  if (!c->pyr.base || c->pyr.n_levels < c->sd_params.n_pyr_levels || c->sd_params.cam.width != c->pyr.w[0] || c->sd_params.cam.height != c->pyr.h[0])
    return fail(c, PLSVO_E_STATE, "seeds_keyframe_detect: the configured pyramids are not those of the stage");
  if (!p) return fail(c, PLSVO_E_INVALID, "seeds_keyframe_detect: NULL params");
  int n_act = 0;
  for (int s = 0; s < n; ++s) n_act += in[s].active ? 1 : 0;
  int cols = 0, rows = 0;
  if (const int rc = detect_check_params(c, n_act, p, "seeds_keyframe_detect", &cols, &rows)) return rc;
  const int cells = cols * rows;
  size_t ts = 0;
  int sources = 0, max_level = std::max(c->sd_max_level, p->n_levels - 1);
  for (int s = 0; s < n; ++s) {
    const plsvo_seed_kf_detect& I = in[s]; const CandMapDev& M = c->cd_maps[(size_t)s];
    if (!I.active) continue;
    if (I.removed_kf < -1 || I.removed_kf > M.n_kf) return fail(c, PLSVO_E_INVALID, "seeds_keyframe_detect: removed_kf outside the keyframe table as it stood");
    if (I.new_kf < 0 || I.new_kf >= M.n_kf) return fail(c, PLSVO_E_INVALID, "seeds_keyframe_detect: new_kf outside the keyframe table");
    const int slot = c->cd_kf_slot[(size_t)M.kf_off + (size_t)I.new_kf];
    if (slot < 0 || slot >= c->pyr.n_slots) return fail(c, PLSVO_E_INVALID, "seeds_keyframe_detect: the keyframe's pyramid slot is out of range");
    if (I.occ_sources & ~(PLSVO_SEED_OCC_SELECTED | PLSVO_SEED_OCC_UPDATED)) return fail(c, PLSVO_E_INVALID, "seeds_keyframe_detect: unknown occupancy source");
    if (!((float)I.depth_mean > 0.0f) || !((float)I.depth_min > 0.0f)) return fail(c, PLSVO_E_INVALID, "seeds_keyframe_detect: depth not positive");
    if (I.n_seg < 0) return fail(c, PLSVO_E_INVALID, "seeds_keyframe_detect: negative count");
    if (I.n_seg > 0 && (!I.seg_px || !I.seg_f || !I.seg_sf || !I.seg_ef || !I.seg_spx || !I.seg_epx || !I.seg_level)) return fail(c, PLSVO_E_INVALID, "seeds_keyframe_detect: null segment array");
    if (!cand_idx_ok(I.seg_level, (size_t)I.n_seg, 0, c->pyr.n_levels)) return fail(c, PLSVO_E_INVALID, "seeds_keyframe_detect: feature level outside the configured pyramid");
    for (int k = 0; k < I.n_seg; ++k) max_level = std::max(max_level, (int)I.seg_level[k]);
    ts += (size_t)I.n_seg; sources |= I.occ_sources;
  }
  if ((sources & PLSVO_SEED_OCC_SELECTED) && !c->cs_selected) return fail(c, PLSVO_E_STATE, "seeds_keyframe_detect: PLSVO_SEED_OCC_SELECTED without a selection (plsvo_candidates_select)");
  if ((sources & PLSVO_SEED_OCC_UPDATED) && !c->sd_have_report) return fail(c, PLSVO_E_STATE, "seeds_keyframe_detect: PLSVO_SEED_OCC_UPDATED without a fetched update (plsvo_seeds_update_fetch)");
  for (int s = 0; s < n; ++s)                       // the segments' room, from the mirrored list lengths
    if (in[s].active && (long long)c->sd_host[(size_t)s].n_seg + in[s].n_seg > c->sd_lim[2 * (size_t)s + 1])
      return fail(c, PLSVO_E_CAPACITY, "seeds_keyframe_detect: a stream's line-seed list lacks rows (plsvo_seeds_reserve); nothing was changed");
  if (ts > (size_t)INT32_MAX) return fail(c, PLSVO_E_CAPACITY, "seeds_keyframe_detect: batch too large");
  if (n_act == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t A = (size_t)n_act;
  Blob blob;
  const size_t b_jobs = blob.reserve<SeedStartJobDev>(A);
  const size_t s_px = blob.reserve<double>(ts * 2), s_f = blob.reserve<double>(ts * 3), s_sf = blob.reserve<double>(ts * 3), s_ef = blob.reserve<double>(ts * 3),
               s_spx = blob.reserve<double>(ts * 2), s_epx = blob.reserve<double>(ts * 2), s_lv = blob.reserve<int>(ts);
  auto put = [&](size_t sec, size_t at, const void* src, size_t count, size_t elem) { if (count && src) memcpy(blob.host.data() + sec + at * elem, src, count * elem); };
  size_t as = 0;
  int pos = 0;
  for (int s = 0; s < n; ++s) {
    const plsvo_seed_kf_detect& I = in[s];
    if (!I.active) continue;
    SeedStartJobDev& J = blob.at<SeedStartJobDev>(b_jobs)[pos++];
    memset(&J, 0, sizeof(J));
    J.stream = s; J.removed_kf = I.removed_kf; J.new_batch = I.new_batch ? 1 : 0; J.new_kf = I.new_kf; J.occ_sources = I.occ_sources; J.n_seg = I.n_seg;
    J.lim_pt = c->sd_lim[2 * (size_t)s]; J.seg_at = (long long)as; J.d_occ = I.d_occupancy;
    if (I.occ_sources & PLSVO_SEED_OCC_UPDATED) for (int k = 0; k < 6; ++k) J.n_upd_rows += c->sd_last[(size_t)s].pt[k];
    {                                               // PointSeed::PointSeed / LineSeed::LineSeed (:53-74): float arguments, float members
      const float depth_mean = (float)I.depth_mean, depth_min = (float)I.depth_min;
      const float mu = 1.0 / depth_mean, z_range = 1.0 / depth_min;
      const float sigma2 = z_range * z_range / 36;
      J.mu = mu; J.z_range = z_range; J.sigma2 = sigma2;
    }
    const size_t ns = (size_t)I.n_seg;
    put(s_px, as * 2, I.seg_px, ns * 2, 8); put(s_f, as * 3, I.seg_f, ns * 3, 8); put(s_sf, as * 3, I.seg_sf, ns * 3, 8); put(s_ef, as * 3, I.seg_ef, ns * 3, 8);
    put(s_spx, as * 2, I.seg_spx, ns * 2, 8); put(s_epx, as * 2, I.seg_epx, ns * 2, 8); put(s_lv, as, I.seg_level, ns, 4);
    as += ns;
  }
  if (const int rc = upload_blob(c, c->sd_d_in, blob)) return rc;
  HIP_TRY(c, c->sk_d_occ.ensure(A * (size_t)cells));
  HIP_TRY(c, c->sk_d_slots.ensure(A * sizeof(int)));
  const char* d = reinterpret_cast<const char*>(c->sd_d_in.p);
  auto D = [&](size_t o) { return reinterpret_cast<const double*>(d + o); };
  SeedStartBatchDev b{};
  b.l = c->sd_b;
  b.l.k_seg_px = D(s_px); b.l.k_seg_f = D(s_f); b.l.k_seg_sf = D(s_sf); b.l.k_seg_ef = D(s_ef); b.l.k_seg_spx = D(s_spx); b.l.k_seg_epx = D(s_epx);
  b.l.k_seg_level = reinterpret_cast<const int*>(d + s_lv);
  b.jobs = reinterpret_cast<const SeedStartJobDev*>(d + b_jobs); b.n_act = n_act;
  b.cell = p->cell_size; b.cols = cols; b.n_cells = cells; b.width = c->pyr.w[0]; b.height = c->pyr.h[0];
  b.f_pt_px = c->cs_b.f_pt_px; b.scalars = c->cs_b.scalars;   // (read under PLSVO_SEED_OCC_SELECTED only)
  b.occ = c->sk_d_occ.as<uint8_t>(); b.slots = c->sk_d_slots.as<int>(); b.report = c->sk_d_report.as<SeedStartReportDev>();
  {
    EventPair ep{}; prof_begin(c, PLSVO_K_NEWCAND, &ep);
    // the occupancy rows are re-armed ahead of every launch, as the tail split re-arms its flags: the kernel only ever stores a 1
    hipError_t launched = hipMemsetAsync(b.occ, 0, A * (size_t)cells, c->stream);
    if (launched == hipSuccess) launched = launch_seeds_occupancy(b, c->stream);
    int rc = PLSVO_OK;
    if (launched == hipSuccess) {
      rc = detect_enqueue_keys(c, 0, b.slots, n_act, p, cells, cols, b.occ);
      b.keys = c->det_keys.as<unsigned long long>();
      if (rc == PLSVO_OK) {
        launched = launch_seeds_start(b, c->stream);
        // the start launch is what re-arms the keys: if it could not be enqueued behind the detection, a memset arms them in its place
        if (launched != hipSuccess) (void)hipMemsetAsync(b.keys, 0, A * (size_t)cells * sizeof(unsigned long long), c->stream);
      }
    }
    prof_end(c, PLSVO_K_NEWCAND, &ep);
    if (rc) return rc;
    HIP_TRY(c, launched);
  }
  for (int s = 0; s < n; ++s) {                     // upper bounds until a fetch: the device alone knows the corners, and with no_room it appends no segment either
    if (!in[s].active) continue;
    SeedStreamDev& S = c->sd_host[(size_t)s];
    S.n_pt = (int)std::min((long long)S.n_pt + cells, (long long)c->sd_lim[2 * (size_t)s]); S.n_seg += in[s].n_seg; S.batch_counter += in[s].new_batch ? 1 : 0;
  }
  c->sd_max_level = max_level;
  c->sk_have_report = true;
  return PLSVO_OK;
}

extern "C" int plsvo_seeds_keyframe_fetch(plsvo_ctx* c, int n, plsvo_seed_kf_report* out) {
  CTX_CHECK(c);
  if (const int rc = seeds_ready(c, n, out, "seeds_keyframe_fetch")) return rc;
  if (!c->sk_have_report) return fail(c, PLSVO_E_STATE, "seeds_keyframe_fetch: no plsvo_seeds_keyframe_detect since the seed tables were staged");
  static_assert(sizeof(SeedStartReportDev) == sizeof(plsvo_seed_kf_report) && sizeof(plsvo_seed_kf_report) == 32, "the device's report is the public one");
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(out, c->sk_d_report.p, (size_t)n * sizeof(plsvo_seed_kf_report), hipMemcpyDeviceToHost, c->stream));   // (the caller's own buffer: a plain copy, landed by the wait below)
  Readback rb;
  rb.add(c->sd_b.streams, (size_t)n * sizeof(SeedStreamDev));
  if (const int rc = rb.wait(c)) return rc;
  const SeedStreamDev* const streams = rb.at<SeedStreamDev>(0);
  for (int s = 0; s < n; ++s) {                     // the mirrors are exact again, as behind plsvo_seeds_fetch_lists
    SeedStreamDev& S = c->sd_host[(size_t)s];
    S.n_pt = streams[s].n_pt; S.n_seg = streams[s].n_seg; S.batch_counter = streams[s].batch_counter;
  }
  return PLSVO_OK;
}

extern "C" int plsvo_seeds_fetch_lists(plsvo_ctx* c, int n, plsvo_seed_list* out) {
  CTX_CHECK(c);
  if (const int rc = seeds_ready(c, n, out, "seeds_fetch_lists")) return rc;
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  Readback rb;                                     // the tables are one allocation: one range
  rb.add(c->sd_d_tab.p, c->sd_tab_bytes);
  if (const int rc = rb.wait(c)) return rc;
  const char* const h = rb.at<char>(0);
  const SeedListBatchDev& b = c->sd_b; const SeedsBatchDev& q = b.s;
  const char* base = reinterpret_cast<const char*>(c->sd_d_tab.p);
  auto cp = [&](void* dst, const void* dev, size_t at, size_t count, size_t elem) { if (dst && count) memcpy(dst, h + (reinterpret_cast<const char*>(dev) - base) + at * elem, count * elem); };
  const SeedStreamDev* streams = reinterpret_cast<const SeedStreamDev*>(h + (reinterpret_cast<const char*>(b.streams) - base));
  for (int s = 0; s < n; ++s) {
    const SeedStreamDev& S = streams[s]; plsvo_seed_list& O = out[s];
    const size_t np = (size_t)S.n_pt, ns = (size_t)S.n_seg, po = (size_t)S.pt_off, so = (size_t)S.seg_off;
    O.n_pt = S.n_pt; O.n_seg = S.n_seg; O.batch_counter = S.batch_counter; O.reserved0 = 0;
    cp(O.pt_ref_kf, q.pt_ref_frame, po, np, 4); cp(O.pt_batch_id, b.pt_batch_id, po, np, 4); cp(O.pt_px, q.pt_px, po * 2, np * 2, 8); cp(O.pt_f, q.pt_f, po * 3, np * 3, 8);
    cp(O.pt_level, q.pt_level, po, np, 4); cp(O.pt_type, q.pt_type, po, np, 1); cp(O.pt_grad, q.pt_grad, po * 2, np * 2, 8); cp(O.pt_a, q.pt_a, po, np, 4); cp(O.pt_b, q.pt_b, po, np, 4);
    cp(O.pt_mu, q.pt_mu, po, np, 4); cp(O.pt_z_range, q.pt_z_range, po, np, 4); cp(O.pt_sigma2, q.pt_sigma2, po, np, 4);
    cp(O.seg_ref_kf, q.seg_ref_frame, so, ns, 4); cp(O.seg_batch_id, b.seg_batch_id, so, ns, 4); cp(O.seg_px, q.seg_px, so * 2, ns * 2, 8); cp(O.seg_f, q.seg_f, so * 3, ns * 3, 8);
    cp(O.seg_sf, q.seg_sf, so * 3, ns * 3, 8); cp(O.seg_ef, q.seg_ef, so * 3, ns * 3, 8); cp(O.seg_spx, b.seg_spx, so * 2, ns * 2, 8); cp(O.seg_epx, b.seg_epx, so * 2, ns * 2, 8);
    cp(O.seg_level, q.seg_level, so, ns, 4); cp(O.seg_a, q.seg_a, so, ns, 4); cp(O.seg_b, q.seg_b, so, ns, 4); cp(O.seg_mu_s, q.seg_mu_s, so, ns, 4); cp(O.seg_mu_e, q.seg_mu_e, so, ns, 4);
    cp(O.seg_z_range_s, q.seg_z_range_s, so, ns, 4); cp(O.seg_z_range_e, q.seg_z_range_e, so, ns, 4); cp(O.seg_sigma2_s, q.seg_sigma2_s, so, ns, 4); cp(O.seg_sigma2_e, q.seg_sigma2_e, so, ns, 4);
    c->sd_host[(size_t)s].n_pt = S.n_pt; c->sd_host[(size_t)s].n_seg = S.n_seg;   // (exact again behind a keyframe event with a removal)
  }
  return PLSVO_OK;
}

extern "C" int plsvo_seeds_fetch_rows(plsvo_ctx* c, int n, plsvo_seed_rows* out) {
  CTX_CHECK(c);
  if (const int rc = seeds_ready(c, n, out, "seeds_fetch_rows")) return rc;
  if (!c->sd_have_report) return fail(c, PLSVO_E_STATE, "seeds_fetch_rows: no fetched update since the seed tables were staged");
  if (n == 0) return PLSVO_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const SeedWorkSections W = seed_work_sections((size_t)n, c->sd_t_pt, c->sd_t_seg);
  Readback rb;
  rb.add(c->sd_d_work.p, W.end);
  if (const int rc = rb.wait(c)) return rc;
  auto cp = [&](void* dst, size_t sec, size_t at, size_t count, size_t elem) { if (dst && count) memcpy(dst, rb.at<char>(0) + sec + at * elem, count * elem); };
  for (int s = 0; s < n; ++s) {
    const SeedReportDev& R = c->sd_last[(size_t)s]; const SeedStreamDev& S = c->sd_host[(size_t)s]; plsvo_seed_rows& O = out[s];
    size_t np = 0, ns = 0;
    for (int k = 0; k < 6; ++k) { np += (size_t)R.pt[k]; ns += (size_t)R.seg[k]; }
    const size_t po = (size_t)S.pt_off, so = (size_t)S.seg_off;
    O.n_pt = (int32_t)np; O.n_seg = (int32_t)ns; O.active = np + ns > 0; O.reserved0 = 0;
    cp(O.pt_status, W.p_st, po, np, 4); cp(O.pt_a, W.p_a, po, np, 4); cp(O.pt_b, W.p_b, po, np, 4); cp(O.pt_mu, W.p_mu, po, np, 4); cp(O.pt_sigma2, W.p_s2, po, np, 4);
    cp(O.pt_xyz_world, W.p_xyz, po * 3, np * 3, 8); cp(O.pt_px_cur, W.p_px, po * 2, np * 2, 8); cp(O.pt_depth, W.p_z, po, np, 8);
    cp(O.seg_status, W.s_st, so, ns, 4); cp(O.seg_a, W.s_a, so, ns, 4); cp(O.seg_b, W.s_b, so, ns, 4); cp(O.seg_mu_s, W.s_mus, so, ns, 4); cp(O.seg_mu_e, W.s_mue, so, ns, 4);
    cp(O.seg_sigma2_s, W.s_s2s, so, ns, 4); cp(O.seg_sigma2_e, W.s_s2e, so, ns, 4); cp(O.seg_xyz_world_s, W.s_xs, so * 3, ns * 3, 8); cp(O.seg_xyz_world_e, W.s_xe, so * 3, ns * 3, 8);
    cp(O.seg_depth_s, W.s_zs, so, ns, 8); cp(O.seg_depth_e, W.s_ze, so, ns, 8);
  }
  return PLSVO_OK;
}
