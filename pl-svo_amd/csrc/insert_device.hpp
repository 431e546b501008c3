// insert_device.hpp -- the frame of the last candidate run becomes a keyframe of the resident map tables on gfx950: one WAVE per stream,
// four waves per workgroup, no LDS, nothing synchronised across waves; a stream that does not insert returns at once.  Included by
// seeds_kernels.hip (compiled with -ffp-contract=off: every table is bit-identical to tests/np_insert.py; the only floating-point work
// is sel_bearing on the segments' end points, a point's bearing is copied from the row the selection wrote for the pose optimiser).
//
//   map_insert_plan_kernel   decides and counts, writing scratch only: the plan the host checks against the stream's room
//   map_insert_kernel        builds the new lists in a staging copy of the stream's rows, then copies them back
//
//   the rejected features (src/pose_optimizer.cpp:218, :239), addFrameRef of every feature (src/frame_handler_mono.cpp:358-369,
//   include/plsvo/feature3D.h:202-206), addCandidatePointToFrame / addCandidateSegmentToFrame (src/map.cpp:292-309, :384-401),
//   safeDeleteFrame with removePtFrameRef / removeLsFrameRef (:53-114), safeDeletePoint / safeDeleteSegment (:116-139),
//   removeFrameCandidates (:326-340), addKeyframe (:153-156)
//
// The sequential loops of the reference become order-independent forms:
//   * "the front observation is in the new frame" (addCandidate*ToFrame): some feature of the new frame holds the landmark -- the lowest
//     and the highest feature index per landmark (atomicMin / atomicMax; a segment can be a feature twice, the later one in front);
//   * removePtFrameRef over the removed keyframe's list: what happens to a landmark depends only on its list length after the pushes and
//     on how many features of that keyframe hold it (atomicAdd per feature, the joined original features included) -- one lane per
//     landmark plays its own few steps: erase the first observations in that keyframe while the list is longer than two, then delete;
//   * every new list is a gather: the new observation(s), the old list less the erased entries; a keyframe's old features, then the
//     original features that joined it in candidate-list order (ballot prefix per keyframe); offsets are prefix sums in rounds of 64;
//   * the candidate lists close up with the selection's stable compaction.
// Lists shift in both directions, so nothing is shuffled under its readers: the wave gathers into the staging rows, waits, and copies
// them over its own rows.  A refused call has run the plan only, which writes scratch.
#pragma once
#include <hip/hip_runtime.h>

#include "select_device.hpp"

namespace plsvo_hip {

#pragma clang fp contract(off)

constexpr int kInsWaves = kSelWaves;
constexpr uint8_t kInsJoined = 32;                  // event bit: a candidate whose original feature joined its keyframe (reported as PLSVO_LM_EVENT_JOINED)
constexpr unsigned int kInsNone = 0xffffffffu;
constexpr int kInsCandRemoved = 1 << 16;

__device__ __forceinline__ int ins_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int ins_wave_scan(int v, int lane) {          // inclusive
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(v, (unsigned)d, 64); if (lane >= d) v += t; }
  return v;
}

// one kind of landmark of one stream: its rows of the resident tables, of the selection's features and of the insertion's scratch
struct InsView {
  int n_lm, n_kf, n_cand, n_feat, remove;
  int* kf_off; int* kf_lm; int* type; int* nfail; uint8_t* event; int* cand;
  int* obs_off; int* obs_kf; int* obs_level; double* obs_a; double* obs_b; double* obs_c; double* obs_d; uint8_t* obs_type;
  const int* f_lm; const uint8_t* keep;
  InsertKindDev k;                                  // scratch and staging, advanced to the stream's rows
};

template <bool SEG>
__device__ __forceinline__ InsView ins_view(const InsertBatchDev& b, const CandMapDev& M, const InsertJobDev& J, int job) {
  const SelectBatchDev& s = b.s; const CandBatchDev& c = s.c;
  const InsertKindDev& K = SEG ? b.seg : b.pt;
  InsView V;
  const long long lm_off = SEG ? M.seg_off : M.pt_off, kf_ftr = SEG ? M.kfseg_off : M.kfpt_off, obs = SEG ? M.segobs_off : M.ptobs_off;
  const long long cnd = SEG ? M.segc_off : M.ptc_off, ftr = SEG ? 2 * M.oseg_off : M.opt_off;
  V.n_lm = SEG ? M.n_seg : M.n_pt; V.n_kf = M.n_kf; V.n_cand = SEG ? M.n_seg_cand : M.n_pt_cand; V.n_feat = s.scalars[3 * job + (SEG ? 1 : 0)]; V.remove = J.remove_kf;
  V.kf_off = const_cast<int*>(SEG ? c.kf_seg_off : c.kf_pt_off) + M.kf_off + M.stream; V.kf_lm = const_cast<int*>(SEG ? c.kf_seg_lm : c.kf_pt_lm) + kf_ftr;
  V.type = const_cast<int*>(SEG ? c.seg_type : c.pt_type) + lm_off; V.nfail = (SEG ? s.seg_nfail : s.pt_nfail) + lm_off; V.event = (SEG ? s.seg_event : s.pt_event) + lm_off;
  V.cand = const_cast<int*>(SEG ? c.seg_cand : c.pt_cand) + cnd;
  V.obs_off = const_cast<int*>(SEG ? c.seg_obs_off : c.pt_obs_off) + lm_off + M.stream;
  V.obs_kf = const_cast<int*>(SEG ? c.seg_obs_kf : c.pt_obs_kf) + obs; V.obs_level = const_cast<int*>(SEG ? c.seg_obs_level : c.pt_obs_level) + obs;
  if (SEG) {
    V.obs_a = const_cast<double*>(c.seg_obs_spx) + 2 * obs; V.obs_b = const_cast<double*>(c.seg_obs_epx) + 2 * obs;
    V.obs_c = const_cast<double*>(c.seg_obs_sf) + 3 * obs; V.obs_d = const_cast<double*>(c.seg_obs_ef) + 3 * obs; V.obs_type = nullptr;
  } else {
    V.obs_a = const_cast<double*>(c.pt_obs_px) + 2 * obs; V.obs_b = const_cast<double*>(c.pt_obs_f) + 3 * obs;
    V.obs_c = const_cast<double*>(c.pt_obs_grad) + 2 * obs; V.obs_d = nullptr; V.obs_type = const_cast<uint8_t*>(c.pt_obs_type) + obs;
  }
  V.f_lm = (SEG ? s.f_seg_lm : s.f_pt_lm) + ftr; V.keep = (SEG ? J.seg_keep : J.pt_keep) + ftr;
  V.k.f0 = K.f0 + lm_off; V.k.f1 = K.f1 + lm_off; V.k.cnt = K.cnt + lm_off; V.k.len = K.len + lm_off; V.k.erase = K.erase + lm_off;
  V.k.cand_kf = K.cand_kf + cnd; V.k.new_lm = K.new_lm + ftr;
  V.k.kf_off2 = K.kf_off2 + M.kf_off + M.stream; V.k.kf_lm2 = K.kf_lm2 + kf_ftr; V.k.obs_off2 = K.obs_off2 + lm_off + M.stream;
  V.k.obs_kf2 = K.obs_kf2 + obs; V.k.obs_level2 = K.obs_level2 + obs;
  V.k.obs_a2 = K.obs_a2 + 2 * obs; V.k.obs_b2 = K.obs_b2 + (SEG ? 2 : 3) * obs; V.k.obs_c2 = K.obs_c2 + (SEG ? 3 : 2) * obs;
  V.k.obs_d2 = SEG ? K.obs_d2 + 3 * obs : nullptr; V.k.obs_type2 = SEG ? nullptr : K.obs_type2 + obs;
  return V;
}

// The decisions of one kind, in scratch.  out: features in the keyframes' lists, observations, candidates left, joined, deleted.
__device__ __forceinline__ void ins_plan_kind(const InsView& V, int* out) {
  const int lane = threadIdx.x & 63;
  for (int lm = lane; lm < V.n_lm; lm += 64) { V.k.f0[lm] = kInsNone; V.k.f1[lm] = 0u; V.k.cnt[lm] = 0; }
  cand_wave_sync();
  // -- the new frame's features: a rejected feature and one on a deleted landmark have no landmark
  for (int i = lane; i < V.n_feat; i += 64) {
    int lm = V.f_lm[i];
    if (!V.keep[i] || V.type[lm] == PLSVO_LM_DELETED) lm = -1;
    V.k.new_lm[i] = lm;
    if (lm >= 0) { atomicMin(&V.k.f0[lm], (unsigned int)i); atomicMax(&V.k.f1[lm], (unsigned int)i + 1u); }
  }
  cand_wave_sync();
  // -- the candidate lists: an entry whose landmark the new frame observes joins the keyframe of its original feature (the LAST observation)
  int n_left = 0, n_joined = 0, n_joined_removed = 0;
  for (int base = 0; base < V.n_cand; base += 64) {
    const int j = base + lane;
    int to = -1;
    if (j < V.n_cand) {
      const int lm = V.cand[j], o0 = V.obs_off[lm], o1 = V.obs_off[lm + 1];
      const int orig = o1 > o0 ? V.obs_kf[o1 - 1] : V.n_kf;        // (an empty list: its only observation is the new frame's)
      if (cand_visit_load(&V.k.f0[lm]) != kInsNone) { to = orig; if (orig == V.remove) atomicAdd(&V.k.cnt[lm], 1); }
      else if (V.remove >= 0 && orig == V.remove) { to = -2; atomicAdd(&V.k.cnt[lm], kInsCandRemoved); }
      V.k.cand_kf[j] = to;
    }
    n_left += __popcll(__ballot(j < V.n_cand && to == -1));
    n_joined += __popcll(__ballot(to >= 0));
    n_joined_removed += __popcll(__ballot(to >= 0 && to == V.remove));
  }
  // -- the removed keyframe's own features
  int n_removed_ftr = 0;
  if (V.remove >= 0) {
    const int r0 = V.kf_off[V.remove], r1 = V.kf_off[V.remove + 1];
    n_removed_ftr = r1 - r0;
    for (int j = r0 + lane; j < r1; j += 64) {
      const int lm = V.kf_lm[j];
      if (lm >= 0) atomicAdd(&V.k.cnt[lm], 1);
    }
  }
  cand_wave_sync();
  // -- one lane per landmark: removePtFrameRef / removeLsFrameRef once per feature of the removed keyframe that holds it
  int n_obs = 0, n_deleted = 0;
  for (int base = 0; base < V.n_lm; base += 64) {
    const int lm = base + lane;
    int len = 0;
    bool del = false;
    if (lm < V.n_lm) {
      const unsigned int f0 = cand_visit_load(&V.k.f0[lm]), f1 = cand_visit_load(&V.k.f1[lm]);
      const int cw = (int)cand_visit_load(reinterpret_cast<const unsigned int*>(&V.k.cnt[lm]));
      const int o0 = V.obs_off[lm], o1 = V.obs_off[lm + 1];
      const int n_new = f0 == kInsNone ? 0 : (f1 - 1u != f0 ? 2 : 1);
      const bool was_deleted = V.type[lm] == PLSVO_LM_DELETED;
      int held = cw & (kInsCandRemoved - 1), in_removed = 0, erase = 0;
      if (V.remove >= 0 && (held > 0 || was_deleted))
        for (int o = o0; o < o1; ++o) in_removed += V.obs_kf[o] == V.remove ? 1 : 0;
      len = (o1 - o0) + n_new;
      del = cw >= kInsCandRemoved;                  // removeFrameCandidates
      for (int left = in_removed; held > 0 && !del; --held) {
        if (len <= 2) del = true;                   // safeDeletePoint / safeDeleteSegment
        else if (left > 0) { --left; --len; ++erase; }   // deleteFrameRef: the first one in that keyframe
      }
      if (!del && was_deleted) { len -= in_removed - erase; erase = in_removed; }   // deleted earlier: the removed row leaves its list
      if (del) len = 0;
      V.k.len[lm] = len; V.k.erase[lm] = del ? -1 : erase;
    }
    n_obs += ins_wave_sum(len);
    n_deleted += __popcll(__ballot(del));
  }
  out[0] = V.kf_off[V.n_kf] - n_removed_ftr + (n_joined - n_joined_removed) + V.n_feat;
  out[1] = n_obs; out[2] = n_left; out[3] = n_joined; out[4] = n_deleted;
}

__global__ __launch_bounds__(64 * kInsWaves) void map_insert_plan_kernel(const InsertBatchDev b) {
  const int lane = threadIdx.x & 63;
  const int job = blockIdx.x * kInsWaves + (int)(threadIdx.x >> 6);
  if (job >= b.s.c.n_jobs) return;                  // whole waves leave: nothing below synchronises across waves
  const InsertJobDev& J = b.jobs[job];
  const CandMapDev& M = b.s.c.maps[job];
  if (!J.is_kf) {                                   // not touched: its sizes as they stand, for the report
    if (lane == 0) {
      const CandBatchDev& c = b.s.c;
      InsertPlanDev O = {};
      O.n_kf = M.n_kf; O.new_kf = -1; O.n_pt_cand = M.n_pt_cand; O.n_seg_cand = M.n_seg_cand;
      O.n_kf_pt = (c.kf_pt_off + M.kf_off + M.stream)[M.n_kf]; O.n_kf_seg = (c.kf_seg_off + M.kf_off + M.stream)[M.n_kf];
      O.n_pt_obs = (c.pt_obs_off + M.pt_off + M.stream)[M.n_pt]; O.n_seg_obs = (c.seg_obs_off + M.seg_off + M.stream)[M.n_seg];
      b.plan[job] = O;
    }
    return;
  }
  int p[5], s[5];
  ins_plan_kind(ins_view<false>(b, M, J, job), p);
  ins_plan_kind(ins_view<true>(b, M, J, job), s);
  if (lane == 0) {
    InsertPlanDev& O = b.plan[job];
    O.n_kf = M.n_kf + 1 - (J.remove_kf >= 0 ? 1 : 0); O.new_kf = O.n_kf - 1;
    O.n_kf_pt = p[0]; O.n_pt_obs = p[1]; O.n_pt_cand = p[2]; O.n_joined_pt = p[3]; O.n_deleted_pt = p[4];
    O.n_kf_seg = s[0]; O.n_seg_obs = s[1]; O.n_seg_cand = s[2]; O.n_joined_seg = s[3]; O.n_deleted_seg = s[4];
  }
}

// One kind's new tables from the plan's scratch.  Returns the candidates left.
template <bool SEG>
__device__ __forceinline__ int ins_commit_kind(const InsertBatchDev& b, const CandMapDev& M, const InsView& V) {
  const SelectBatchDev& s = b.s;
  const int lane = threadIdx.x & 63;
  const kf_u64 below = ((kf_u64)1 << lane) - 1;
  const int shift_from = V.remove >= 0 ? V.remove : 0x7fffffff;       // keyframe indices above it drop by one
  const int new_kf = V.n_kf - (V.remove >= 0 ? 1 : 0);                // the new keyframe's index in the final table
  // -- observation offsets: prefix sums of the new lengths
  int total = 0;
  for (int base = 0; base < V.n_lm; base += 64) {
    const int lm = base + lane;
    const int len = lm < V.n_lm ? V.k.len[lm] : 0;
    const int incl = ins_wave_scan(len, lane);
    if (lm < V.n_lm) V.k.obs_off2[lm] = total + incl - len;
    total += __shfl(incl, 63, 64);
  }
  if (lane == 0) V.k.obs_off2[V.n_lm] = total;
  // -- observation lists: the new frame's in front (the later feature first), then the old list less the erased entries
  for (int lm = lane; lm < V.n_lm; lm += 64) {
    const int erase = V.k.erase[lm];
    if (erase < 0) continue;
    int at = V.k.obs_off2[lm];                      // (this lane's own store above)
    const unsigned int f0 = cand_visit_load(&V.k.f0[lm]), f1 = cand_visit_load(&V.k.f1[lm]);
    for (int k = 0; k < 2 && f0 != kInsNone; ++k) {
      const unsigned int i = k == 0 ? f1 - 1u : f0;
      if (k == 1 && f1 - 1u == f0) break;
      V.k.obs_kf2[at] = new_kf;
      if (SEG) {
        const long long o = 2 * M.oseg_off + i;
        const double spx[2] = { s.f_seg_px[4 * o], s.f_seg_px[4 * o + 1] }, epx[2] = { s.f_seg_px[4 * o + 2], s.f_seg_px[4 * o + 3] };
        double sf[3], ef[3];
        sel_bearing(s.c, spx, sf); sel_bearing(s.c, epx, ef);
        V.k.obs_a2[2 * at] = spx[0]; V.k.obs_a2[2 * at + 1] = spx[1]; V.k.obs_b2[2 * at] = epx[0]; V.k.obs_b2[2 * at + 1] = epx[1];
#pragma unroll
        for (int d = 0; d < 3; ++d) { V.k.obs_c2[3 * at + d] = sf[d]; V.k.obs_d2[3 * at + d] = ef[d]; }
        V.k.obs_level2[at] = s.f_seg_level[o];
      } else {
        const long long o = M.opt_off + i;
        V.k.obs_a2[2 * at] = s.f_pt_px[2 * o]; V.k.obs_a2[2 * at + 1] = s.f_pt_px[2 * o + 1];
#pragma unroll
        for (int d = 0; d < 3; ++d) V.k.obs_b2[3 * at + d] = s.pt_f[3 * o + d];
        V.k.obs_c2[2 * at] = s.f_pt_grad[2 * o]; V.k.obs_c2[2 * at + 1] = s.f_pt_grad[2 * o + 1];
        V.k.obs_level2[at] = s.f_pt_level[o]; V.k.obs_type2[at] = s.f_pt_type[o];
      }
      ++at;
    }
    int left = erase;
    for (int o = V.obs_off[lm]; o < V.obs_off[lm + 1]; ++o) {
      const int kf = V.obs_kf[o];
      if (kf == V.remove && left > 0) { --left; continue; }
      V.k.obs_kf2[at] = kf > shift_from ? kf - 1 : kf; V.k.obs_level2[at] = V.obs_level[o];
      V.k.obs_a2[2 * at] = V.obs_a[2 * o]; V.k.obs_a2[2 * at + 1] = V.obs_a[2 * o + 1];
      if (SEG) {
        V.k.obs_b2[2 * at] = V.obs_b[2 * o]; V.k.obs_b2[2 * at + 1] = V.obs_b[2 * o + 1];
#pragma unroll
        for (int d = 0; d < 3; ++d) { V.k.obs_c2[3 * at + d] = V.obs_c[3 * o + d]; V.k.obs_d2[3 * at + d] = V.obs_d[3 * o + d]; }
      } else {
#pragma unroll
        for (int d = 0; d < 3; ++d) V.k.obs_b2[3 * at + d] = V.obs_b[3 * o + d];
        V.k.obs_c2[2 * at] = V.obs_c[2 * o]; V.k.obs_c2[2 * at + 1] = V.obs_c[2 * o + 1];
        V.k.obs_type2[at] = V.obs_type[o];
      }
      ++at;
    }
  }
  // -- the keyframes' feature lists: the old features, then the original features that joined, in candidate-list order; the new frame last
  int n_ftr = 0, row = 0;
  for (int k = 0; k <= V.n_kf; ++k) {               // (wave-uniform)
    if (k == V.remove) continue;
    if (lane == 0) V.k.kf_off2[row] = n_ftr;
    const int* list = k < V.n_kf ? V.kf_lm + V.kf_off[k] : V.k.new_lm;
    const int len = k < V.n_kf ? V.kf_off[k + 1] - V.kf_off[k] : V.n_feat;
    for (int j = lane; j < len; j += 64) {
      int lm = list[j];
      if (lm >= 0 && V.k.erase[lm] < 0) lm = -1;    // ftr->feat3D = NULL
      V.k.kf_lm2[n_ftr + j] = lm;
    }
    n_ftr += len;
    for (int base = 0; base < V.n_cand; base += 64) {
      const int j = base + lane;
      const bool here = j < V.n_cand && V.k.cand_kf[j] == k;
      const kf_u64 mask = __ballot(here);
      if (here) {
        int lm = V.cand[j];
        if (V.k.erase[lm] < 0) lm = -1;
        V.k.kf_lm2[n_ftr + __popcll(mask & below)] = lm;
      }
      n_ftr += __popcll(mask);
    }
    ++row;
  }
  if (lane == 0) V.k.kf_off2[row] = n_ftr;
  // -- the landmarks: a joined candidate is TYPE_UNKNOWN without failures; a deleted one is TYPE_DELETED
  for (int j = lane; j < V.n_cand; j += 64)
    if (V.k.cand_kf[j] >= 0) { const int lm = V.cand[j]; V.type[lm] = PLSVO_LM_UNKNOWN; V.nfail[lm] = 0; V.event[lm] |= kInsJoined; }
  cand_wave_sync();
  for (int lm = lane; lm < V.n_lm; lm += 64)
    if (V.k.erase[lm] < 0) { V.type[lm] = PLSVO_LM_DELETED; V.event[lm] |= kSelDeleted; }
  // -- the candidate list closes up
  int kept = 0;
  for (int base = 0; base < V.n_cand; base += 64) {
    const int j = base + lane;
    int lm = -1;
    bool keep = false;
    if (j < V.n_cand) { lm = V.cand[j]; keep = V.k.cand_kf[j] == -1; }
    const kf_u64 mask = __ballot(keep);             // every lane's load is back before the first store of the round
    if (keep) V.cand[kept + __popcll(mask & below)] = lm;
    kept += __popcll(mask);
  }
  cand_wave_sync();                                 // the staging rows are complete, and every read of the old rows is done
  // -- the staging rows become the stream's rows
  for (int i = lane; i <= row; i += 64) V.kf_off[i] = V.k.kf_off2[i];
  for (int i = lane; i < n_ftr; i += 64) V.kf_lm[i] = V.k.kf_lm2[i];
  for (int i = lane; i <= V.n_lm; i += 64) V.obs_off[i] = V.k.obs_off2[i];
  for (int i = lane; i < total; i += 64) {
    V.obs_kf[i] = V.k.obs_kf2[i]; V.obs_level[i] = V.k.obs_level2[i];
    V.obs_a[2 * i] = V.k.obs_a2[2 * i]; V.obs_a[2 * i + 1] = V.k.obs_a2[2 * i + 1];
    if (SEG) {
      V.obs_b[2 * i] = V.k.obs_b2[2 * i]; V.obs_b[2 * i + 1] = V.k.obs_b2[2 * i + 1];
#pragma unroll
      for (int d = 0; d < 3; ++d) { V.obs_c[3 * i + d] = V.k.obs_c2[3 * i + d]; V.obs_d[3 * i + d] = V.k.obs_d2[3 * i + d]; }
    } else {
#pragma unroll
      for (int d = 0; d < 3; ++d) V.obs_b[3 * i + d] = V.k.obs_b2[3 * i + d];
      V.obs_c[2 * i] = V.k.obs_c2[2 * i]; V.obs_c[2 * i + 1] = V.k.obs_c2[2 * i + 1];
      V.obs_type[i] = V.k.obs_type2[i];
    }
  }
  return kept;
}

__global__ __launch_bounds__(64 * kInsWaves) void map_insert_kernel(const InsertBatchDev b) {
  const CandBatchDev& c = b.s.c;
  const int lane = threadIdx.x & 63;
  const int job = blockIdx.x * kInsWaves + (int)(threadIdx.x >> 6);
  if (job >= c.n_jobs) return;                      // whole waves leave: nothing below synchronises across waves
  const InsertJobDev& J = b.jobs[job];
  if (!J.is_kf) return;
  CandMapDev& M = const_cast<CandMapDev&>(c.maps[job]);
  const int n_kf = M.n_kf, remove = J.remove_kf;
  const int n_ptc = ins_commit_kind<false>(b, M, ins_view<false>(b, M, J, job));
  const int n_segc = ins_commit_kind<true>(b, M, ins_view<true>(b, M, J, job));
  // -- safeDeleteFrame takes the row out, addKeyframe appends the new one; the matcher's frame table follows the keyframe table
  double* const kf_T = const_cast<double*>(c.kf_T) + 7 * M.kf_off;
  double* const fr_T = c.frame_T + 7 * M.f_off; int* const fr_slot = c.frame_slot + M.f_off;
  const int new_kf = n_kf - (remove >= 0 ? 1 : 0);
  if (remove >= 0) {
    for (int base = remove; base < n_kf - 1; base += 64) {
      const int i = base + lane;
      double T[7] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
      int slot = 0;
      if (i < n_kf - 1) {
#pragma unroll
        for (int d = 0; d < 7; ++d) T[d] = kf_T[7 * (i + 1) + d];
        slot = fr_slot[i + 1];
      }
      cand_wave_sync();                             // every lane's row is in registers before the row below it is overwritten
      if (i < n_kf - 1) {
#pragma unroll
        for (int d = 0; d < 7; ++d) { kf_T[7 * i + d] = T[d]; fr_T[7 * i + d] = T[d]; }
        fr_slot[i] = slot;
      }
      cand_wave_sync();
    }
  }
  if (lane == 0) {
    const double* T = J.d_T ? J.d_T : J.T;
#pragma unroll
    for (int d = 0; d < 7; ++d) { kf_T[7 * new_kf + d] = T[d]; fr_T[7 * new_kf + d] = T[d]; }
    fr_slot[new_kf] = J.kf_slot;
    M.n_kf = new_kf + 1; M.n_pt_cand = n_ptc; M.n_seg_cand = n_segc;
  }
}

// FrameHandlerBase::optimizeStructure's result: one thread per moved landmark (a landmark is listed once)
__global__ __launch_bounds__(256) void map_set_positions_kernel(const PositionsBatchDev b) {
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i < b.n_pt) {
    const long long at = b.pt_at[i];
#pragma unroll
    for (int d = 0; d < 3; ++d) b.pt_pos[3 * at + d] = b.pt_src[3 * i + d];
  } else if (i - b.n_pt < b.n_seg) {
    const int k = i - b.n_pt;
    const long long at = b.seg_at[k];
#pragma unroll
    for (int d = 0; d < 3; ++d) { b.seg_spos[3 * at + d] = b.seg_ssrc[3 * k + d]; b.seg_epos[3 * at + d] = b.seg_esrc[3 * k + d]; }
  }
}

}  // namespace plsvo_hip
