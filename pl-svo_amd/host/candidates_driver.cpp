// candidates_driver.cpp -- exercises plsvo::reprojector::mapCandidates (hip_adapter.hpp) the way Reprojector::reprojectMap builds its
// candidate set (src/reprojector.cpp:157-183), and compares it with a host loop written in the reference's form: the lists walked in
// order, a last_projected_kf_id_ mark per landmark, reproject() per landmark, getCloseViewObs per filed landmark
// (src/feature3D.cpp:80-125), a stable sort by descending type_.  A map is built from a binary dump written by
// tests/test_gpu_adapter_candidates.py; the adapter's result is printed for the test, a disagreement with the host loop is exit code 4.
// The host loop is independent of the kernel in CONTROL FLOW only: it transforms and inverts poses with plsvo_math.hpp's se3_act /
// se3_inv, the helpers the kernel uses, so it is no arithmetic oracle.  The arithmetic is checked by the test, which compares what this
// program prints with tests/np_candidates.py (numpy, float64, shares no code with the library).
// Usage: candidates_driver <input.bin> <output.txt>
// Input (doubles): W H fx fy cx cy cell seg_cell frame_id n_kf n_pt n_seg n_ptc n_segc n_ov | T[7] | overlap[n_ov] |
//   n_pt x (pos[3] type n_obs, n_obs x (kf px[2] f[3] level type grad[2])) | n_seg x (spos[3] epos[3] type n_obs, n_obs x (kf spx[2] epx[2]
//   sf[3] ef[3] level)) | n_kf x (T[7] n_pf n_sf, n_pf x lm, n_sf x lm) | pt_cand[n_ptc] | seg_cand[n_segc]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <memory>
#include <vector>

#include "plsvo/hip_adapter.hpp"
#include "plsvo/mini_types.hpp"

namespace ph = plsvo_hip;
typedef plsvo::reprojector::MapCandidate<mini::Point, mini::PointFeat> PtCand;
typedef plsvo::reprojector::MapCandidate<mini::LineSeg, mini::LineFeat> SegCand;

static mini::SE3 pose(const double* T) { return mini::SE3(mini::Quat(T[3], T[0], T[1], T[2]), mini::Vec3(T[4], T[5], T[6])); }
static ph::SE3d se3(const mini::SE3& T) { double v[7] = { T.q.x(), T.q.y(), T.q.z(), T.q.w(), T.t[0], T.t[1], T.t[2] }; return ph::se3_load(v); }

// Reprojector::reproject for one position (:389-423): world2cam(T * pos), isInFrame(px.cast<int>(), 8), the cell
static int reproject(const mini::Frame& fr, const mini::Vec3& pos, int cell_size, double* px) {
  double c[3];
  ph::se3_act(se3(fr.T_f_w_), pos.v, c);
  px[0] = fr.cam_->fx() * (c[0] / c[2]) + fr.cam_->cx(); px[1] = fr.cam_->fy() * (c[1] / c[2]) + fr.cam_->cy();
  if (!(px[0] == px[0] && px[1] == px[1] && std::fabs(px[0]) < 1e9 && std::fabs(px[1]) < 1e9)) return -1;
  const int ox = (int)px[0], oy = (int)px[1];
  if (!(ox >= 8 && ox < fr.cam_->width() - 8 && oy >= 8 && oy < fr.cam_->height() - 8)) return -1;
  return (int)(px[1] / cell_size) * ((fr.cam_->width() + cell_size - 1) / cell_size) + (int)(px[0] / cell_size);
}
static void frame_pos(const mini::Frame& fr, double* p) { const ph::SE3d Ti = ph::se3_inv(se3(fr.T_f_w_)); p[0] = Ti.t[0]; p[1] = Ti.t[1]; p[2] = Ti.t[2]; }
static void normalize3(double* v) { const double n = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); v[0] /= n; v[1] /= n; v[2] /= n; }
// getCloseViewObs (src/feature3D.cpp:80-125); an empty list: no observation, no view
template <class FeatT>
static bool close_view_obs(const double* framepos, const double* pos, const std::list<FeatT*>& obs, FeatT*& ftr) {
  ftr = nullptr;
  if (obs.empty()) return false;
  double obs_dir[3] = { framepos[0] - pos[0], framepos[1] - pos[1], framepos[2] - pos[2] };
  normalize3(obs_dir);
  auto min_it = obs.begin();
  double min_cos_angle = 0;
  for (auto it = obs.begin(), ite = obs.end(); it != ite; ++it) {
    double kp[3]; frame_pos(*(*it)->frame, kp);
    double dir[3] = { kp[0] - pos[0], kp[1] - pos[1], kp[2] - pos[2] };
    normalize3(dir);
    const double cos_angle = (obs_dir[0] * dir[0] + obs_dir[1] * dir[1]) + obs_dir[2] * dir[2];
    if (cos_angle > min_cos_angle) { min_cos_angle = cos_angle; min_it = it; }
  }
  ftr = *min_it;
  return !(min_cos_angle < 0.5);
}

struct Rd {
  std::vector<double> v; size_t at = 0;
  double d() { if (at >= v.size()) { fprintf(stderr, "short input\n"); exit(2); } return v[at++]; }
  int i() { return (int)d(); }
  void vec(double* o, int n) { for (int k = 0; k < n; ++k) o[k] = d(); }
};

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s in.bin out.txt\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror("open"); return 2; }
  Rd r;
  { fseek(f, 0, SEEK_END); const long n = ftell(f); fseek(f, 0, SEEK_SET); r.v.resize((size_t)n / 8); if (fread(r.v.data(), 8, r.v.size(), f) != r.v.size()) return 2; fclose(f); }
  mini::Camera cam;
  cam.w_ = r.i(); cam.h_ = r.i(); cam.fx_ = r.d(); cam.fy_ = r.d(); cam.cx_ = r.d(); cam.cy_ = r.d();
  const int cell = r.i(), seg_cell = r.i(), frame_id = r.i(), n_kf = r.i(), n_pt = r.i(), n_seg = r.i(), n_ptc = r.i(), n_segc = r.i(), n_ov = r.i();
  double T[7]; r.vec(T, 7);
  mini::FramePtr frame(new mini::Frame());
  frame->id_ = frame_id; frame->cam_ = &cam; frame->T_f_w_ = pose(T);
  std::vector<int> ov((size_t)n_ov);
  for (int k = 0; k < n_ov; ++k) ov[(size_t)k] = r.i();
  std::vector<mini::FramePtr> kfs;
  for (int k = 0; k < n_kf; ++k) { kfs.push_back(mini::FramePtr(new mini::Frame())); kfs.back()->id_ = k; kfs.back()->cam_ = &cam; }
  std::vector<mini::Point> points((size_t)n_pt);
  std::vector<mini::LineSeg> lines((size_t)n_seg);
  std::list<mini::PointFeat> pfeat;      // (lists: the addresses stay put)
  std::list<mini::LineFeat> lfeat;
  for (int i = 0; i < n_pt; ++i) {
    mini::Point& p = points[(size_t)i];
    r.vec(p.pos_.v, 3); p.type_ = r.i();
    const int n_obs = r.i();
    for (int o = 0; o < n_obs; ++o) {
      pfeat.push_back(mini::PointFeat());
      mini::PointFeat& ft = pfeat.back();
      ft.frame = kfs[(size_t)r.i()].get(); r.vec(ft.px.v, 2); r.vec(ft.f.v, 3); ft.level = r.i();
      ft.type = r.i() ? mini::PointFeat::EDGELET : mini::PointFeat::CORNER; r.vec(ft.grad.v, 2); ft.feat3D = &p;
      p.obs_.push_back(&ft);
    }
  }
  for (int i = 0; i < n_seg; ++i) {
    mini::LineSeg& s = lines[(size_t)i];
    r.vec(s.spos_.v, 3); r.vec(s.epos_.v, 3); s.type_ = r.i();
    const int n_obs = r.i();
    for (int o = 0; o < n_obs; ++o) {
      lfeat.push_back(mini::LineFeat());
      mini::LineFeat& ft = lfeat.back();
      ft.frame = kfs[(size_t)r.i()].get(); r.vec(ft.spx.v, 2); r.vec(ft.epx.v, 2); r.vec(ft.sf.v, 3); r.vec(ft.ef.v, 3); ft.level = r.i(); ft.feat3D = &s;
      s.obs_.push_back(&ft);
    }
  }
  // the keyframes' own feature lists: features of their own (the observation lists above are what getCloseViewObs walks)
  for (int k = 0; k < n_kf; ++k) {
    r.vec(T, 7); kfs[(size_t)k]->T_f_w_ = pose(T);
    const int n_pf = r.i(), n_sf = r.i();
    for (int j = 0; j < n_pf; ++j) { const int lm = r.i(); pfeat.push_back(mini::PointFeat()); pfeat.back().frame = kfs[(size_t)k].get(); pfeat.back().feat3D = lm >= 0 ? &points[(size_t)lm] : nullptr; kfs[(size_t)k]->pt_fts_.push_back(&pfeat.back()); }
    for (int j = 0; j < n_sf; ++j) { const int lm = r.i(); lfeat.push_back(mini::LineFeat()); lfeat.back().frame = kfs[(size_t)k].get(); lfeat.back().feat3D = lm >= 0 ? &lines[(size_t)lm] : nullptr; kfs[(size_t)k]->seg_fts_.push_back(&lfeat.back()); }
  }
  std::list<mini::Point*> pt_cand;
  std::list<mini::LineSeg*> seg_cand;
  for (int k = 0; k < n_ptc; ++k) pt_cand.push_back(&points[(size_t)r.i()]);
  for (int k = 0; k < n_segc; ++k) seg_cand.push_back(&lines[(size_t)r.i()]);
  std::list<mini::FramePtr> keyframes(kfs.begin(), kfs.end());
  std::vector<std::pair<mini::FramePtr, size_t> > overlap_kfs, overlap_ref;
  for (int k = 0; k < n_ov; ++k) { overlap_kfs.push_back(std::make_pair(kfs[(size_t)ov[(size_t)k]], (size_t)0)); overlap_ref.push_back(overlap_kfs.back()); }

  // ---- the adapter ----
  std::vector<PtCand> pts;
  std::vector<SegCand> segs;
  std::vector<uint8_t> pfail, sfail;
  if (!plsvo::reprojector::mapCandidates(frame, keyframes, overlap_kfs, pt_cand, seg_cand, cell, seg_cell, pts, segs, &pfail, &sfail)) return 3;
  std::vector<int> marks_pt, marks_seg;
  for (auto& p : points) { marks_pt.push_back(p.last_projected_kf_id_); p.last_projected_kf_id_ = -1; }
  for (auto& s : lines) { marks_seg.push_back(s.last_projected_kf_id_); s.last_projected_kf_id_ = -1; }

  // ---- the same in the reference's form ----
  std::vector<PtCand> rpts;
  std::vector<SegCand> rsegs;
  auto reproject_pt = [&](mini::Point* p) { PtCand c; c.feat3D = p; c.cell[0] = reproject(*frame, p->pos_, cell, c.px); if (c.cell[0] < 0) return false; rpts.push_back(c); return true; };
  auto reproject_seg = [&](mini::LineSeg* s) {
    SegCand c; c.feat3D = s; c.cell[0] = reproject(*frame, s->spos_, seg_cell, c.px); c.cell[1] = reproject(*frame, s->epos_, seg_cell, c.px + 2);
    if (c.cell[0] < 0 || c.cell[1] < 0) return false;
    rsegs.push_back(c); return true; };
  for (auto& okf : overlap_ref) {
    for (auto it = okf.first->pt_fts_.begin(); it != okf.first->pt_fts_.end(); ++it) {
      if ((*it)->feat3D == NULL) continue;
      if ((*it)->feat3D->last_projected_kf_id_ == frame->id_) continue;
      (*it)->feat3D->last_projected_kf_id_ = frame->id_;
      if (reproject_pt((*it)->feat3D)) okf.second++;
    }
    for (auto it = okf.first->seg_fts_.begin(); it != okf.first->seg_fts_.end(); ++it) {
      if ((*it)->feat3D == NULL) continue;
      if ((*it)->feat3D->last_projected_kf_id_ == frame->id_) continue;
      (*it)->feat3D->last_projected_kf_id_ = frame->id_;
      if (reproject_seg((*it)->feat3D)) okf.second++;
    }
  }
  std::vector<uint8_t> rpfail, rsfail;
  for (auto p : pt_cand) rpfail.push_back(reproject_pt(p) ? 0 : 1);
  for (auto s : seg_cand) rsfail.push_back(reproject_seg(s) ? 0 : 1);
  double fp[3]; frame_pos(*frame, fp);
  for (auto& c : rpts) { c.has_view = close_view_obs(fp, c.feat3D->pos_.v, c.feat3D->obs_, c.ref_ftr); c.active = c.has_view && c.feat3D->type_ != mini::TYPE_DELETED; }
  for (auto& c : rsegs) {
    double cpos[3];
    for (int k = 0; k < 3; ++k) cpos[k] = 0.5 * (c.feat3D->spos_[k] + c.feat3D->epos_[k]);
    c.has_view = close_view_obs(fp, cpos, c.feat3D->obs_, c.ref_ftr); c.active = c.has_view && c.feat3D->type_ != mini::TYPE_DELETED;
  }
  std::stable_sort(rpts.begin(), rpts.end(), [](const PtCand& a, const PtCand& b) { return a.feat3D->type_ > b.feat3D->type_; });
  std::stable_sort(rsegs.begin(), rsegs.end(), [](const SegCand& a, const SegCand& b) { return a.feat3D->type_ > b.feat3D->type_; });

  // ---- compare, print ----
  int bad = 0;
  if (pts.size() != rpts.size() || segs.size() != rsegs.size() || pfail != rpfail || sfail != rsfail) bad = 1;
  for (size_t i = 0; !bad && i < pts.size(); ++i)
    if (pts[i].feat3D != rpts[i].feat3D || memcmp(pts[i].px, rpts[i].px, 16) || pts[i].cell[0] != rpts[i].cell[0] || pts[i].ref_ftr != rpts[i].ref_ftr ||
        pts[i].has_view != rpts[i].has_view || pts[i].active != rpts[i].active) bad = 1;
  for (size_t i = 0; !bad && i < segs.size(); ++i)
    if (segs[i].feat3D != rsegs[i].feat3D || memcmp(segs[i].px, rsegs[i].px, 32) || segs[i].cell[0] != rsegs[i].cell[0] || segs[i].cell[1] != rsegs[i].cell[1] ||
        segs[i].ref_ftr != rsegs[i].ref_ftr || segs[i].has_view != rsegs[i].has_view || segs[i].active != rsegs[i].active) bad = 1;
  for (size_t k = 0; k < overlap_kfs.size(); ++k) if (overlap_kfs[k].second != overlap_ref[k].second) bad = 1;
  for (size_t i = 0; i < points.size(); ++i) if (marks_pt[i] != points[i].last_projected_kf_id_) bad = 1;
  for (size_t i = 0; i < lines.size(); ++i) if (marks_seg[i] != lines[i].last_projected_kf_id_) bad = 1;
  FILE* o = fopen(argv[2], "w");
  if (!o) { perror("open"); return 2; }
  for (auto& c : pts) fprintf(o, "pt %d %.17g %.17g %d %d %d %d\n", (int)(c.feat3D - points.data()), c.px[0], c.px[1], c.cell[0], c.ref_ftr ? c.ref_ftr->frame->id_ : -1, c.has_view ? 1 : 0, c.active ? 1 : 0);
  for (auto& c : segs) fprintf(o, "seg %d %.17g %.17g %.17g %.17g %d %d %d %d %d\n", (int)(c.feat3D - lines.data()), c.px[0], c.px[1], c.px[2], c.px[3], c.cell[0], c.cell[1], c.ref_ftr ? c.ref_ftr->frame->id_ : -1, c.has_view ? 1 : 0, c.active ? 1 : 0);
  fprintf(o, "count"); for (auto& k : overlap_kfs) fprintf(o, " %d", (int)k.second); fprintf(o, "\n");
  fprintf(o, "pfail"); for (auto v : pfail) fprintf(o, " %d", (int)v); fprintf(o, "\n");
  fprintf(o, "sfail"); for (auto v : sfail) fprintf(o, " %d", (int)v); fprintf(o, "\n");
  fprintf(o, "marks"); for (auto v : marks_pt) fprintf(o, " %d", v); fprintf(o, "\n");
  fprintf(o, "agree %d\n", bad ? 0 : 1);
  fclose(o);
  return bad ? 4 : 0;
}
