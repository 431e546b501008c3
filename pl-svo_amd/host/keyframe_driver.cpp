// keyframe_driver.cpp -- exercises the keyframe stage of the adapter (hip_adapter.hpp: frame_utils::getSceneDepth,
// keyframe::getCloseKeyframes / needNewKf / setKeyPoints) the way FrameHandlerMono::processFrame and Reprojector::reprojectMap use the
// reference's functions (src/frame_handler_mono.cpp:351-358, :396; src/reprojector.cpp:147-163): a frame and a few keyframes built from
// a binary dump written by tests/test_gpu_adapter_keyframe.py; the results are printed for the test to compare with the C ABI's.
// Usage: keyframe_driver <input.bin> <output.txt>
// Input (doubles): W H n_pt n_seg n_kf min_t min_r | fx fy cx cy | T_new[7] | T_last[7] | n_pt x (px py alive x y z) |
//                  n_seg x (alive sx sy sz ex ey ez) | n_kf x (T[7], 5 x (valid x y z)) | key_pts_prev[5]
#include <cstdio>
#include <cstdlib>
#include <list>
#include <memory>
#include <vector>

#include "plsvo/hip_adapter.hpp"
#include "plsvo/mini_types.hpp"

static std::vector<double> read_doubles(FILE* f, size_t n) { std::vector<double> v(n); if (n && fread(v.data(), 8, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } return v; }
static mini::SE3 pose(const double* T) { return mini::SE3(mini::Quat(T[3], T[0], T[1], T[2]), mini::Vec3(T[4], T[5], T[6])); }

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s in.bin out.txt\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror("open"); return 2; }
  std::vector<double> hdr = read_doubles(f, 7);
  const int n_pt = (int)hdr[2], n_seg = (int)hdr[3], n_kf = (int)hdr[4];
  mini::Camera cam;
  std::vector<double> c = read_doubles(f, 4);
  cam.fx_ = c[0]; cam.fy_ = c[1]; cam.cx_ = c[2]; cam.cy_ = c[3]; cam.w_ = (int)hdr[0]; cam.h_ = (int)hdr[1];
  std::vector<double> Tn = read_doubles(f, 7), Tl = read_doubles(f, 7);
  std::vector<double> pts = read_doubles(f, (size_t)n_pt * 6), segs = read_doubles(f, (size_t)n_seg * 7), kfs = read_doubles(f, (size_t)n_kf * 27);
  std::vector<double> prev = read_doubles(f, 5);
  fclose(f);

  mini::FramePtr frame(new mini::Frame()), last(new mini::Frame());
  frame->id_ = 100; frame->cam_ = &cam; frame->T_f_w_ = pose(Tn.data());
  last->id_ = 99; last->cam_ = &cam; last->T_f_w_ = pose(Tl.data());
  std::vector<mini::Point> points((size_t)n_pt);
  std::vector<mini::PointFeat> pfeat((size_t)n_pt);
  for (int i = 0; i < n_pt; ++i) {
    const double* p = &pts[(size_t)i * 6];
    points[(size_t)i].pos_ = mini::Vec3(p[3], p[4], p[5]);
    pfeat[(size_t)i].frame = frame.get(); pfeat[(size_t)i].px = mini::Vec2(p[0], p[1]);
    pfeat[(size_t)i].feat3D = p[2] != 0.0 ? &points[(size_t)i] : nullptr;
    frame->pt_fts_.push_back(&pfeat[(size_t)i]);
  }
  std::vector<mini::LineSeg> lines((size_t)n_seg);
  std::vector<mini::LineFeat> lfeat((size_t)n_seg);
  for (int i = 0; i < n_seg; ++i) {
    const double* p = &segs[(size_t)i * 7];
    lines[(size_t)i].spos_ = mini::Vec3(p[1], p[2], p[3]); lines[(size_t)i].epos_ = mini::Vec3(p[4], p[5], p[6]);
    lfeat[(size_t)i].frame = frame.get(); lfeat[(size_t)i].feat3D = p[0] != 0.0 ? &lines[(size_t)i] : nullptr;
    frame->seg_fts_.push_back(&lfeat[(size_t)i]);
  }
  for (int s = 0; s < 5; ++s) frame->key_pts_[(size_t)s] = prev[(size_t)s] >= 0 ? &pfeat[(size_t)prev[(size_t)s]] : nullptr;
  std::list<mini::FramePtr> keyframes;
  std::vector<mini::Point> kpoints((size_t)n_kf * 5);
  std::vector<mini::PointFeat> kfeat((size_t)n_kf * 5);
  for (int i = 0; i < n_kf; ++i) {
    const double* p = &kfs[(size_t)i * 27];
    mini::FramePtr kf(new mini::Frame());
    kf->id_ = i; kf->cam_ = &cam; kf->T_f_w_ = pose(p);
    for (int k = 0; k < 5; ++k) {
      const double* q = p + 7 + 4 * k;
      const size_t at = (size_t)i * 5 + (size_t)k;
      kpoints[at].pos_ = mini::Vec3(q[1], q[2], q[3]);
      kfeat[at].frame = kf.get(); kfeat[at].feat3D = &kpoints[at];
      kf->key_pts_[(size_t)k] = q[0] != 0.0 ? &kfeat[at] : nullptr;
    }
    keyframes.push_back(kf);
  }

  FILE* o = fopen(argv[2], "w");
  if (!o) { perror("open"); return 2; }
  double depth_mean = -1.0, depth_min = -1.0;
  const bool has = plsvo::frame_utils::getSceneDepth(*frame, depth_mean, depth_min);
  fprintf(o, "depth %d %.17g %.17g\n", has ? 1 : 0, depth_mean, depth_min);
  std::list<std::pair<mini::FramePtr, double> > close_kfs;
  if (!plsvo::keyframe::getCloseKeyframes(frame, keyframes, close_kfs)) return 3;
  for (auto it = close_kfs.begin(); it != close_kfs.end(); ++it) fprintf(o, "close %d %.17g\n", it->first->id_, it->second);
  fprintf(o, "need %d\n", plsvo::keyframe::needNewKf(last, close_kfs, hdr[5], hdr[6]) ? 1 : 0);
  std::list<std::pair<mini::FramePtr, double> > none;
  fprintf(o, "need_empty %d\n", plsvo::keyframe::needNewKf(last, none, hdr[5], hdr[6]) ? 1 : 0);
  if (!plsvo::keyframe::setKeyPoints(*frame)) return 3;
  fprintf(o, "keypts");
  for (int s = 0; s < 5; ++s) fprintf(o, " %d", frame->key_pts_[(size_t)s] ? (int)(frame->key_pts_[(size_t)s] - pfeat.data()) : -1);
  fprintf(o, "\n");
  fclose(o);
  return 0;
}
