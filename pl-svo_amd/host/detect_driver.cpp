// detect_driver.cpp -- exercises plsvo::feature_detection::FastDetector (hip_adapter.hpp) the way DepthFilter::initializeSeeds uses it
// (src/depth_filter.cpp:161-165): a frame built from a binary dump written by tests/test_gpu_adapter_detect.py, one detection on an
// empty grid, one after setExistingFeatures on a list of existing features, one after a single setGridOccpuancy; the feature lists are
// printed for the test to compare with the C ABI's result.  The detector resets its grid after every detect, as the reference does.
// Usage: detect_driver <input.bin> <output.txt>
#include <cstdio>
#include <cstdlib>
#include <list>
#include <vector>

#include "plsvo/hip_adapter.hpp"
#include "plsvo/mini_types.hpp"

static std::vector<double> read_doubles(FILE* f, size_t n) { std::vector<double> v(n); if (n && fread(v.data(), 8, n, f) != n) { fprintf(stderr, "short read\n"); exit(2); } return v; }

static void print_and_free(FILE* o, const char* tag, std::list<mini::PointFeat*>& fts, const mini::Frame* frame) {
  for (mini::PointFeat* ft : fts) {
    fprintf(o, "%s %.17g %.17g %d %.17g %.17g %.17g %d\n", tag, ft->px[0], ft->px[1], ft->level, ft->f[0], ft->f[1], ft->f[2], ft->frame == frame ? 1 : 0);
    delete ft;
  }
  fts.clear();
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s in.bin out.txt\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror("open"); return 2; }
  std::vector<double> hdr = read_doubles(f, 7);
  const int W = (int)hdr[0], H = (int)hdr[1], n_levels = (int)hdr[2], n_pyr_levels = (int)hdr[3], cell = (int)hdr[4], n_existing = (int)hdr[6];
  const double threshold = hdr[5];
  mini::Camera cam;
  std::vector<double> c = read_doubles(f, 4);
  cam.fx_ = c[0]; cam.fy_ = c[1]; cam.cx_ = c[2]; cam.cy_ = c[3]; cam.w_ = W; cam.h_ = H;
  mini::Frame frame;
  frame.id_ = 20; frame.cam_ = &cam;
  frame.img_pyr_.resize((size_t)n_levels);
  for (int l = 0; l < n_levels; ++l) {
    frame.img_pyr_[(size_t)l].alloc(W >> l, H >> l);
    const size_t nb = (size_t)(W >> l) * (H >> l);
    if (fread(frame.img_pyr_[(size_t)l].data, 1, nb, f) != nb) { fprintf(stderr, "short image read\n"); return 2; }
  }
  std::vector<double> ex = read_doubles(f, (size_t)n_existing * 2);
  fclose(f);
  std::vector<mini::PointFeat> existing((size_t)n_existing);
  for (int i = 0; i < n_existing; ++i) {
    existing[(size_t)i].frame = &frame; existing[(size_t)i].px = mini::Vec2(ex[(size_t)i * 2], ex[(size_t)i * 2 + 1]);
    frame.pt_fts_.push_back(&existing[(size_t)i]);
  }
  FILE* o = fopen(argv[2], "w");
  if (!o) { perror("open"); return 2; }
  plsvo::feature_detection::FastDetector detector(W, H, cell, n_pyr_levels);
  fprintf(o, "grid %d %d\n", detector.grid_n_cols(), detector.grid_n_rows());
  std::list<mini::PointFeat*> fts;
  detector.detect(&frame, frame.img_pyr_, threshold, fts);
  if (!detector.ok()) { fprintf(stderr, "FastDetector::detect failed\n"); return 3; }
  print_and_free(o, "free", fts, &frame);
  detector.setExistingFeatures(frame.pt_fts_);
  detector.detect(&frame, frame.img_pyr_, threshold, fts);
  if (!detector.ok()) return 3;
  print_and_free(o, "existing", fts, &frame);
  if (n_existing > 0) detector.setGridOccpuancy(existing[0]);
  detector.detect(&frame, frame.img_pyr_, threshold, fts);
  if (!detector.ok()) return 3;
  print_and_free(o, "one", fts, &frame);
  detector.detect(&frame, frame.img_pyr_, threshold, fts);     // the grid was reset: the same as the first list
  if (!detector.ok()) return 3;
  print_and_free(o, "reset", fts, &frame);
  fclose(o);
  return 0;
}
