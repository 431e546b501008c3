// Stand-alone harness for pl-svo_amd/csrc/capi_transfer.hpp -- the staging and readback path of the C ABI's host layer -- on a plain
// plsvo_ctx object against the emulated runtime (tests/host/emu: device memory is host memory, a copy is a memmove).  Built as host
// code under AddressSanitizer and UBSan by tests/test_capi_transfer_host.py: every offset and size below is checked against the real allocations.
// Prints "<checks> <failures>"; exit status 0 when no check failed.
#define __HIPCC__ 1   // the emulated runtime's device language, as tests/host/build_emu.sh sets it: this is a plain host program
#include <cstdint>
#include <cstdio>
#include <stdexcept>

#include "capi_ctx.hpp"

static int g_checks = 0, g_bad = 0;
#define CHECK(cond) do { ++g_checks; if (!(cond)) { ++g_bad; fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } } while (0)

static std::vector<uint8_t> pattern(size_t n, unsigned seed) {
  std::vector<uint8_t> v(n);
  unsigned x = seed * 2654435761u + 12345u;
  for (size_t i = 0; i < n; ++i) { x = x * 1664525u + 1013904223u; v[i] = (uint8_t)(x >> 24); }
  return v;
}

static void test_blob_add() {
  Blob b;
  const double d3[3] = { 1.5, -2.25, 3.0 };
  const uint8_t odd[7] = { 1, 2, 3, 4, 5, 6, 7 };
  const std::vector<uint8_t> big = pattern(257, 1);
  const std::vector<int> iv = { 7, 8, 9 };
  const size_t o_d = b.add(d3, (size_t)3);
  const size_t o_null = b.add(static_cast<const double*>(nullptr), (size_t)5);   // no array given: zeros
  const size_t o_empty = b.add(static_cast<const int*>(nullptr), (size_t)0);      // nothing at all: the 16-byte minimum section
  const size_t o_odd = b.add(odd, sizeof(odd));
  const size_t o_big = b.add(big.data(), big.size());                            // 257 bytes: the next section starts two alignment steps on
  const size_t o_vec = b.add(iv);
  const size_t o_res = b.reserve<float>(3);
  const size_t offs[7] = { o_d, o_null, o_empty, o_odd, o_big, o_vec, o_res };
  for (size_t o : offs) CHECK(o % 256 == 0);
  for (int k = 1; k < 7; ++k) CHECK(offs[k] > offs[k - 1]);
  CHECK(o_d == 0 && o_null == 256 && o_empty == 512 && o_odd == 768 && o_big == 1024 && o_vec == 1536 && o_res == 1792);
  CHECK(b.host.size() == o_res + 16);                                           // 3 floats: the 16-byte minimum
  // (the views are taken after the last add: the blob has stopped moving)
  CHECK(memcmp(b.at<double>(o_d), d3, sizeof(d3)) == 0);
  for (int k = 0; k < 5; ++k) CHECK(b.at<double>(o_null)[k] == 0.0);
  for (int k = 0; k < 16; ++k) CHECK(b.at<uint8_t>(o_empty)[k] == 0);
  CHECK(memcmp(b.at<uint8_t>(o_odd), odd, sizeof(odd)) == 0 && b.at<uint8_t>(o_odd)[7] == 0);
  CHECK(memcmp(b.at<uint8_t>(o_big), big.data(), big.size()) == 0);
  CHECK(memcmp(b.at<int>(o_vec), iv.data(), iv.size() * sizeof(int)) == 0);
  Blob last;   // a blob whose last section is the minimum one ends 16 bytes behind its offset
  last.add(odd, sizeof(odd));
  CHECK(last.add(static_cast<const float*>(nullptr), (size_t)0) == 256 && last.host.size() == 272);
  Carver cv;
  CHECK(cv.take<double>(3) == 0 && cv.take<uint8_t>(0) == 256 && cv.take<int>(65) == 512 && cv.off == 512 + 65 * sizeof(int));
}

static void test_upload_blob(plsvo_ctx* c) {
  DevBuf buf;
  Blob empty;
  CHECK(upload_blob(c, buf, empty) == PLSVO_OK && buf.p && buf.cap >= 256);
  CHECK(c->pinned_next == 0 && !c->pinned[0] && !c->pinned[1]);                   // nothing travelled
  // blobs of growing size in a row: the two pinned buffers are used in turn, and each is regrown when it comes up again too small
  const size_t sizes[4] = { 1000, (size_t)3 << 19, (size_t)3 << 20, (size_t)4 << 20 };
  size_t cap_seen[4] = { 0, 0, 0, 0 };
  for (int k = 0; k < 4; ++k) {
    Blob b;
    const std::vector<uint8_t> src = pattern(sizes[k], 10 + (unsigned)k);
    const size_t o0 = b.add(src.data(), src.size() / 2), o1 = b.add(src.data() + src.size() / 2, src.size() - src.size() / 2);
    const int slot = c->pinned_next;
    CHECK(slot == (k & 1));
    CHECK(upload_blob(c, buf, b) == PLSVO_OK);
    CHECK(c->pinned_next == (slot ^ 1) && c->pinned[slot] && c->pinned_cap[slot] >= b.host.size() && c->pinned_done[slot]);
    cap_seen[k] = c->pinned_cap[slot];
    CHECK(buf.cap >= b.host.size() && memcmp(buf.p, b.host.data(), b.host.size()) == 0);
    CHECK(memcmp(Blob::dev<uint8_t>(buf, o0), src.data(), src.size() / 2) == 0);
    CHECK(memcmp(Blob::dev<uint8_t>(buf, o1), src.data() + src.size() / 2, src.size() - src.size() / 2) == 0);
  }
  CHECK(cap_seen[0] == ((size_t)1 << 20) && cap_seen[1] == 2 * sizes[1] && cap_seen[2] == 2 * sizes[2] && cap_seen[3] == 2 * sizes[3]);   // 1 MB at least, else twice the blob
  // just over 8 MB: straight from the blob, no pinned buffer is touched
  {
    Blob b;
    const std::vector<uint8_t> src = pattern(((size_t)8 << 20) + 1, 99);
    b.add(src.data(), src.size());
    const int slot = c->pinned_next;
    const size_t cap0 = c->pinned_cap[0], cap1 = c->pinned_cap[1];
    CHECK(upload_blob(c, buf, b) == PLSVO_OK);
    CHECK(c->pinned_next == slot && c->pinned_cap[0] == cap0 && c->pinned_cap[1] == cap1);
    CHECK(buf.cap >= b.host.size() && memcmp(buf.p, b.host.data(), b.host.size()) == 0);
  }
  buf.release();
}

// n ranges of the given sizes out of one device buffer each; every view must hold its source's bytes at a 64-byte-aligned offset
static void readback_case(plsvo_ctx* c, const std::vector<size_t>& bytes, bool expect_pinned) {
  std::vector<DevBuf> dev(bytes.size());
  std::vector<std::vector<uint8_t>> src(bytes.size());
  Readback rb;
  size_t total = 0;
  for (size_t k = 0; k < bytes.size(); ++k) {
    src[k] = pattern(bytes[k], 1000 + (unsigned)k);
    CHECK(dev[k].ensure(bytes[k]) == hipSuccess);
    if (bytes[k]) memcpy(dev[k].p, src[k].data(), bytes[k]);
    CHECK(rb.add(bytes[k] ? dev[k].p : nullptr, bytes[k]) == (int)k);     // (a zero-length range may have no source at all)
    total += (bytes[k] + 63) & ~(size_t)63;
  }
  CHECK(rb.total == total);
  CHECK(rb.wait(c) == PLSVO_OK);
  if (expect_pinned) {
    CHECK(rb.base == c->dl_pinned && rb.fallback.empty() && c->dl_pinned_cap >= total);
  } else {
    CHECK(rb.base == rb.fallback.data() && rb.fallback.size() == std::max(total, (size_t)64));   // sized by the helper
  }
  for (size_t k = 0; k < bytes.size(); ++k) {
    const uint8_t* h = rb.at<uint8_t>((int)k);
    CHECK((size_t)(h - rb.base) % 64 == 0 && (size_t)(h - rb.base) + bytes[k] <= std::max(total, (size_t)64));
    CHECK(bytes[k] == 0 || memcmp(h, src[k].data(), bytes[k]) == 0);
  }
  bool threw = false;   // no view of a range that was not added
  try { (void)rb.at<uint8_t>((int)bytes.size()); } catch (const std::out_of_range&) { threw = true; }
  CHECK(threw);
  for (DevBuf& d : dev) d.release();
}

static void test_readback(plsvo_ctx* c) {
  readback_case(c, { 100 }, true);
  CHECK(c->dl_pinned_cap == ((size_t)64 << 10));                                  // the first buffer: the 64 KB minimum
  readback_case(c, { 0, 7, 64, 0 }, true);
  readback_case(c, { 9000, 0, 1, 63, 65, 0, 128, 40000, 5 }, true);
  CHECK(c->dl_pinned_cap == ((size_t)64 << 10));
  readback_case(c, { 70000, 3 }, true);                                           // larger than the buffer: regrown to twice the total
  CHECK(c->dl_pinned_cap == 2 * (70016 + 64));
  readback_case(c, { ((size_t)4 << 20) - 64, 1 }, true);                          // exactly 4 MB of sections: still pinned
  CHECK(c->dl_pinned_cap == ((size_t)8 << 20));
  readback_case(c, { ((size_t)4 << 20) - 64, 65 }, false);                        // 64 bytes more: the fallback vector
  readback_case(c, { ((size_t)4 << 20) + 1 }, false);
  readback_case(c, { 0 }, true);                                                  // nothing to copy: a wait and a valid (empty) view
  Readback none;
  CHECK(none.wait(c) == PLSVO_OK);
}

int main() {
  plsvo_ctx ctx;
  test_blob_add();
  test_upload_blob(&ctx);
  test_readback(&ctx);
  for (int k = 0; k < 2; ++k) { if (ctx.pinned[k]) (void)hipHostFree(ctx.pinned[k]); if (ctx.pinned_done[k]) (void)hipEventDestroy(ctx.pinned_done[k]); }
  if (ctx.dl_pinned) (void)hipHostFree(ctx.dl_pinned);
  printf("%d %d\n", g_checks, g_bad);
  return g_bad == 0 ? 0 : 1;
}
