// capi_transfer.hpp -- the ONE staging path and the ONE readback path of the C ABI's host layer, over plsvo_ctx*.  Included by capi_ctx.hpp
// behind the definition of plsvo_ctx (which holds the pinned buffers); internal, header only.
//   staging:  Blob (host sections, 256-byte aligned) -> upload_blob (one host-to-device copy) ; Carver lays out the device-side outputs
//   readback: Readback (add ranges, wait once, read typed views)
#pragma once

// All input arrays of a batch travel as ONE host-to-device copy: sections of a single blob, each 256-byte aligned.
// (A single-frame call used to pay a dozen small pageable copies; small blobs go through a pinned staging buffer.)
struct PLSVO_LOCAL Blob {
  std::vector<uint8_t> host;
  // a section of n elements to be filled in place: take the pointers (at<T>) only after the LAST reserve / add, which may move the blob
  template <typename T> size_t reserve(size_t n) {
    const size_t off = (host.size() + 255) & ~(size_t)255;
    host.resize(off + std::max(n * sizeof(T), (size_t)16));
    return off;
  }
  // a section holding p[0 .. n), or n zero elements when p is NULL (an optional array the kernel still indexes)
  template <typename T> size_t add(const T* p, size_t n) {
    const size_t off = reserve<T>(n);
    if (p && n) memcpy(host.data() + off, p, n * sizeof(T));
    return off;
  }
  template <typename T> size_t add(const std::vector<T>& v) { return add(v.data(), v.size()); }
  template <typename T> T* at(size_t off) { return reinterpret_cast<T*>(host.data() + off); }                                              // host view of a section
  template <typename T> static const T* dev(const DevBuf& buf, size_t off) { return reinterpret_cast<const T*>(buf.as<uint8_t>() + off); }   // device view, once uploaded into buf
};

// carve typed arrays out of one device allocation (256-byte aligned sections)
struct PLSVO_LOCAL Carver {
  size_t off = 0;
  template <typename T> size_t take(size_t n) { const size_t o = (off + 255) & ~(size_t)255; off = o + std::max(n, (size_t)1) * sizeof(T); return o; }
  template <typename T> static T* dev(const DevBuf& buf, size_t o) { return reinterpret_cast<T*>(buf.as<uint8_t>() + o); }
};

static const size_t kPinnedMax = (size_t)8 << 20;   // blobs up to 8 MB (hundreds of frames) bounce through pinned memory
static inline int upload_blob(plsvo_ctx* c, DevBuf& buf, const Blob& blob) {
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

// Any number of device ranges to the host with ONE wait: add() them, wait(), then read at<T>(k) -- range k's bytes, a 64-byte-aligned
// section of the context's pinned download buffer when the total is at most 4 MB (a per-frame caller's results: device-to-PAGEABLE
// copies are staged and waited for one by one by the driver), of `fallback` otherwise or when no pinned memory is to be had.  `fallback`
// is sized HERE, so the decision and the storage can never disagree.  The pinned views hold until the context's next wait(): consume them
// before the same function or a callee fetches again.  at(k) of a range that was not added throws (std::vector::at).
struct PLSVO_LOCAL Readback {
  struct Range { const void* src; size_t bytes, off; };
  std::vector<Range> ranges;
  std::vector<uint8_t> fallback;
  size_t total = 0;
  const uint8_t* base = nullptr;
  int add(const void* src, size_t bytes) { ranges.push_back({ src, bytes, total }); total += (bytes + 63) & ~(size_t)63; return (int)ranges.size() - 1; }
  int wait(plsvo_ctx* c) {
    bool pinned = total <= ((size_t)4 << 20);
    if (pinned && c->dl_pinned_cap < total) {
      if (c->dl_pinned) (void)hipHostFree(c->dl_pinned);
      c->dl_pinned = nullptr; c->dl_pinned_cap = 0;
      const size_t want = std::max(total * 2, (size_t)64 << 10);
      if (hipHostMalloc(&c->dl_pinned, want, hipHostMallocDefault) == hipSuccess) c->dl_pinned_cap = want; else { c->dl_pinned = nullptr; pinned = false; }
    }
    if (!pinned) fallback.resize(std::max(total, (size_t)64));
    uint8_t* const to = pinned ? static_cast<uint8_t*>(c->dl_pinned) : fallback.data();
    base = to;
    for (const Range& r : ranges)
      if (r.bytes) HIP_TRY(c, hipMemcpyAsync(to + r.off, r.src, r.bytes, hipMemcpyDeviceToHost, c->stream));   // (zero-length ranges are skipped)
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return PLSVO_OK;
  }
  template <typename T> const T* at(int k) const { return reinterpret_cast<const T*>(base + ranges.at((size_t)k).off); }
};
