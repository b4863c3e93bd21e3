// cms_stage.h -- CmsStage: the device block and the pinned block behind the host-buffer entries of the C-ABI ("lay out one block, one copy up,
// launches, one copy back, one wait").  Both grow on demand and never shrink.  Plain C++17 without a HIP include (tests/emu/stage_emu.cpp drives
// it with malloc and counters): memory, copies and the stream wait come from the policy M -- cms_api_util.h has the HIP one.
//   int M::take(void** p, size_t bytes, bool pinned)      allocate; 0 or the library's error code
//   int M::give(void* p, bool pinned)                     free
//   int M::wait(void* stream)                             until everything enqueued on the stream is through
//   int M::copy(void* dst, const void* src, size_t bytes, bool to_device, void* stream)      asynchronous, in stream order
//   int M::range_error(const char* who)                   the error code of a copy refused by up / back, its message naming the entry
#pragma once
#include <cstddef>
#include <cstdint>

template <class M> struct CmsStageT {
  uint8_t* d = nullptr; size_t d_bytes = 0;      // device block
  uint8_t* h = nullptr; size_t h_bytes = 0;      // pinned block

  // A block that is large enough is kept; one that is too small is replaced by need + need / 2 bytes, after the stream has been waited for (work
  // enqueued there may still use the old block).  Either size may be 0: a side nobody asks for is never allocated.  Pointers are taken AFTER this.
  int reserve(void* stream, size_t dev_bytes, size_t host_bytes) {
    const int rc = grow(stream, d, d_bytes, dev_bytes, false);
    return rc ? rc : grow(stream, h, h_bytes, host_bytes, true);
  }
  // h[0, bytes) -> d[0, bytes) and d[begin, end) -> h[begin, end): a range that either block does not hold is refused, whoever sized the blocks
  int up(void* stream, size_t bytes, const char* who) {
    if (bytes > d_bytes || bytes > h_bytes) return M::range_error(who);
    return bytes ? M::copy(d, h, bytes, true, stream) : 0;
  }
  int back(void* stream, size_t begin, size_t end, const char* who) {
    if (begin > end || end > d_bytes || end > h_bytes) return M::range_error(who);
    return end > begin ? M::copy(h + begin, d + begin, end - begin, false, stream) : 0;
  }
  int back_and_wait(void* stream, size_t begin, size_t end, const char* who) {
    const int rc = back(stream, begin, end, who);
    return rc ? rc : M::wait(stream);
  }
  void release() {      // (the owner's streams are idle: handles are destroyed between calls)
    if (d) (void)M::give(d, false);
    if (h) (void)M::give(h, true);
    d = h = nullptr; d_bytes = h_bytes = 0;
  }

 private:
  static int grow(void* stream, uint8_t*& p, size_t& have, size_t need, bool pinned) {
    if (need <= have) return 0;
    if (p) {
      int rc = M::wait(stream);
      if (rc) return rc;
      uint8_t* old = p;
      p = nullptr; have = 0;      // (zeroed before the new allocation: a failure leaves an empty block, not a dangling one)
      rc = M::give(old, pinned);
      if (rc) return rc;
    }
    const size_t want = need + need / 2;
    void* q = nullptr;
    const int rc = M::take(&q, want, pinned);
    if (rc) return rc;
    p = static_cast<uint8_t*>(q); have = want;
    return 0;
  }
};
