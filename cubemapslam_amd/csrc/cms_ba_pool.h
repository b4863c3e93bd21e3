// cms_ba_pool.h -- the per-device caches behind the local-BA host code's streams, events, device slabs and pinned blocks: what a destroyed
// window leaves for the next one.  Plain C++17 without a HIP include (tests/emu/ba_pool_emu.cpp compiles it alone): both types only answer
// "nothing cached" / "cache full" and never create or destroy a resource -- cms_api_ba.hip does that, outside their locks.  They are the one
// piece of the library every host thread of every rank runs concurrently (the cms-ba-plan workers, the group threads, the frame thread).
#pragma once
#include <cstddef>
#include <mutex>
#include <vector>

#define BA_POOL_DEVICES 64      // devices 0..63 are cached; a resource of any other device never is
static inline bool ba_pool_device_ok(int device) { return device >= 0 && device < BA_POOL_DEVICES; }

// idle handles (streams, events) per device, last in first out
template <class H> class BaIdleList {
  std::mutex mu_;
  std::vector<H> idle_[BA_POOL_DEVICES];
  const size_t max_idle_;
 public:
  explicit BaIdleList(size_t max_idle) : max_idle_(max_idle) {}      // per device; 0: unbounded
  H take(int device) {                                               // H() (a null handle): nothing cached -- the caller creates one
    if (!ba_pool_device_ok(device)) return H();
    std::lock_guard<std::mutex> lk(mu_);
    if (idle_[device].empty()) return H();
    H h = idle_[device].back(); idle_[device].pop_back();
    return h;
  }
  bool give(int device, H h) {                                       // false: full -- the caller destroys it
    if (!ba_pool_device_ok(device)) return false;
    std::lock_guard<std::mutex> lk(mu_);
    if (max_idle_ && idle_[device].size() >= max_idle_) return false;
    idle_[device].push_back(h);
    return true;
  }
};

struct BaBlock { void* p; size_t bytes; };      // a device slab / pinned block

// cached memory blocks per device, bounded in bytes and in blocks
class BaBlockCache {
  std::mutex mu_;
  std::vector<BaBlock> blocks_[BA_POOL_DEVICES];
  size_t bytes_[BA_POOL_DEVICES] = {0};
  const size_t max_bytes_, max_blocks_;
 public:
  BaBlockCache(size_t max_bytes, size_t max_blocks) : max_bytes_(max_bytes), max_blocks_(max_blocks) {}      // per device; max_blocks 0: unbounded
  // the smallest cached block that is large enough and not absurdly larger (bytes <= 4 x need + 1 MB); false: nothing cached -- the caller allocates
  bool take(int device, size_t need, BaBlock* out) {
    if (!ba_pool_device_ok(device)) return false;
    std::lock_guard<std::mutex> lk(mu_);
    std::vector<BaBlock>& v = blocks_[device];
    int best = -1;
    for (size_t i = 0; i < v.size(); ++i)
      if (v[i].bytes >= need && v[i].bytes <= 4 * need + (1u << 20) && (best < 0 || v[i].bytes < v[best].bytes)) best = (int)i;
    if (best < 0) return false;
    *out = v[best];
    v[best] = v.back(); v.pop_back();
    bytes_[device] -= out->bytes;
    return true;
  }
  bool give(int device, BaBlock b) {                                 // false: full -- the caller frees it
    if (!ba_pool_device_ok(device)) return false;
    std::lock_guard<std::mutex> lk(mu_);
    if ((max_blocks_ && blocks_[device].size() >= max_blocks_) || bytes_[device] + b.bytes > max_bytes_) return false;
    blocks_[device].push_back(b);
    bytes_[device] += b.bytes;
    return true;
  }
  std::vector<BaBlock> drain(int device) {                           // everything cached for the device: the caller frees it
    std::vector<BaBlock> out;
    if (!ba_pool_device_ok(device)) return out;
    std::lock_guard<std::mutex> lk(mu_);
    out.swap(blocks_[device]);
    bytes_[device] = 0;
    return out;
  }
  size_t cached_bytes(int device) { if (!ba_pool_device_ok(device)) return 0; std::lock_guard<std::mutex> lk(mu_); return bytes_[device]; }
  size_t cached_blocks(int device) { if (!ba_pool_device_ok(device)) return 0; std::lock_guard<std::mutex> lk(mu_); return blocks_[device].size(); }
};
