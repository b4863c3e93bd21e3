// ba_pool_emu.cpp -- host-only exercise of cubemapslam_amd/csrc/cms_ba_pool.h (the caches behind the local-BA streams, events, slabs and pinned blocks).
// Handles and blocks are faked with records that know their state (held by a caller / cached / freed); every hand-over is checked against it.
// Exit status 0 only when every check holds.  tests/test_ba_pool_cpu.py builds this plainly and under the host sanitizers and runs each build.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>
#include "../../cubemapslam_amd/csrc/cms_ba_pool.h"

static std::atomic<int> g_failed{0};
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "ba_pool_emu: line %d: %s\n", __LINE__, #c); g_failed.fetch_add(1); } } while (0)

static const size_t MB = (size_t)1 << 20;
enum { HELD = 0, CACHED = 1, FREED = 2 };
struct Rec { std::atomic<int> state{HELD}; size_t bytes = 0; };
static BaBlock block(Rec* r) { return BaBlock{r, r->bytes}; }
static Rec* rec(const BaBlock& b) { return static_cast<Rec*>(b.p); }
static bool move(Rec* r, int from, int to) { int f = from; return r->state.compare_exchange_strong(f, to); }      // false: somebody else had it

static void best_fit() {
  BaBlockCache c((size_t)2 << 30, 512);
  Rec r[4];
  const size_t mb[4] = {1, 3, 6, 64};
  for (int i = 0; i < 4; ++i) { r[i].bytes = mb[i] * MB; CHECK(c.give(0, block(&r[i]))); }
  CHECK(c.cached_bytes(0) == 74 * MB && c.cached_blocks(0) == 4);
  BaBlock b{nullptr, 0};
  CHECK(c.take(0, 2 * MB, &b) && b.p == &r[1] && b.bytes == 3 * MB);      // the smallest that is large enough
  CHECK(!c.take(0, 8 * MB, &b));                                          // 6 MB is too small, 64 MB > 4 x 8 + 1 MB
  CHECK(c.take(0, 16 * MB - MB / 4, &b) && b.p == &r[3]);                 // 64 MB <= 4 x 15.75 + 1 MB: the bound itself is taken
  CHECK(c.cached_bytes(0) == 7 * MB && c.cached_blocks(0) == 2);
  CHECK(!c.take(1, 1 * MB, &b));                                          // another device's cache is another cache
}

static void caps() {
  {
    BaBlockCache c(10 * MB, 512);
    Rec a, b, d;
    a.bytes = 6 * MB; b.bytes = 6 * MB; d.bytes = 4 * MB;
    CHECK(c.give(0, block(&a)));
    CHECK(!c.give(0, block(&b)) && c.cached_bytes(0) == 6 * MB);          // past the byte cap: the caller frees
    CHECK(c.give(0, block(&d)) && c.cached_bytes(0) == 10 * MB);          // exactly the cap fits
    CHECK(c.give(1, block(&b)));                                          // the caps are per device
  }
  {
    BaBlockCache c((size_t)2 << 30, 512);
    std::vector<Rec> r(513);
    for (int i = 0; i < 513; ++i) { r[i].bytes = 1024; CHECK(c.give(0, block(&r[i])) == (i < 512)); }
    CHECK(c.cached_blocks(0) == 512 && c.cached_bytes(0) == 512 * 1024);
    BaBlockCache u(MB, 0);                                                // no block cap: only the bytes bound it
    for (int i = 0; i < 513; ++i) CHECK(u.give(0, block(&r[i])));
  }
  // a random sequence against a model: the byte counter equals the sum of the cached blocks after every call (a counter gone "negative" would not)
  BaBlockCache c(40 * MB, 16);
  std::vector<Rec> r(64);
  std::vector<int> where(64, HELD);
  uint32_t x = 12345;
  auto rnd = [&]() { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return x; };
  for (int i = 0; i < 64; ++i) r[i].bytes = (1 + rnd() % 8) * MB / 2;
  for (int it = 0; it < 20000; ++it) {
    const int i = (int)(rnd() % 64), op = (int)(rnd() % 16);
    if (op == 0) { for (const BaBlock& b : c.drain(0)) { CHECK(where[rec(b) - r.data()] == CACHED); where[rec(b) - r.data()] = HELD; } }
    else if (op < 8 && where[i] == HELD) { if (c.give(0, block(&r[i]))) where[i] = CACHED; }
    else if (op >= 8) {
      BaBlock b{nullptr, 0};
      const size_t need = (1 + rnd() % 8) * MB / 2;
      if (c.take(0, need, &b)) { CHECK(where[rec(b) - r.data()] == CACHED && b.bytes >= need && b.bytes <= 4 * need + MB); where[rec(b) - r.data()] = HELD; }
    }
    size_t sum = 0, n = 0;
    for (int k = 0; k < 64; ++k) if (where[k] == CACHED) { sum += r[k].bytes; ++n; }
    CHECK(c.cached_bytes(0) == sum && c.cached_blocks(0) == n && sum <= 40 * MB && n <= 16);
    if (g_failed.load()) return;
  }
}

static void drain_and_devices() {
  BaBlockCache c((size_t)2 << 30, 512);
  std::vector<Rec> r(10);
  for (int i = 0; i < 10; ++i) { r[i].bytes = (size_t)(i + 1) * 4096; CHECK(c.give(i < 7 ? 3 : 4, block(&r[i]))); }
  std::vector<BaBlock> d = c.drain(3);
  std::vector<int> seen(10, 0);
  for (const BaBlock& b : d) { CHECK(b.bytes == rec(b)->bytes); ++seen[rec(b) - r.data()]; }
  for (int i = 0; i < 10; ++i) CHECK(seen[i] == (i < 7 ? 1 : 0));        // every cached block of the device, once
  CHECK(c.cached_bytes(3) == 0 && c.cached_blocks(3) == 0 && c.drain(3).empty());
  CHECK(c.cached_blocks(4) == 3);
  // devices outside 0..63 are never cached
  BaIdleList<int> l(4);
  for (int dev : {-1, 64, 1 << 30, -(1 << 30)}) {
    BaBlock b{nullptr, 0};
    CHECK(!c.give(dev, block(&r[0])) && !c.take(dev, 1, &b) && c.drain(dev).empty() && c.cached_bytes(dev) == 0 && c.cached_blocks(dev) == 0);
    CHECK(!l.give(dev, 7) && l.take(dev) == 0);
  }
  CHECK(c.give(63, block(&r[0])) && c.drain(63).size() == 1);
}

static void handle_lists() {
  BaIdleList<int> l(3), unbounded(0);
  CHECK(l.take(0) == 0);                                                  // (handles are non-zero: 0 says "nothing cached")
  for (int i = 1; i <= 4; ++i) CHECK(l.give(0, i) == (i <= 3));          // the fourth is the caller's to destroy
  CHECK(l.give(1, 9));                                                    // per device
  CHECK(l.take(0) == 3 && l.take(0) == 2 && l.take(0) == 1 && l.take(0) == 0 && l.take(1) == 9);
  for (int i = 1; i <= 100000; ++i) CHECK(unbounded.give(5, i));
  CHECK(unbounded.take(5) == 100000);
}

// 16 threads, 20 000 random take / give / drain operations each, two devices, one block cache and one handle list between them
static void concurrency() {
  const int T = 16, OPS = 20000;
  BaBlockCache cache(24 * MB, 32);
  BaIdleList<Rec*> handles(8);
  std::vector<std::vector<Rec*>> made(T), held_b(T), held_h(T);
  std::atomic<long> freed{0};
  auto release = [&](Rec* r) { CHECK(move(r, CACHED, FREED)); freed.fetch_add(1); };
  auto worker = [&](int t) {
    uint32_t x = 2463534242u + 977u * (uint32_t)t;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return x; };
    for (int it = 0; it < OPS; ++it) {
      const int dev = (int)(rnd() & 1), op = (int)(rnd() % 100);
      std::vector<Rec*>& hb = held_b[t];
      std::vector<Rec*>& hh = held_h[t];
      if (op < 2) {
        for (const BaBlock& b : cache.drain(dev)) release(rec(b));
      } else if (op < 35) {                                               // a block: cached or new
        const size_t need = (1 + rnd() % 16) * MB / 8;
        BaBlock b{nullptr, 0};
        if (cache.take(dev, need, &b)) { CHECK(move(rec(b), CACHED, HELD) && b.bytes == rec(b)->bytes && b.bytes >= need); hb.push_back(rec(b)); }
        else { Rec* r = new Rec; r->bytes = need; made[t].push_back(r); hb.push_back(r); }
      } else if (op < 65 && !hb.empty()) {                                // a block goes back (marked before it is visible to the others)
        const size_t k = rnd() % hb.size();
        Rec* r = hb[k]; hb[k] = hb.back(); hb.pop_back();
        CHECK(move(r, HELD, CACHED));
        if (!cache.give(dev, block(r))) release(r);
      } else if (op < 83) {                                               // a handle: idle or new
        Rec* r = handles.take(dev);
        if (r) CHECK(move(r, CACHED, HELD));
        else { r = new Rec; made[t].push_back(r); }
        hh.push_back(r);
      } else if (!hh.empty()) {
        Rec* r = hh.back(); hh.pop_back();
        CHECK(move(r, HELD, CACHED));
        if (!handles.give(dev, r)) release(r);
      }
    }
  };
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t) th.emplace_back(worker, t);
  for (std::thread& q : th) q.join();
  // every record ever made is held by a thread, cached, or was reported to be freed -- exactly one of the three
  long n_made = 0, n_held = 0, n_cached = 0, n_state[3] = {0, 0, 0};
  for (int t = 0; t < T; ++t) {
    n_made += (long)made[t].size();
    for (Rec* r : held_b[t]) { CHECK(r->state.load() == HELD); ++n_held; }
    for (Rec* r : held_h[t]) { CHECK(r->state.load() == HELD); ++n_held; }
  }
  size_t cached_bytes = 0;
  for (int dev = 0; dev < 2; ++dev) {
    cached_bytes = cache.cached_bytes(dev);
    size_t sum = 0;
    for (const BaBlock& b : cache.drain(dev)) { CHECK(rec(b)->state.load() == CACHED); sum += b.bytes; ++n_cached; }
    CHECK(sum == cached_bytes && sum <= 24 * MB && cache.cached_bytes(dev) == 0);
    int nh = 0;
    for (Rec* r = handles.take(dev); r; r = handles.take(dev)) { CHECK(r->state.load() == CACHED); ++n_cached; ++nh; }
    CHECK(nh <= 8);
  }
  for (int t = 0; t < T; ++t) for (Rec* r : made[t]) ++n_state[r->state.load()];
  CHECK(n_state[HELD] == n_held && n_state[CACHED] == n_cached && n_state[FREED] == freed.load());
  CHECK(n_made == n_held + n_cached + freed.load() && n_made > 1000 && freed.load() > 100 && n_cached > 0);
  for (int t = 0; t < T; ++t) for (Rec* r : made[t]) delete r;
  printf("ba_pool_emu: %ld records: %ld held, %ld cached, %ld freed\n", n_made, n_held, n_cached, freed.load());
}

int main() {
  best_fit();
  caps();
  drain_and_devices();
  handle_lists();
  concurrency();
  if (g_failed.load()) { fprintf(stderr, "ba_pool_emu: %d checks failed\n", g_failed.load()); return 1; }
  printf("ba_pool_emu: ok\n");
  return 0;
}
