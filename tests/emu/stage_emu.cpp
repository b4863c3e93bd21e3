// stage_emu.cpp -- host-only exercise of cubemapslam_amd/csrc/cms_stage.h (CmsStage: the device block and the pinned block behind the host-buffer
// entries).  The memory policy is malloc with a record per block (size, side, how often freed) and counters for waits and copies; the copies are
// memcpy, so a sanitizer build sees every byte CmsStage lets through.  Exit status 0 only when every check holds.  tests/test_stage_cpu.py builds
// this plainly and under the host sanitizers and runs each build.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include "../../cubemapslam_amd/csrc/cms_stage.h"

static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "stage_emu: line %d: %s\n", __LINE__, #c); ++g_failed; } } while (0)

enum { ERR_ALLOC = -2, ERR_RANGE = -7 };
struct Rec { size_t bytes; bool pinned; int freed; };
struct World {
  std::map<void*, Rec> blocks;      // every block ever handed out
  int live = 0, takes = 0, gives = 0, waits = 0, copies = 0, range_errors = 0;
  bool waited = false;              // a wait that no free has followed yet
  bool releasing = false;           // release() frees without a wait: its owner's streams are idle
  bool fail_next_take = false;
  void* last_stream = nullptr;
  std::string last_who;
};
static World g;
static int g_stream_tag;
static void* const STREAM = &g_stream_tag;

struct EmuMem {
  static int take(void** p, size_t bytes, bool pinned) {
    CHECK(bytes > 0);                                       // a side nobody asked for is never allocated
    CHECK(!g.waited);                                       // (a wait is always followed by the free it was made for)
    if (g.fail_next_take) { g.fail_next_take = false; *p = nullptr; return ERR_ALLOC; }
    *p = malloc(bytes);
    g.blocks[*p] = Rec{bytes, pinned, 0};                   // (an address malloc hands out again starts a new record: the old one was checked at its free)
    ++g.live; ++g.takes;
    return 0;
  }
  static int give(void* p, bool pinned) {
    auto it = g.blocks.find(p);
    CHECK(it != g.blocks.end());
    if (it == g.blocks.end()) return 0;
    CHECK(it->second.freed == 0 && it->second.pinned == pinned);
    CHECK(g.releasing || g.waited);                         // the stream was waited for before a block it may still use is freed
    g.waited = false;
    ++it->second.freed; --g.live; ++g.gives;
    free(p);
    return 0;
  }
  static int wait(void* stream) { CHECK(!g.waited); g.waited = true; g.last_stream = stream; ++g.waits; return 0; }
  static int copy(void* dst, const void* src, size_t bytes, bool, void* stream) { memcpy(dst, src, bytes); g.last_stream = stream; ++g.copies; return 0; }
  static int range_error(const char* who) { g.last_who = who; ++g.range_errors; return ERR_RANGE; }
};
using Stage = CmsStageT<EmuMem>;

static void release(Stage& s) { g.releasing = true; s.release(); g.releasing = false; CHECK(!s.d && !s.h && s.d_bytes == 0 && s.h_bytes == 0); }

static void keep_and_grow() {
  Stage s;
  CHECK(s.reserve(STREAM, 1000, 400) == 0);
  CHECK(s.d && s.h && s.d_bytes == 1500 && s.h_bytes == 600 && g.waits == 0);      // need + need / 2; nothing was held: no wait
  uint8_t* d0 = s.d; uint8_t* h0 = s.h;
  CHECK(s.reserve(STREAM, 1500, 600) == 0 && s.d == d0 && s.h == h0 && g.takes == 2 && g.waits == 0);      // exactly the capacity: kept
  CHECK(s.reserve(STREAM, 1, 0) == 0 && s.d == d0 && s.h == h0);
  CHECK(s.reserve(STREAM, 1501, 600) == 0 && s.d_bytes == 2251 && s.h == h0 && g.waits == 1 && g.gives == 1);      // one side grows alone
  CHECK(g.last_stream == STREAM);
  CHECK(s.reserve(STREAM, 0, 601) == 0 && s.d_bytes == 2251 && s.h_bytes == 901 && g.waits == 2 && g.gives == 2);
  CHECK(!g.waited && g.live == 2);
  release(s);
  CHECK(g.live == 0 && g.waits == 2);
}

static void zero_sides() {
  const int takes0 = g.takes;
  Stage s;
  CHECK(s.reserve(STREAM, 0, 0) == 0 && !s.d && !s.h && g.takes == takes0);
  CHECK(s.reserve(STREAM, 0, 64) == 0 && !s.d && s.d_bytes == 0 && s.h && g.takes == takes0 + 1);      // pinned-only user
  CHECK(s.up(STREAM, 0, "zero") == 0 && s.back(STREAM, 0, 0, "zero") == 0);                            // nothing to copy is no range error ...
  CHECK(s.up(STREAM, 1, "zero") == ERR_RANGE);                                                         // ... but one byte into a block that is not there is
  release(s);
  Stage t;
  CHECK(t.reserve(STREAM, 64, 0) == 0 && t.d && !t.h && t.h_bytes == 0 && g.takes == takes0 + 2);      // device-only user
  release(t);
  release(t);                                                                                          // (releasing an empty stage frees nothing)
  CHECK(g.live == 0);
}

static void failing_allocation() {
  Stage s;
  g.fail_next_take = true;
  CHECK(s.reserve(STREAM, 100, 100) == ERR_ALLOC && !s.d && s.d_bytes == 0 && !s.h && s.h_bytes == 0);
  CHECK(s.reserve(STREAM, 100, 100) == 0 && s.d && s.h);
  const int gives0 = g.gives;
  g.fail_next_take = true;                                               // the regrowth fails behind the free: an empty block, not a dangling one
  CHECK(s.reserve(STREAM, 1000, 100) == ERR_ALLOC && !s.d && s.d_bytes == 0 && s.h && s.h_bytes == 150 && g.gives == gives0 + 1);
  CHECK(s.up(STREAM, 1, "after failure") == ERR_RANGE);
  CHECK(s.reserve(STREAM, 1000, 100) == 0 && s.d && s.d_bytes == 1500 && g.gives == gives0 + 1);      // (nothing was held: nothing freed twice)
  release(s);
  CHECK(g.live == 0);
}

static void ranges() {
  Stage s;
  CHECK(s.reserve(STREAM, 200, 100) == 0 && s.d_bytes == 300 && s.h_bytes == 150);      // the pinned block is the shorter one ...
  for (size_t i = 0; i < s.h_bytes; ++i) s.h[i] = (uint8_t)(i * 7 + 1);
  memset(s.d, 0, s.d_bytes);
  const int copies0 = g.copies, errs0 = g.range_errors;
  CHECK(s.up(STREAM, 150, "entry_a") == 0 && memcmp(s.d, s.h, 150) == 0 && g.copies == copies0 + 1);
  CHECK(s.up(STREAM, 151, "entry_a") == ERR_RANGE && g.last_who == "entry_a" && g.copies == copies0 + 1);
  memset(s.h, 0, s.h_bytes);
  CHECK(s.back(STREAM, 40, 150, "entry_b") == 0 && s.h[39] == 0 && s.h[40] == (uint8_t)(40 * 7 + 1) && s.h[149] == (uint8_t)(149 * 7 + 1));
  CHECK(s.back(STREAM, 40, 151, "entry_b") == ERR_RANGE && g.last_who == "entry_b");
  CHECK(s.back(STREAM, 151, 150, "entry_b") == ERR_RANGE);
  CHECK(s.back_and_wait(STREAM, 0, 150, "entry_c") == 0 && g.waited);
  g.waited = false;
  CHECK(s.back_and_wait(STREAM, 0, 151, "entry_c") == ERR_RANGE && !g.waited);           // a refused copy is not waited for
  release(s);
  Stage t;
  CHECK(t.reserve(STREAM, 100, 200) == 0 && t.d_bytes == 150 && t.h_bytes == 300);       // ... or the device block is
  memset(t.h, 3, t.h_bytes);
  CHECK(t.up(STREAM, 150, "entry_d") == 0 && t.up(STREAM, 151, "entry_d") == ERR_RANGE);
  CHECK(t.back(STREAM, 0, 150, "entry_d") == 0 && t.back(STREAM, 150, 151, "entry_d") == ERR_RANGE);
  CHECK(g.range_errors == errs0 + 6);
  release(t);
  CHECK(g.live == 0);
}

static void random_calls() {
  std::mt19937 rng(20240607u);
  Stage s[3];
  for (int i = 0; i < 10000; ++i) {
    Stage& q = s[rng() % 3];
    const size_t dn = rng() % 4 == 0 ? 0 : (size_t)1 << (rng() % 16), hn = rng() % 4 == 0 ? 0 : (size_t)(rng() % 50000);
    const size_t d0 = q.d_bytes, h0 = q.h_bytes;
    uint8_t* dp = q.d; uint8_t* hp = q.h;
    const int waits0 = g.waits, gives0 = g.gives;
    CHECK(q.reserve(STREAM, dn, hn) == 0);
    CHECK(q.d_bytes == (dn > d0 ? dn + dn / 2 : d0) && q.h_bytes == (hn > h0 ? hn + hn / 2 : h0));
    CHECK((dn > d0) || q.d == dp);
    CHECK((hn > h0) || q.h == hp);
    const int freed = (dn > d0 && dp ? 1 : 0) + (hn > h0 && hp ? 1 : 0);
    CHECK(g.waits == waits0 + freed && g.gives == gives0 + freed && !g.waited);
    const size_t n = q.d_bytes < q.h_bytes ? q.d_bytes : q.h_bytes;
    if (n) { memset(q.h, i & 255, n); CHECK(q.up(STREAM, n, "random") == 0 && q.back(STREAM, n / 2, n, "random") == 0); }
    CHECK(q.up(STREAM, n + 1, "random") == ERR_RANGE);
  }
  for (Stage& q : s) release(q);
  CHECK(g.live == 0 && g.takes == g.gives);
  for (const auto& kv : g.blocks) CHECK(kv.second.freed == 1);
}

int main() {
  keep_and_grow();
  zero_sides();
  failing_allocation();
  ranges();
  random_calls();
  if (g_failed) { fprintf(stderr, "stage_emu: %d check(s) failed\n", g_failed); return 1; }
  printf("stage_emu: ok (%d blocks, %d waits, %d copies, %d refused ranges)\n", g.takes, g.waits, g.copies, g.range_errors);
  return 0;
}
