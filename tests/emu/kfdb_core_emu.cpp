// kfdb_core_emu.cpp -- a stand-alone program over the host build of csrc/cms_kfdb_core.h (no HIP, no Python): replays the cases that
// tests/kfdb_cases.py wrote as a token stream (kfdb_cases.to_text) on a CmsKfdbHost and compares every detect with the results recorded in the
// stream -- the numpy restatement's -- candidate lists as lists, common-word counts as ints, scores as float bits.  Exits non-zero at the first
// difference.  tests/test_kfdb_cpu.py builds it plain and with AddressSanitizer + UBSan and runs each build as a child process.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>
#include "../../cubemapslam_amd/csrc/cms_kfdb_core.h"

static std::ifstream in;
static std::string tok() {
  std::string t;
  if (!(in >> t)) { std::printf("kfdb_core_emu: unexpected end of the stream\n"); std::exit(2); }
  return t;
}
static long long num() { return std::strtoll(tok().c_str(), nullptr, 10); }
static double dbl() { const unsigned long long b = std::strtoull(tok().c_str(), nullptr, 10); double d; std::memcpy(&d, &b, 8); return d; }
static float flt() { const uint32_t b = (uint32_t)std::strtoul(tok().c_str(), nullptr, 10); float f; std::memcpy(&f, &b, 4); return f; }
static void expect(const std::string& want) {
  const std::string t = tok();
  if (t != want) { std::printf("kfdb_core_emu: expected '%s', read '%s'\n", want.c_str(), t.c_str()); std::exit(2); }
}
#define FAIL(...) do { std::printf("kfdb_core_emu: case %s detect %d job %d: ", name.c_str(), n_detect, j); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } while (0)

int main(int argc, char** argv) {
  if (argc != 2) { std::printf("usage: kfdb_core_emu <cases.txt>\n"); return 2; }
  in.open(argv[1]);
  if (!in) { std::printf("kfdb_core_emu: cannot open %s\n", argv[1]); return 2; }
  int n_cases = 0, n_jobs = 0;
  std::string t;
  while (in >> t) {
    if (t != "case") { std::printf("kfdb_core_emu: expected 'case'\n"); return 2; }
    const std::string name = tok();
    const int K = (int)num(), maxf = (int)num();
    CmsKfdbHost db(K, maxf);
    int n_detect = 0;
    for (std::string op = tok(); op != "end"; op = tok()) {
      if (op == "set_bow") {
        const int slot = (int)num(), n = (int)num();
        std::vector<int> id((size_t)n);
        std::vector<double> val((size_t)n);
        for (int& i : id) i = (int)num();
        for (double& v : val) v = dbl();
        if (db.set_bow(slot, n, id.data(), val.data())) { std::printf("kfdb_core_emu: case %s: set_bow refused\n", name.c_str()); return 1; }
      } else if (op == "refill") {
        db.refill((int)num());
      } else if (op == "clear") {
        db.clear((int)num());
      } else if (op == "covis") {
        const int slot = (int)num();
        int neigh[CMS_KFDB_COVIS];
        for (int& n : neigh) n = (int)num();
        if (db.set_covisibles(1, &slot, neigh)) { std::printf("kfdb_core_emu: case %s: set_covisibles refused\n", name.c_str()); return 1; }
      } else if (op == "add") {
        const int n = (int)num();
        std::vector<int> s((size_t)n), g((size_t)n);
        for (int& i : s) i = (int)num();
        for (int& i : g) i = (int)num();
        if (db.add(n, s.data(), g.data())) { std::printf("kfdb_core_emu: case %s: add refused\n", name.c_str()); return 1; }
      } else if (op == "erase") {
        const int n = (int)num();
        std::vector<int> s((size_t)n);
        for (int& i : s) i = (int)num();
        if (db.erase(n, s.data())) { std::printf("kfdb_core_emu: case %s: erase refused\n", name.c_str()); return 1; }
      } else if (op == "detect") {
        const int nj = (int)num();
        for (int j = 0; j < nj; ++j) {
          expect("job");
          CmsKfdbQuery q;
          q.mode = (int)num(); q.group = (int)num(); q.min_score = flt();
          std::vector<int> conn((size_t)num());
          for (int& c : conn) c = (int)num();
          q.n_connected = q.mode == CMS_KFDB_LOOP ? (int)conn.size() : 0; q.connected = conn.data();
          std::vector<int> id;
          std::vector<double> val;
          const std::string form = tok();
          if (form == "slot") {
            const int s = (int)num();
            id = db.slots[(size_t)s].id; val = db.slots[(size_t)s].val;
          } else {
            id.resize((size_t)num()); val.resize(id.size());
            for (int& i : id) i = (int)num();
            for (double& v : val) v = dbl();
          }
          q.bow = CmsKfdbBow{(int)id.size(), id.data(), val.data()};
          std::vector<int> cand, common((size_t)K);
          std::vector<float> score((size_t)K);
          db.detect(q, &cand, common.data(), score.data());
          expect("expect");
          const size_t nc = (size_t)num();
          std::vector<int> want(nc);
          for (int& c : want) c = (int)num();
          if (want != cand) FAIL("%zu candidates, %zu expected (or another order)", cand.size(), nc);
          for (int s = 0; s < K; ++s) { const int w = (int)num(); if (w != common[(size_t)s]) FAIL("common words of slot %d: %d, expected %d", s, common[(size_t)s], w); }
          for (int s = 0; s < K; ++s) {
            const uint32_t w = (uint32_t)num();
            uint32_t g;
            std::memcpy(&g, &score[(size_t)s], 4);
            if (w != g) FAIL("score bits of slot %d: %08x, expected %08x", s, g, w);
          }
          ++n_jobs;
        }
        ++n_detect;
      } else { std::printf("kfdb_core_emu: unknown operation '%s'\n", op.c_str()); return 2; }
    }
    ++n_cases;
  }
  std::printf("kfdb_core_emu: ok (%d cases, %d queries)\n", n_cases, n_jobs);
  return 0;
}
