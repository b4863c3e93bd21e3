// covis_core_emu.cpp -- csrc/cms_covis_core.h on its own, for tests/test_covis_cpu.py::test_core_emulation (plain and under ASan + UBSan): replays
// the cases of tests/covis_cases.py from a text file (covis_cases.to_text: the tables, the queries and the restatement's answers) and compares.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../cubemapslam_amd/csrc/cms_covis_core.h"

static FILE* g_f;
static bool next_int(long long* v) { return fscanf(g_f, "%lld", v) == 1; }
static int rd() {
  long long v;
  if (!next_int(&v)) { fprintf(stderr, "covis_core_emu: the file ends inside a case\n"); exit(2); }
  return (int)v;
}
static std::vector<int> rdv(size_t n) {
  std::vector<int> v(n);
  for (int& x : v) x = rd();
  return v;
}
static int g_case = 0, g_query = 0;
static void check(bool ok, const char* what) {
  if (!ok) { fprintf(stderr, "covis_core_emu: case %d, query %d: %s differs\n", g_case, g_query, what); exit(1); }
}

int main(int argc, char** argv) {
  if (argc != 2 || !(g_f = fopen(argv[1], "r"))) { fprintf(stderr, "usage: covis_core_emu cases.txt\n"); return 2; }
  char word[16];
  int n_queries = 0;
  while (fscanf(g_f, "%15s", word) == 1) {
    if (strcmp(word, "case") != 0) { fprintf(stderr, "covis_core_emu: expected `case`\n"); return 2; }
    ++g_case; g_query = 0;
    const int K = rd(), maxf = rd(), M = rd();
    CmsCovisHostStore st(K, maxf, K);
    std::vector<int> slots;
    for (int m = 0; m < M; ++m) {
      const int slot = rd(), n = rd();
      const std::vector<int> mp = rdv((size_t)n), oct = rdv((size_t)n);
      check(st.put(slot, n, mp.data(), oct.data()) == 0, "put");
      slots.push_back(slot);
    }
    check(st.build(M, slots.data()) == 0, "build");
    const CmsCovisHost& ix = st.index;
    const int nq = rd();
    for (int q = 0; q < nq; ++q, ++n_queries) {
      g_query = q;
      const int kind = rd(), nj = rd();
      if (kind == 1) {
        const std::vector<int> off = rdv((size_t)nj + 1), ids = rdv((size_t)off[(size_t)nj]), want = rdv((size_t)nj * (size_t)M);
        std::vector<int> got((size_t)nj * (size_t)M + 1, -7);
        check(ix.votes(nj, off.data(), ids.data(), got.data()) == 0, "the code of votes");
        got.pop_back();
        check(got == want, "votes");
      } else if (kind == 2) {
        const int th = rd();
        const std::vector<int> jobs = rdv((size_t)nj), ww = rdv((size_t)nj * (size_t)M), wo = rdv((size_t)nj * (size_t)M), wn = rdv((size_t)nj);
        std::vector<int> w((size_t)nj * (size_t)M), o((size_t)nj * (size_t)M), n((size_t)nj);
        check(ix.connections(nj, jobs.data(), th, w.data(), o.data(), n.data()) == 0, "the code of connections");
        check(w == ww, "weights"); check(o == wo, "order"); check(n == wn, "n_connected");
      } else if (kind == 3) {
        const int th_obs = rd();
        const std::vector<int> off = rdv((size_t)nj + 1);
        const size_t Q = (size_t)off[(size_t)nj];
        const std::vector<int> jobs = rdv(Q), er = rdv(Q), wm = rdv(Q), wr = rdv(Q), wf = rdv(Q);
        std::vector<uint8_t> erasable(Q + 1), red(Q + 1);
        for (size_t i = 0; i < Q; ++i) erasable[i] = (uint8_t)er[i];
        std::vector<int> nm(Q + 1), nr(Q + 1);
        check(ix.culling(nj, off.data(), jobs.data(), erasable.data(), th_obs, nm.data(), nr.data(), red.data()) == 0, "the code of culling");
        for (size_t i = 0; i < Q; ++i) { check(nm[i] == wm[i], "n_mps"); check(nr[i] == wr[i], "n_redundant"); check(red[i] == wf[i], "redundant"); }
      } else if (kind == 4) {
        const int cap = rd();
        const std::vector<int> off = rdv((size_t)nj + 1), kfs = rdv((size_t)off[(size_t)nj]);
        const int want_rc = rd();
        const std::vector<int> wn = rdv((size_t)nj);
        std::vector<int> ids((size_t)nj * (size_t)cap + 1, -7), n((size_t)nj + 1);
        check(ix.local_points(nj, off.data(), kfs.data(), cap, ids.data(), n.data()) == want_rc, "the code of local_points");
        for (int j = 0; j < nj; ++j) {
          check(n[(size_t)j] == wn[(size_t)j], "n_out");
          const int k = wn[(size_t)j] < cap ? wn[(size_t)j] : cap;
          const std::vector<int> want = rdv((size_t)k);
          for (int i = 0; i < k; ++i) check(ids[(size_t)j * (size_t)cap + (size_t)i] == want[(size_t)i], "ids_out");
        }
        check(ids.back() == -7, "the end of ids_out");
      } else { fprintf(stderr, "covis_core_emu: unknown query kind %d\n", kind); return 2; }
    }
    // the refusals leave the index in place: a row that names an id twice, an empty slot, a slot twice
    if (M >= 2) {
      std::vector<int> w0((size_t)M), o0((size_t)M), w1((size_t)M), o1((size_t)M);
      int n0 = 0, n1 = 0, job = 0;
      ix.connections(1, &job, 1, w0.data(), o0.data(), &n0);
      const int dup_mp[3] = {42, 7, 42}, dup_oct[3] = {0, 0, 0};
      int free_slot = 0;
      while (free_slot < K && st.slots[(size_t)free_slot].used) ++free_slot;
      if (free_slot < K) {
        const std::vector<int> twice = {slots[0], slots[1], slots[0]}, empty = {slots[0], free_slot};
        check(st.build(3, twice.data()) == -1, "a slot named twice");
        check(st.build(2, empty.data()) == -1, "an empty slot");
        check(st.put(free_slot, 3, dup_mp, dup_oct) == 0, "put");
        check(st.build(2, empty.data()) == -1, "an id twice in a row");
        ix.connections(1, &job, 1, w1.data(), o1.data(), &n1);
        check(ix.n_members == M && w0 == w1 && o0 == o1 && n0 == n1, "the index after refused builds");
      }
    }
  }
  fclose(g_f);
  printf("covis_core_emu: ok (%d cases, %d queries)\n", g_case, n_queries);
  return 0;
}
