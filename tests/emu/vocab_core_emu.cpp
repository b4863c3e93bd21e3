// vocab_core_emu.cpp -- the host side of ComputeBoW as a stand-alone program for the sanitizer builds (tests/test_vocab_cpu.py): the text-format
// loader (cubemapslam_amd/host/io_formats.cpp), the tree checks and re-laying, and the batch transform of csrc/cms_vocab_core.h on small seeded trees.
// Exits non-zero unless save -> load -> save is byte-identical, every malformed input is refused with a message, and the transform's outputs keep
// their invariants (ids ascend, every listed feature once, values finite) for every weighting and scoring.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "io_formats.h"
#include "../../cubemapslam_amd/csrc/cms_vocab_core.h"

using CubemapSLAM::VocabularyText;

static unsigned long long g_state = 88172645463325252ull;
static unsigned rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return (unsigned)(g_state >> 11); }
static int fails = 0;
#define CHECK(c, what) do { if (!(c)) { std::printf("FAILED: %s (line %d)\n", what, __LINE__); ++fails; } } while (0)

// a complete tree of branching k and depth L in level order, with `early` of the root's children turned into words
static VocabularyText make_tree(int k, int L, int scoring, int weighting, int early) {
  VocabularyText t;
  t.k = k; t.L = L; t.scoring = scoring; t.weighting = weighting;
  t.parent.assign(1, 0); t.is_leaf.assign(1, 0); t.desc.assign(32, 0); t.weight.assign(1, 0.0);
  std::vector<int> prev(1, 0);
  for (int level = 1; level <= L; ++level) {
    std::vector<int> cur;
    for (int p : prev)
      for (int c = 0; c < k; ++c) {
        const int id = t.nodes();
        const bool leaf = level == L || (level == 1 && c < early);
        t.parent.push_back(p); t.is_leaf.push_back(leaf ? 1 : 0);
        for (int b = 0; b < 32; ++b) t.desc.push_back((uint8_t)((p ? t.desc[32 * (size_t)p + b] : 0) ^ (rnd() & rnd() & rnd() & 255u)));
        const unsigned r = rnd() % 10;
        t.weight.push_back(!leaf ? 0.25 : r == 0 ? 0.0 : r == 1 ? -1.0 : 0.001 * (double)(rnd() % 5000 + 1));
        if (!leaf) cur.push_back(id);
      }
    prev.swap(cur);
  }
  return t;
}

static void run_transforms(const VocabularyText& t) {
  CmsVocabTree tree;
  const char* why = cms_vocab_relayout(t.k, t.L, t.scoring, t.weighting, t.nodes(), t.parent.data(), t.is_leaf.data(), t.desc.data(), t.weight.data(), &tree);
  CHECK(why == nullptr, why ? why : "relayout");
  if (why) return;
  const int ns[] = {0, 1, 65, 300};
  for (int n : ns)
    for (int levelsup = 0; levelsup <= t.L + 1; ++levelsup) {
      std::vector<uint8_t> desc(32 * (size_t)(n > 0 ? n : 1));
      for (auto& b : desc) b = (uint8_t)rnd();
      for (int i = 0; i + 1 < n; i += 3)      // every third descriptor repeats its neighbour: words with several features
        for (int b = 0; b < 32; ++b) desc[32 * (size_t)(i + 1) + b] = desc[32 * (size_t)i + b];
      CmsVocabResult r;
      cms_vocab_transform_host(tree.view(), n, desc.data(), levelsup, &r);
      CHECK(r.word_id.size() == r.word_val.size() && r.node_off.size() == r.node_id.size() + 1, "sizes");
      for (size_t i = 1; i < r.word_id.size(); ++i) CHECK(r.word_id[i] > r.word_id[i - 1], "word ids ascend");
      for (size_t i = 1; i < r.node_id.size(); ++i) CHECK(r.node_id[i] > r.node_id[i - 1], "node ids ascend");
      for (double v : r.word_val) CHECK(std::isfinite(v) && v > 0, "values");
      std::vector<int> seen((size_t)(n > 0 ? n : 1), 0);
      for (size_t e = 0; e < r.node_id.size(); ++e)
        for (int q = r.node_off[e]; q < r.node_off[e + 1]; ++q) {
          CHECK(r.node_feat[(size_t)q] >= 0 && r.node_feat[(size_t)q] < n && !seen[(size_t)r.node_feat[(size_t)q]]++, "a feature is listed once");
          CHECK(q == r.node_off[e] || r.node_feat[(size_t)q] > r.node_feat[(size_t)q - 1], "features ascend inside a node");
        }
      if (t.L - levelsup <= 0 && !r.node_id.empty()) CHECK(r.node_id.size() == 1 && r.node_id[0] == 0, "L - levelsup <= 0: the root");
    }
}

static bool refused(const std::string& text, const char* what) {
  VocabularyText t;
  std::string why;
  if (!CubemapSLAM::ParseVocabularyText(text, &t, &why)) { CHECK(!why.empty(), "a refusal carries a message"); return true; }
  CmsVocabTree tree;
  const char* w = cms_vocab_relayout(t.k, t.L, t.scoring, t.weighting, t.nodes(), t.parent.data(), t.is_leaf.data(), t.desc.data(), t.weight.data(), &tree);
  if (!w) std::printf("FAILED: accepted a malformed file: %s\n", what);
  return w != nullptr;
}

int main() {
  for (int scoring : {0, 1, 5})
    for (int weighting = 0; weighting < 4; ++weighting) {
      const VocabularyText t = make_tree(3 + weighting, 3, scoring, weighting, weighting % 2);
      run_transforms(t);
      const std::string a = CubemapSLAM::FormatVocabularyText(t);
      VocabularyText u;
      std::string why;
      CHECK(CubemapSLAM::ParseVocabularyText(a, &u, &why), why.c_str());
      CHECK(CubemapSLAM::FormatVocabularyText(u) == a, "save -> load -> save");
      VocabularyText w;
      CHECK(CubemapSLAM::ParseVocabularyText(a.substr(0, a.size() - 1), &w, &why) && w.parent == u.parent && w.desc == u.desc && w.weight == u.weight,
            "without the trailing newline");
      CHECK(CubemapSLAM::ParseVocabularyText(a + "\n\n", &w, &why) && w.parent == u.parent, "with empty lines behind");
      run_transforms(u);
    }
  const std::string d32 = " 1 2 3 4 5 6 7 8 9 10 11 12 13 14 15 16 17 18 19 20 21 22 23 24 25 26 27 28 29 30 31 32  ";
  int n_refused = 0;
  n_refused += refused("", "empty");
  n_refused += refused("21 3  0 0\n0 1" + d32 + "1\n", "k out of range");
  n_refused += refused("2 0  0 0\n0 1" + d32 + "1\n", "L out of range");
  n_refused += refused("2 3  6 0\n0 1" + d32 + "1\n", "scoring out of range");
  n_refused += refused("2 3  0 4\n0 1" + d32 + "1\n", "weighting out of range");
  n_refused += refused("2 2  0 0\n0 0" + d32 + "1\n0 1" + d32 + "1\n", "inner node without children");
  n_refused += refused("2 2  0 0\n0 1" + d32 + "1\n1 1" + d32 + "1\n", "leaf with children");
  n_refused += refused("2 2  0 0\n1 1" + d32 + "1\n", "parent id not smaller");
  n_refused += refused("2 2  0 0\n0 1" + d32 + "1\n5 1" + d32 + "1\n", "parent id beyond the file");
  n_refused += refused("2 2  0 0\n0 1" + d32 + "1\n0 1" + d32 + "1\n0 1" + d32 + "1\n", "more than k children");
  n_refused += refused("2 2  0 0\n0 1 1 2 3\n", "short line");
  n_refused += refused("2 2  0 0\n", "no words");
  CHECK(n_refused == 12, "every malformed file is refused");
  if (fails) return 1;
  std::printf("vocab_core_emu: ok\n");
  return 0;
}
