// Host build of what the three RANSAC solvers share -- cubemapslam_amd/csrc/cms_ransac_core.h and cms_ransac_job_check.h, and through them the
// PnP and Sim3 job checks -- on its own for tests/test_ransac_common_cpu.py: the headers are included as they stand and compiled by g++.  With
// -DRANSAC_EMU_MAIN it is a stand-alone program (for a run under the host sanitizers) that reads a case file and prints one line per record:
//   file = int32 count, then per record an int32 kind and
//     0  resolve      int32 K (3, 4 or 8), N, draws[K]                                          -> "r idx..."
//     1  hypotheses   int32 N, min_inliers, max_its, iterations, n_iterations                   -> "h H_max H_min"
//     2  mask         int32 N, uint8 bytes[N]: packed, counted against the bytes, unpacked      -> "m N set words..."
//     3  iterations   float64 probability, float32 epsilon                                      -> "i n"
// Every buffer of the program has exactly the size the helper may touch.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "cubemapslam_hip.h"
#include "cms_ransac_core.h"
#include "cms_pnp_job_check.h"
#include "cms_sim3_job_check.h"

static int resolve(int K, int N, const int* draws, int* idx) {
  if (K == 3) cms_ransac_resolve_draws<3>(N, draws, idx);
  else if (K == 4) cms_ransac_resolve_draws<4>(N, draws, idx);
  else if (K == 8) cms_ransac_resolve_draws<8>(N, draws, idx);
  else return -1;
  return 0;
}

extern "C" int emu_resolve_draws(int K, int N, const int* draws, int* idx) { return resolve(K, N, draws, idx); }
extern "C" void emu_hypotheses(int N, int min_inliers, int max_its, int iterations, int n_iterations, int* H_max, int* H_min) {
  cms_ransac_hypotheses(N, min_inliers, max_its, iterations, n_iterations, H_max, H_min);
}
extern "C" int emu_check_draws(const int* draws, int n_draws, int H, int K, int N) { return cms_ransac_check_draws(draws, n_draws, H, K, N); }
extern "C" int emu_check_best_mask(const uint8_t* mask, int N, int best_inliers) { return cms_ransac_check_best_mask(mask, N, best_inliers); }
extern "C" int emu_pnp_check_job(const cms_pnp_job* q, int* H) { return cms_pnp_check_job(*q, H); }
extern "C" int emu_sim3_check_job(const cms_sim3_job* q, int* H_draws, int* H_run) { return cms_sim3_check_job(*q, H_draws, H_run); }
extern "C" int emu_iterations(double probability, float epsilon) { return cms_ransac_iterations(probability, epsilon); }
extern "C" void emu_mask_pack(const uint8_t* bytes, int N, unsigned long long* words) { cms_mask_pack(bytes, N, words); }
extern "C" void emu_mask_unpack(const unsigned long long* words, int N, uint8_t* bytes) { cms_mask_unpack(words, N, bytes); }

#ifdef RANSAC_EMU_MAIN
static bool rd(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, bytes, 1, f) == 1; }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t count = 0;
  if (!rd(f, &count, 4)) return 2;
  for (int c = 0; c < count; ++c) {
    int32_t kind = -1;
    if (!rd(f, &kind, 4)) return 2;
    if (kind == 0) {
      int32_t kn[2];
      if (!rd(f, kn, 8) || kn[0] < 1 || kn[0] > 8) return 2;
      std::vector<int> draws((size_t)kn[0]), idx((size_t)kn[0]);
      if (!rd(f, draws.data(), 4 * draws.size()) || resolve(kn[0], kn[1], draws.data(), idx.data())) return 2;
      printf("r");
      for (int v : idx) printf(" %d", v);
      printf("\n");
    } else if (kind == 1) {
      int32_t v[5];
      if (!rd(f, v, 20)) return 2;
      int H_max = -1, H_min = -1;
      cms_ransac_hypotheses(v[0], v[1], v[2], v[3], v[4], &H_max, &H_min);
      printf("h %d %d\n", H_max, H_min);
    } else if (kind == 2) {
      int32_t N = 0;
      if (!rd(f, &N, 4) || N < 0) return 2;
      std::vector<uint8_t> bytes((size_t)N), back((size_t)N, 7);
      std::vector<unsigned long long> words(((size_t)N + 63) / 64, 0ull);
      if (!rd(f, bytes.data(), bytes.size())) return 2;
      cms_mask_pack(bytes.data(), N, words.data());
      int set = 0;
      for (uint8_t b : bytes) set += b ? 1 : 0;
      cms_mask_unpack(words.data(), N, back.data());
      if (cms_ransac_check_best_mask(back.data(), N, set)) return 3;
      printf("m %d %d", N, set);
      for (unsigned long long w : words) printf(" %llx", w);
      printf("\n");
    } else if (kind == 3) {
      double p = 0;
      float e = 0;
      if (!rd(f, &p, 8) || !rd(f, &e, 4)) return 2;
      printf("i %d\n", cms_ransac_iterations(p, e));
    } else return 2;
  }
  fclose(f);
  return 0;
}
#endif
