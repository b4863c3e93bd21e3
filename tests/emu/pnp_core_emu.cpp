// Host build of cubemapslam_amd/csrc/cms_pnp_core.h on its own for tests/test_pnp_cpu.py: the header is included as it stands (it compiles under g++,
// so there is nothing to paste), compiled with g++ -ffp-contract=off, and every stage of one solve is handed out.  With -DPNP_EMU_MAIN it is a
// stand-alone program that runs the solves and inlier tests of a case file (for a run under the host sanitizers):
//   file = int32 count, then per case: int32 n, int32 F, double pws[3n], us[2n], bearings[3n]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "cms_pnp_core.h"

extern "C" int emu_stages_size() { return (int)sizeof(CmsPnpStages); }
extern "C" double emu_compute_pose(int n, int F, const double* pws, const double* us, const double* bearings, CmsPnpStages* st, double* ut, double* alphas, double* R,
                                   double* t) {
  std::vector<double> pcs(3 * (size_t)n);
  double mtm[144];
  return cms_pnp_compute_pose(n, F, pws, us, bearings, alphas, pcs.data(), mtm, ut, R, t, st);
}

#ifdef PNP_EMU_MAIN
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  double sum = 0;
  int nan_poses = 0, inl = 0;
  for (int c = 0; c < count; ++c) {
    int32_t n = 0, F = 0;
    if (fread(&n, 4, 1, f) != 1 || fread(&F, 4, 1, f) != 1 || n < 1) return 2;
    std::vector<double> pws(3 * (size_t)n), us(2 * (size_t)n), be(3 * (size_t)n), al(4 * (size_t)n);
    if (fread(pws.data(), 8, pws.size(), f) != pws.size() || fread(us.data(), 8, us.size(), f) != us.size() || fread(be.data(), 8, be.size(), f) != be.size()) return 2;
    double ut[144], R[9], t[3];
    CmsPnpStages st;
    const double e = emu_compute_pose(n, F, pws.data(), us.data(), be.data(), &st, ut, al.data(), R, t);
    if (e == e) sum += e; else ++nan_poses;
    for (int i = 0; i < n; ++i) {
      const float P[3] = {(float)pws[3 * i], (float)pws[3 * i + 1], (float)pws[3 * i + 2]}, p2[2] = {(float)us[2 * i], (float)us[2 * i + 1]};
      inl += cms_pnp_is_inlier(F, R, t, P, p2, 5.991f) ? 1 : 0;
    }
    int idx[4];
    const int dr[4] = {n - 1, 0, n > 2 ? n - 3 : 0, 0};
    if (n >= 4) cms_pnp_resolve_draws(n, dr, idx);
  }
  fclose(f);
  printf("%d cases, sum of finite errors %.6g, %d NaN poses, %d inliers\n", count, sum, nan_poses, inl);
  return 0;
}
#endif
