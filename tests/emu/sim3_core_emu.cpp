// Host build of cubemapslam_amd/csrc/cms_sim3_core.h on its own for tests/test_sim3_cpu.py: the header is included as it stands (it compiles under
// g++, so there is nothing to paste), compiled with g++ -ffp-contract=off, and every stage of one solve is handed out.  With -DSIM3_EMU_MAIN it
// is a stand-alone program that runs the solves, inlier tests and draw resolutions of a case file (for a run under the host sanitizers):
//   file = int32 count, then per case: int32 n (>= 3), int32 F, int32 fix_scale, float x1[3n], x2[3n], me1[n], me2[n]; the solve is on points 0, 1, 2
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "cms_sim3_core.h"

extern "C" int emu_stages_size() { return (int)sizeof(CmsSim3Stages); }
extern "C" int emu_motion_size() { return (int)sizeof(CmsSim3Motion); }
extern "C" void emu_sim3_compute(const float* P1, const float* P2, int fix_scale, CmsSim3Motion* m, CmsSim3Stages* st) { cms_sim3_compute(P1, P2, fix_scale, m, st); }

#ifdef SIM3_EMU_MAIN
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t count = 0;
  if (fread(&count, 4, 1, f) != 1) return 2;
  int nan_motions = 0, inl = 0;
  long long idx_sum = 0;
  for (int c = 0; c < count; ++c) {
    int32_t n = 0, F = 0, fix = 0;
    if (fread(&n, 4, 1, f) != 1 || fread(&F, 4, 1, f) != 1 || fread(&fix, 4, 1, f) != 1 || n < 3) return 2;
    std::vector<float> x1(3 * (size_t)n), x2(3 * (size_t)n), me1((size_t)n), me2((size_t)n);
    if (fread(x1.data(), 4, x1.size(), f) != x1.size() || fread(x2.data(), 4, x2.size(), f) != x2.size() || fread(me1.data(), 4, me1.size(), f) != me1.size() ||
        fread(me2.data(), 4, me2.size(), f) != me2.size()) return 2;
    CmsSim3Motion m;
    CmsSim3Stages st;
    cms_sim3_compute(x1.data(), x2.data(), fix, &m, &st);
    bool finite = true;
    for (int k = 0; k < 12; ++k) finite = finite && m.T12[k] - m.T12[k] == 0.0f;      // false for NaN and inf
    if (!finite) ++nan_motions;
    for (int i = 0; i < n; ++i) inl += cms_sim3_is_inlier(F, m.T12, m.T21, x1.data() + 3 * i, x2.data() + 3 * i, me1[(size_t)i], me2[(size_t)i]) ? 1 : 0;
    int idx[3];
    const int dr[3] = {n - 1, 0, n - 3};
    cms_sim3_resolve_draws(n, dr, idx);
    idx_sum += idx[0] + idx[1] + idx[2];
  }
  fclose(f);
  printf("%d cases, %d NaN motions, %d inliers, index sum %lld\n", count, nan_motions, inl, idx_sum);
  return 0;
}
#endif
