// Host build of cubemapslam_amd/csrc/cms_ba_group_kind.h (the group key of cms_ba_optimize_many and the per-window choices of the kernels that sum the
// Schur slices) for tests/test_ba_group_kind_cpu.py.
//   ba_group_kind_emu <BA_S3_STRIDE> <BA_LDS_CEILING> <solve_reduce_max>  < windows
// One window per input line: device fast_plan edge_list deterministic det_points has_runs se_waves det_ranges np solve3_ok slices
// One output line per window:  kind solve_presum solve_sums_slices solve3_lds presum_lds
// The presum decision is made the way ba_plan_sizes makes it (from np alone), the other one the way cms_ba_optimize_many makes it (from the window's own
// slice count, for deterministic windows of the fused chain that carry the edge-major list), then both are handed to the key.
#include <cstdio>
#include <cstdlib>
#include "../../cubemapslam_amd/csrc/cms_ba_group_kind.h"

int main(int argc, char** argv) {
  if (argc != 4) { fprintf(stderr, "usage: ba_group_kind_emu <stride> <lds ceiling> <solve_reduce_max>\n"); return 2; }
  const int stride = atoi(argv[1]);
  const size_t ceiling = (size_t)atoll(argv[2]);
  const int reduce_max = atoi(argv[3]);
  int dev, fast, edge, det, detp, runs, waves, ranges, np, s3ok, slices;
  long n = 0;
  for (;;) {
    const int got = scanf("%d %d %d %d %d %d %d %d %d %d %d", &dev, &fast, &edge, &det, &detp, &runs, &waves, &ranges, &np, &s3ok, &slices);
    if (got == EOF) break;
    if (got != 11 || np < 0 || np > 1000 || dev < 0 || dev > 63 || ranges < 0 || ranges > 128) { fprintf(stderr, "bad input line %ld\n", n + 1); return 2; }
    const size_t lds3 = ba_solve3_lds(np, stride);
    const int np2 = np * (np + 1) / 2;
    BaKindIn in;
    in.device = dev; in.fast_plan = fast != 0; in.edge_list = edge != 0; in.deterministic = det != 0; in.det_points = detp != 0; in.has_runs = runs != 0;
    in.se_waves = waves; in.det_ranges = ranges;
    in.solve_presum = ba_solve_presum_fits(s3ok != 0, lds3, np2, ceiling);
    in.solve_sums_slices = in.deterministic && !in.det_points && in.edge_list && ba_solve_sums_slices(slices, reduce_max);
    printf("%d %d %d %zu %zu\n", ba_group_kind(in), in.solve_presum ? 1 : 0, in.solve_sums_slices ? 1 : 0, lds3, ba_solve3_presum_lds(lds3, np2));
    ++n;
  }
  printf("ba_group_kind_emu: ok %ld windows\n", n);
  return 0;
}
