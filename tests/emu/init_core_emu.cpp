// Host build of cubemapslam_amd/csrc/cms_init_core.h on its own: the header and the host loop over it (cubemapslam_amd/host/init_host.cpp) are included
// as they stand, compiled with g++ -ffp-contract=off.  With -DINIT_EMU_MAIN it is a stand-alone program that runs the whole attempts of a case file
// (for a run under the host sanitizers, -fsanitize=address,undefined):
//   file = int32 count, int32 F, float cos_fov, then per case: int32 n1, n2, iterations, float sigma, float keys1[2 n1], rays1[3 n1], keys2[2 n2],
//   rays2[3 n2], int32 matches12[n1], draws[8 iterations]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../cubemapslam_amd/host/init_host.cpp"

#ifdef INIT_EMU_MAIN
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t count = 0, F = 0;
  float cos_fov = 0;
  if (fread(&count, 4, 1, f) != 1 || fread(&F, 4, 1, f) != 1 || fread(&cos_fov, 4, 1, f) != 1) return 2;
  int ok = 0, refused = 0, tri = 0;
  double score = 0;
  for (int c = 0; c < count; ++c) {
    int32_t n1 = 0, n2 = 0, its = 0;
    float sigma = 0;
    if (fread(&n1, 4, 1, f) != 1 || fread(&n2, 4, 1, f) != 1 || fread(&its, 4, 1, f) != 1 || fread(&sigma, 4, 1, f) != 1 || n1 < 1 || n2 < 1 || its < 1) return 2;
    std::vector<float> k1(2 * (size_t)n1), r1(3 * (size_t)n1), k2(2 * (size_t)n2), r2(3 * (size_t)n2), p3d(3 * (size_t)n1);
    std::vector<int32_t> m(n1), d(8 * (size_t)its);
    std::vector<uint8_t> tr(n1);
    if (fread(k1.data(), 4, k1.size(), f) != k1.size() || fread(r1.data(), 4, r1.size(), f) != r1.size() || fread(k2.data(), 4, k2.size(), f) != k2.size() ||
        fread(r2.data(), 4, r2.size(), f) != r2.size() || fread(m.data(), 4, m.size(), f) != m.size() || fread(d.data(), 4, d.size(), f) != d.size())
      return 2;
    cms_init_job q;
    std::memset(&q, 0, sizeof(q));
    q.n1 = n1; q.n2 = n2; q.keys1 = k1.data(); q.rays1 = r1.data(); q.keys2 = k2.data(); q.rays2 = r2.data(); q.matches12 = m.data();
    q.sigma = sigma; q.iterations = its; q.n_draws = (int)d.size(); q.draws = d.data(); q.p3d = p3d.data(); q.triangulated = tr.data();
    const int rc = hm_init_two_view_host(F, cos_fov, 1, &q);
    if (rc) { ++refused; continue; }
    ok += q.status;
    if (q.score == q.score) score += q.score;
    for (int i = 0; i < n1; ++i) tri += tr[i];
  }
  fclose(f);
  printf("%d cases, %d refused, %d initialised, %d points, sum of scores %.6g\n", count, refused, ok, tri, score);
  return 0;
}
#endif
