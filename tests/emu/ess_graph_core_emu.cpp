// ess_graph_core_emu.cpp -- a stand-alone program (its own main) over the host loop of Optimizer::OptimizeEssentialGraph
// (cubemapslam_amd/host/ess_graph_host.cpp with csrc/cms_ess_graph_core.h), for the host sanitizers: tests/test_essential_graph_cpu.py builds it with
// -fsanitize=address,undefined and runs it once on one job.  Every buffer has exactly the size the call may touch.
//   input   (file argv[1]) int N, fixed, E, fix_scale, iterations; double lambda_init; N x 8 doubles Scw; N x 8 doubles Snc; E x 3 ints
//   output  (stdout) rc, the scalar outputs and every double of S_out / float of Tiw_out as its bit pattern
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../cubemapslam_amd/host/ess_graph_host.cpp"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int hdr[5];
  double lambda;
  if (std::fread(hdr, sizeof(int), 5, f) != 5 || std::fread(&lambda, sizeof(double), 1, f) != 1) return 2;
  const size_t N = (size_t)hdr[0], E = (size_t)hdr[2];
  std::vector<double> Scw(8 * N), Snc(8 * N), S_out(8 * N);
  std::vector<int> edges(3 * E);
  std::vector<float> Tiw(12 * N);
  if (std::fread(Scw.data(), 8, 8 * N, f) != 8 * N || std::fread(Snc.data(), 8, 8 * N, f) != 8 * N || std::fread(edges.data(), 4, 3 * E, f) != 3 * E) return 2;
  std::fclose(f);
  cms_ess_graph_job q = {};
  q.N = hdr[0]; q.fixed = hdr[1]; q.E = hdr[2]; q.fix_scale = hdr[3]; q.iterations = hdr[4]; q.lambda_init = lambda;
  q.Scw = Scw.data(); q.Snc = Snc.data(); q.edges = edges.data(); q.S_out = S_out.data(); q.Tiw_out = Tiw.data();
  const int rc = hm_essential_graph_optimize_host(1, &q);
  std::printf("%d %d %d %d", rc, q.iterations_run, q.trials_run, q.flags);
  auto bits = [](double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; };
  std::printf(" %016" PRIx64 " %016" PRIx64 " %016" PRIx64, bits(q.chi2_initial), bits(q.chi2_final), bits(q.lambda_final));
  for (double v : S_out) std::printf(" %016" PRIx64, bits(v));
  for (float v : Tiw) { uint32_t b; std::memcpy(&b, &v, 4); std::printf(" %08" PRIx32, b); }
  std::printf("\n");
  return 0;
}
