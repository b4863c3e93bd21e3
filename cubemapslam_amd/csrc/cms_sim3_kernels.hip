// cms_sim3_kernels.hip -- Sim3Solver::iterate (src/Sim3Solver.cpp:164-231) on the device, two launches per call over all jobs:
//
//   k_sim3_hypotheses  one wavefront per (job, hypothesis).  Every lane resolves the three draws by the reference's swap-and-pop and runs
//                      compute_sim3 of cms_sim3_core.h on the three pairs: the solve is a few dozen floats of state and no memory, the lanes
//                      do the same operations on the same values, so the wavefront holds T12 / T21 in registers without a second launch or a
//                      round trip through memory (lane 0 stores R, t, s, T12 for the replay).  Then CheckInliers: lanes stride over the
//                      correspondences, the 64-bit ballot is the mask word, the count is the sum of the popcounts (cms_ransac_mask_sweep of
//                      cms_ransac_core.h)
//   k_sim3_select      one wavefront per job replays the loop over its hypotheses in order.  There is no Refine, so the replay is a prefix
//                      maximum over the counts in chunks of 64, seeded with the carried-in best: hypothesis h replaces the best when
//                      count[h] >= the maximum before it, and the call ends at the first such h with count[h] > min_inliers
//
// The device is held to the host build of cms_sim3_core.h bit for bit (tests/test_gpu_sim3.py): every operation of the core is an IEEE-rounded
// + - * / sqrt on both sides (-ffp-contract=off), and the kernels add no arithmetic of their own.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cms_sim3_core.h"

struct CmsSim3JobDev {
  int N, H;             // H: the hypotheses this call evaluates (H_run of cms_sim3_job_check.h)
  int corr0;            // first correspondence in the call's arrays
  int hyp0;             // first hypothesis in the call's arrays
  int words;            // mask words per hypothesis: (N + 63) / 64
  long long word0;      // first word of the job's hypothesis masks
  int mword0;           // first word of the job's rows in the per-job mask arrays (best in, best out)
  int fix_scale, min_inliers, max_its, iterations, best_inliers;
  float best[25];       // R 9 | t 3 | s 1 | T12 12
};
struct CmsSim3OutDev {
  int status, no_more, n_inliers, iterations, iterations_run, best_inliers;
  float best[25];
};
struct CmsSim3Args {
  int F, njobs, nhyp;
  const CmsSim3JobDev* jobs;
  const int* hyp_job;                  // job of every hypothesis
  const int* draws;                    // 3 per hypothesis
  const float* x1; const float* x2; const float* me1; const float* me2;
  float* hyp_motion;                   // 25 per hypothesis: R 9 | t 3 | s 1 | T12 12
  int* hyp_count;
  unsigned long long* hyp_mask;
  const unsigned long long* best_in;   // per job `words`
  unsigned long long* best_out;
  CmsSim3OutDev* out;
};

extern "C" __global__ void __launch_bounds__(64) k_sim3_hypotheses(CmsSim3Args a) {
  const int g = blockIdx.x, lane = threadIdx.x;
  if (g >= a.nhyp) return;
  const CmsSim3JobDev& J = a.jobs[a.hyp_job[g]];
  int idx[3];
  cms_sim3_resolve_draws(J.N, a.draws + 3 * (size_t)g, idx);
  float P1[9], P2[9];
  for (int k = 0; k < 3; ++k) {
    const int i = idx[k] < 0 ? 0 : (idx[k] >= J.N ? J.N - 1 : idx[k]);      // the host has checked the draws; never index beyond the job
    const size_t c = (size_t)J.corr0 + (size_t)i;
    for (int q = 0; q < 3; ++q) { P1[3 * k + q] = a.x1[3 * c + q]; P2[3 * k + q] = a.x2[3 * c + q]; }
  }
  CmsSim3Motion m;
  cms_sim3_compute(P1, P2, J.fix_scale, &m, nullptr);
  if (lane == 0) {
    float* o = a.hyp_motion + 25 * (size_t)g;
    for (int k = 0; k < 9; ++k) o[k] = m.R[k];
    for (int k = 0; k < 3; ++k) o[9 + k] = m.t[k];
    o[12] = m.s;
    for (int k = 0; k < 12; ++k) o[13 + k] = m.T12[k];
  }
  unsigned long long* mask = a.hyp_mask + J.word0 + (long long)(g - J.hyp0) * J.words;
  const int count = cms_ransac_mask_sweep(J.N, J.words, 0, 1, lane, mask, [&](int i) {
    const size_t c = (size_t)J.corr0 + (size_t)i;
    return cms_sim3_is_inlier(a.F, m.T12, m.T21, a.x1 + 3 * c, a.x2 + 3 * c, a.me1[c], a.me2[c]);
  });
  if (lane == 0) a.hyp_count[g] = count;
}

extern "C" __global__ void __launch_bounds__(64) k_sim3_select(CmsSim3Args a) {
  const int j = blockIdx.x, lane = threadIdx.x;
  if (j >= a.njobs) return;
  const CmsSim3JobDev& J = a.jobs[j];
  int best = J.best_inliers;      // the maximum before the chunk (wave-uniform)
  int best_src = -1, accepted = -1;
  for (int base = 0; base < J.H && accepted < 0; base += 64) {
    const int h = base + lane;
    const bool live = h < J.H;
    const int cnt = live ? a.hyp_count[J.hyp0 + h] : -1;
    int incl = cnt;
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(incl, d, 64);
      if (lane >= d && v > incl) incl = v;
    }
    int before = __shfl_up(incl, 1, 64);
    if (lane == 0 || before < best) before = best;
    const bool replaces = live && cnt >= before;                           // :207
    const unsigned long long acc = __ballot(replaces && cnt > J.min_inliers);      // :216
    unsigned long long rep = __ballot(replaces);
    if (acc) {
      const int first = __ffsll((long long)acc) - 1;
      accepted = base + first;
      rep &= first == 63 ? ~0ull : ((1ull << (first + 1)) - 1ull);
    }
    if (rep) best_src = base + 63 - __clzll((long long)rep);
    const int chunk_max = __shfl(incl, 63, 64);
    if (chunk_max > best) best = chunk_max;
  }
  const int run = accepted >= 0 ? accepted + 1 : J.H;
  const int best_inliers = best_src >= 0 ? a.hyp_count[J.hyp0 + best_src] : J.best_inliers;
  // the best mask as it stands (:209): the winner's on status 1, else for the caller's next call
  const unsigned long long* bm = best_src < 0 ? a.best_in + J.mword0 : a.hyp_mask + J.word0 + (long long)best_src * J.words;
  unsigned long long* bo = a.best_out + J.mword0;
  for (int w = lane; w < J.words; w += 64) bo[w] = bm[w];
  CmsSim3OutDev* o = a.out + j;
  const float* src = best_src < 0 ? J.best : a.hyp_motion + 25 * (size_t)(J.hyp0 + best_src);
  if (lane < 25) o->best[lane] = src[lane];
  if (lane == 0) {
    const int iterations = J.iterations + run;
    o->status = accepted >= 0 ? 1 : 0;
    o->n_inliers = accepted >= 0 ? best_inliers : 0;
    o->iterations = iterations; o->iterations_run = run; o->best_inliers = best_inliers;
    o->no_more = (accepted < 0 && iterations >= J.max_its) ? 1 : 0;
  }
}
