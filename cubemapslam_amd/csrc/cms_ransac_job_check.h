// cms_ransac_job_check.h -- the rules the job checks of the PnP, Sim3 and two-view solvers share (cms_{pnp,sim3,init}_job_check.h), the iteration
// count of the two SetRansacParameters and the byte <-> bit form of an inlier mask.  Host code without HIP (tests/emu/ransac_common_emu.cpp builds
// it with g++).  Needs the CMS_* codes (include/cubemapslam_hip.h) before it.
#ifndef CMS_RANSAC_JOB_CHECK_H
#define CMS_RANSAC_JOB_CHECK_H
#include <climits>
#include <cmath>
#include <cstdint>

// The counters of a cms_pnp_job / cms_sim3_job stay far from int's end; min_inliers never lies below the minimal set
template <class Job>
static inline int cms_ransac_check_counters(const Job& q, int min_set) {
  if (q.min_inliers < min_set || q.max_its < 0 || q.max_its > (1 << 20) || q.n_iterations < 0 || q.n_iterations > (1 << 20) || q.iterations > (1 << 30)) return CMS_ERR_ARG;
  if (q.N < 0 || q.n_draws < 0 || q.iterations < 0 || q.best_inliers < 0 || q.best_inliers > q.N) return CMS_ERR_ARG;
  return CMS_OK;
}

// The hypotheses of one call from left = max_its - iterations and n_iterations: H_max = max(left, n_iterations) is what a loop on
// `iterations < max_its || current < n_iterations` runs, H_min = min(left, n_iterations) what a loop on `&&` runs; neither below 0, and both 0
// when N < min_inliers (the solvers return before the loop)
static inline void cms_ransac_hypotheses(int N, int min_inliers, int max_its, int iterations, int n_iterations, int* H_max, int* H_min) {
  *H_max = 0; *H_min = 0;
  if (N < min_inliers) return;
  const int left = max_its - iterations;
  *H_max = left > n_iterations ? left : n_iterations;
  *H_min = left < n_iterations ? left : n_iterations;
  if (*H_max < 0) *H_max = 0;
  if (*H_min < 0) *H_min = 0;
}

// K draws for each of H iterations, draws[K*i + k] in [0, N - 1 - k]: what cms_ransac_resolve_draws (cms_ransac_core.h) turns into indices < N
static inline int cms_ransac_check_draws(const int* draws, int n_draws, int H, int K, int N) {
  if (H > 0 && ((long long)n_draws < (long long)K * H || !draws)) return CMS_ERR_ARG;
  for (int i = 0; i < H; ++i)
    for (int k = 0; k < K; ++k)
      if (draws[K * i + k] < 0 || draws[K * i + k] > N - 1 - k) return CMS_ERR_ARG;
  return CMS_OK;
}

// the carried-in best mask has best_inliers bytes set
static inline int cms_ransac_check_best_mask(const uint8_t* mask, int N, int best_inliers) {
  int nb = 0;
  for (int i = 0; i < N; ++i) nb += mask[i] ? 1 : 0;
  return nb == best_inliers ? CMS_OK : CMS_ERR_ARG;
}

// nIterations of SetRansacParameters (PnPsolver.cpp:147, Sim3Solver.cpp:155): ceil(log(1 - p) / log(1 - epsilon^3)) in double, then the
// conversion to int as the reference's build does it: INT_MIN is what cvttsd2si leaves for NaN and for values no int holds
static inline int cms_ransac_iterations(double probability, float epsilon) {
  const double v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3.0)));
  return (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : INT_MIN;
}

// An inlier mask of N bytes as (N + 63) / 64 words, bit i & 63 of word i >> 6.  Packing ORs into words the caller has zeroed; unpacking writes
// exactly 0 or 1 into the first N bytes.
static inline void cms_mask_pack(const uint8_t* bytes, int N, unsigned long long* words) {
  for (int i = 0; i < N; ++i)
    if (bytes[i]) words[i >> 6] |= 1ull << (i & 63);
}
static inline void cms_mask_unpack(const unsigned long long* words, int N, uint8_t* bytes) {
  for (int i = 0; i < N; ++i) bytes[i] = (uint8_t)((words[i >> 6] >> (i & 63)) & 1ull);
}

#endif
