// cms_ransac_core.h -- what the RANSAC loops of PnPsolver, Sim3Solver and the Initializer share on both sides: the draws of one iteration, ONE
// source for the host builds (libcubemapslam_host.so, tests/emu/ransac_common_emu.cpp) and for the gfx950 kernels, and, under hipcc only, the
// inlier sweep of a wavefront.  Compiles under g++ as it stands; included by cms_{pnp,sim3,init}_core.h.
#ifndef CMS_RANSAC_CORE_H
#define CMS_RANSAC_CORE_H
#include "cms_detmath.h"      // CMS_HD

#if defined(__HIPCC__)
#define CMS_RANSAC_UNROLL _Pragma("unroll")
#else
#define CMS_RANSAC_UNROLL
#endif

// The K draws of one iteration (PnPsolver.cpp:190-204, Sim3Solver.cpp:190-201, Initializer.cpp:92-107): idx = avail[randi]; avail[randi] =
// avail.back(); pop -- without the array of N: at most K places differ from the identity.  draws[k] must lie in [0, N - 1 - k] (the callers
// check).  Both loops run to K with `q < k` as a predicate, so they unroll fully and pos / val stay in registers.
template <int K>
CMS_HD void cms_ransac_resolve_draws(int N, const int* draws, int* idx) {
  int pos[K], val[K];
  CMS_RANSAC_UNROLL
  for (int k = 0; k < K; ++k) {
    const int size = N - k, r = draws[k], last = size - 1;
    int vr = r, vl = last;
    CMS_RANSAC_UNROLL
    for (int q = 0; q < K; ++q) {      // later entries override earlier ones
      if (q < k && pos[q] == r) vr = val[q];
      if (q < k && pos[q] == last) vl = val[q];
    }
    idx[k] = vr;
    pos[k] = r;
    val[k] = vl;
  }
}

#if defined(__HIPCC__)
// CheckInliers of one wavefront over the mask words first_word, first_word + word_step, ... < words: lane l of word w tests correspondence
// 64 w + l with is_inlier(i) (never called for i >= N), the 64-bit ballot is the mask word, and the sum of the popcounts comes back
// (wave-uniform).
template <class IsInlier>
__device__ inline int cms_ransac_mask_sweep(int N, int words, int first_word, int word_step, int lane, unsigned long long* mask, IsInlier is_inlier) {
  int count = 0;
  for (int w = first_word; w < words; w += word_step) {
    const int i = w * 64 + lane;
    bool in = false;
    if (i < N) in = is_inlier(i);
    const unsigned long long b = __ballot(in);
    if (lane == 0) mask[w] = b;
    count += __popcll(b);
  }
  return count;
}
#endif

#endif
