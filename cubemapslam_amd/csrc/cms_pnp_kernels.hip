// cms_pnp_kernels.hip -- PnPsolver::iterate (src/PnPsolver.cpp:167-343) on the device, three launches per call over all jobs (four with the gather):
//
//   k_pnp_gather       cms_pnp_iterate_frames only: pixel, key ray and level sigma2 of every correspondence from the context's resident frame rows
//   k_pnp_hypotheses   one lane per (job, hypothesis): the four draws resolved by the reference's swap-and-pop, compute_pose of cms_pnp_core.h on
//                      the four points, R | t stored as doubles.  32 lanes per workgroup; MtM and the eigenvector matrix (2 x 144 doubles per
//                      lane) live in LDS, 289 doubles apart so that the lanes of a workgroup fall on different banks
//   k_pnp_inliers      one wavefront per (job, hypothesis): CheckInliers, lanes stride over the correspondences, the 64-bit ballot is the mask
//                      word, the count is the sum of the popcounts (cms_ransac_mask_sweep of cms_ransac_core.h, as in the Refine below)
//   k_pnp_select       one workgroup per job replays the loop over its hypotheses in order: best on >, Refine on the best mask (recomputed only
//                      when the best changed since the last failed Refine -- it is a function of the mask alone), accepted on > min_inliers.  The
//                      EPnP over the best inliers is the scalar core run by the first lane on the job's scratch rows, CheckInliers behind it runs
//                      on all lanes
//
// The device is held to the host build of cms_pnp_core.h bit for bit (tests/test_gpu_pnp.py): every operation of the core is an IEEE-rounded
// + - * / sqrt on both sides (-ffp-contract=off), and the kernels add no arithmetic of their own beyond float -> double widening.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cms_pnp_core.h"
#include "cms_types.h"

#define CMS_PNP_HYP_LANES 32
#define CMS_PNP_LANE_DOUBLES 289      // 144 (MtM) + 144 (ut) + 1: 578 dwords, 2 mod 64 -- 32 lanes x 8 bytes cover the 64 banks once
#define CMS_PNP_SELECT_THREADS 256

struct CmsPnpJobDev {
  int N, H;
  int corr0;            // first correspondence in the call's arrays
  int hyp0;             // first hypothesis in the call's arrays
  int words;            // mask words per hypothesis: (N + 63) / 64
  long long word0;      // first word of the job's hypothesis masks
  int mword0;           // first word of the job's rows in the per-job mask arrays (best in, best out, refined out)
  int min_inliers, max_its, iterations, best_inliers;
  float best_Tcw[12];
};
struct CmsPnpOutDev {
  int status, no_more, n_inliers, iterations, iterations_run, best_inliers;
  float Tcw[12], best_Tcw[12];
};
struct CmsPnpArgs {
  int F, njobs, nhyp;
  const CmsPnpJobDev* jobs;
  const int* hyp_job;                  // job of every hypothesis
  const int* draws;                    // 4 per hypothesis
  const float* p3d; const float* p2d; const float* bearing; const float* max_error;
  double* hyp_Rt;                      // 12 per hypothesis
  int* hyp_count;
  unsigned long long* hyp_mask;
  const unsigned long long* best_in;   // per job `words`
  unsigned long long* best_out; unsigned long long* refined_out;
  double* refine_rows;                 // 15 doubles per correspondence: pws 3 | us 2 | bearings 3 | alphas 4 | pcs 3, job after job
  CmsPnpOutDev* out;
};

// cms_pnp_iterate_frames: mvP2D, mvBearings and mvMaxError of every correspondence from the context's resident rows (PnPsolver.cpp:91-97, :158)
struct CmsPnpGatherArgs {
  int ncorr, kp_cap, nlevels;
  const int* corr_job;                 // job of every correspondence
  const int* job_row;                  // frame row of every job
  const float* job_th2;
  const int* kp_idx;                   // mvKeyPointIndices, checked against the row's n (<= kp_cap) on the host
  const CmsKeyPoint* kps; const float* rays;
  float sigma2[16];                    // mvLevelSigma2
  float* p2d; float* bearing; float* max_error;
};
extern "C" __global__ void __launch_bounds__(256) k_pnp_gather(CmsPnpGatherArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.ncorr) return;
  const int j = a.corr_job[i];
  int k = a.kp_idx[i];
  k = k < 0 ? 0 : (k >= a.kp_cap ? a.kp_cap - 1 : k);
  const size_t r = (size_t)a.job_row[j] * a.kp_cap + (size_t)k;
  const CmsKeyPoint kp = a.kps[r];
  int o = kp.octave;
  o = o < 0 ? 0 : (o >= a.nlevels ? a.nlevels - 1 : o);
  a.p2d[2 * (size_t)i] = kp.x; a.p2d[2 * (size_t)i + 1] = kp.y;
  for (int q = 0; q < 3; ++q) a.bearing[3 * (size_t)i + q] = a.rays[3 * r + q];
  a.max_error[i] = a.sigma2[o] * a.job_th2[j];
}

extern "C" __global__ void __launch_bounds__(CMS_PNP_HYP_LANES) k_pnp_hypotheses(CmsPnpArgs a) {
  extern __shared__ double pnp_lds[];
  const int g = blockIdx.x * CMS_PNP_HYP_LANES + threadIdx.x;
  if (g >= a.nhyp) return;
  const CmsPnpJobDev& J = a.jobs[a.hyp_job[g]];
  double* mtm = pnp_lds + (size_t)threadIdx.x * CMS_PNP_LANE_DOUBLES;
  double* ut = mtm + 144;
  int idx[4];
  cms_pnp_resolve_draws(J.N, a.draws + 4 * (size_t)g, idx);
  double pws[12], us[8], bearings[12], alphas[16], pcs[12], R[9], t[3];
  for (int k = 0; k < 4; ++k) {
    const int i = idx[k] < 0 ? 0 : (idx[k] >= J.N ? J.N - 1 : idx[k]);      // the host has checked the draws; never index beyond the job
    const size_t c = (size_t)J.corr0 + (size_t)i;
    for (int j = 0; j < 3; ++j) { pws[3 * k + j] = (double)a.p3d[3 * c + j]; bearings[3 * k + j] = (double)a.bearing[3 * c + j]; }
    us[2 * k] = (double)a.p2d[2 * c]; us[2 * k + 1] = (double)a.p2d[2 * c + 1];
  }
  cms_pnp_compute_pose(4, a.F, pws, us, bearings, alphas, pcs, mtm, ut, R, t, nullptr);
  double* o = a.hyp_Rt + 12 * (size_t)g;
  for (int k = 0; k < 9; ++k) o[k] = R[k];
  for (int k = 0; k < 3; ++k) o[9 + k] = t[k];
}

extern "C" __global__ void __launch_bounds__(64) k_pnp_inliers(CmsPnpArgs a) {
  const int g = blockIdx.x, lane = threadIdx.x;
  const CmsPnpJobDev& J = a.jobs[a.hyp_job[g]];
  double R[9], t[3];
  const double* rt = a.hyp_Rt + 12 * (size_t)g;
  for (int k = 0; k < 9; ++k) R[k] = rt[k];
  for (int k = 0; k < 3; ++k) t[k] = rt[9 + k];
  unsigned long long* mask = a.hyp_mask + J.word0 + (long long)(g - J.hyp0) * J.words;
  const int count = cms_ransac_mask_sweep(J.N, J.words, 0, 1, lane, mask, [&](int i) {
    const size_t c = (size_t)J.corr0 + (size_t)i;
    return cms_pnp_is_inlier(a.F, R, t, a.p3d + 3 * c, a.p2d + 2 * c, a.max_error[c]);
  });
  if (lane == 0) a.hyp_count[g] = count;
}

extern "C" __global__ void __launch_bounds__(CMS_PNP_SELECT_THREADS) k_pnp_select(CmsPnpArgs a) {
  __shared__ double s_mtm[144], s_ut[144], s_R[9], s_t[3];
  __shared__ int s_h, s_refine, s_done, s_count, s_best_src, s_best_inliers, s_iterations, s_run, s_status, s_refined_n;
  __shared__ float s_best_T[12];
  const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const CmsPnpJobDev& J = a.jobs[j];
  const unsigned long long* best_in = a.best_in + J.mword0;
  unsigned long long* best_out = a.best_out + J.mword0;
  unsigned long long* refined_out = a.refined_out + J.mword0;
  const unsigned long long* hyp_mask = a.hyp_mask + J.word0;
  double* rows = a.refine_rows + 15 * (size_t)J.corr0;
  if (tid == 0) {
    s_h = 0; s_done = 0; s_best_src = -1; s_best_inliers = J.best_inliers; s_iterations = J.iterations; s_run = 0; s_status = 0; s_refined_n = 0;
    for (int k = 0; k < 12; ++k) s_best_T[k] = J.best_Tcw[k];
  }
  bool refine_known_to_fail = false;      // thread 0's: the last Refine was on the present best and was not accepted
  __syncthreads();
  for (;;) {
    if (tid == 0) {
      int h = s_h, need = 0;
      while (h < J.H) {
        const int cnt = a.hyp_count[J.hyp0 + h];
        s_iterations++; s_run++;
        const int me = h++;
        if (cnt >= J.min_inliers) {
          if (cnt > s_best_inliers) {
            s_best_inliers = cnt; s_best_src = me; refine_known_to_fail = false;
            const double* rt = a.hyp_Rt + 12 * (size_t)(J.hyp0 + me);
            for (int k = 0; k < 12; ++k) s_best_T[k] = (float)rt[k];
          }
          if (!refine_known_to_fail) { need = 1; break; }
        }
      }
      s_h = h; s_refine = need; s_count = 0;
      if (need) {
        // Refine (:263-309): the best inliers in index order, EPnP over all of them
        const unsigned long long* bm = s_best_src < 0 ? best_in : hyp_mask + (long long)s_best_src * J.words;
        const int cap = J.N;
        double* pws = rows; double* us = pws + 3 * (size_t)cap; double* bearings = us + 2 * (size_t)cap; double* alphas = bearings + 3 * (size_t)cap;
        double* pcs = alphas + 4 * (size_t)cap;
        int n = 0;
        for (int i = 0; i < J.N; ++i) {
          if (!((bm[i >> 6] >> (i & 63)) & 1ull)) continue;
          const size_t c = (size_t)J.corr0 + (size_t)i;
          for (int q = 0; q < 3; ++q) { pws[3 * n + q] = (double)a.p3d[3 * c + q]; bearings[3 * n + q] = (double)a.bearing[3 * c + q]; }
          us[2 * n] = (double)a.p2d[2 * c]; us[2 * n + 1] = (double)a.p2d[2 * c + 1];
          ++n;
        }
        double R[9], t[3];
        cms_pnp_compute_pose(n, a.F, pws, us, bearings, alphas, pcs, s_mtm, s_ut, R, t, nullptr);
        for (int k = 0; k < 9; ++k) s_R[k] = R[k];
        for (int k = 0; k < 3; ++k) s_t[k] = t[k];
      }
    }
    __syncthreads();
    if (!s_refine) break;
    {
      double R[9], t[3];
      for (int k = 0; k < 9; ++k) R[k] = s_R[k];
      for (int k = 0; k < 3; ++k) t[k] = s_t[k];
      const int count = cms_ransac_mask_sweep(J.N, J.words, wave, CMS_PNP_SELECT_THREADS / 64, lane, refined_out, [&](int i) {
        const size_t c = (size_t)J.corr0 + (size_t)i;
        return cms_pnp_is_inlier(a.F, R, t, a.p3d + 3 * c, a.p2d + 2 * c, a.max_error[c]);
      });
      if (lane == 0 && count) atomicAdd(&s_count, count);
    }
    __syncthreads();
    if (tid == 0) {
      if (s_count > J.min_inliers) { s_done = 1; s_status = 1; s_refined_n = s_count; }
      else refine_known_to_fail = true;
    }
    __syncthreads();
    if (s_done) break;
  }
  // the best mask as it stands (:217), for the caller's next call and for the exhausted case (:244-258)
  const unsigned long long* bm = s_best_src < 0 ? best_in : hyp_mask + (long long)s_best_src * J.words;
  for (int w = tid; w < J.words; w += CMS_PNP_SELECT_THREADS) best_out[w] = bm[w];
  if (tid == 0) {
    CmsPnpOutDev o;
    o.status = s_status; o.no_more = 0; o.n_inliers = s_refined_n; o.iterations = s_iterations; o.iterations_run = s_run; o.best_inliers = s_best_inliers;
    for (int k = 0; k < 9; ++k) o.Tcw[k] = s_status == 1 ? (float)s_R[k] : 0.0f;
    for (int k = 0; k < 3; ++k) o.Tcw[9 + k] = s_status == 1 ? (float)s_t[k] : 0.0f;
    for (int k = 0; k < 12; ++k) o.best_Tcw[k] = s_best_T[k];
    if (s_status == 0 && s_iterations >= J.max_its) {
      o.no_more = 1;
      if (s_best_inliers >= J.min_inliers) o.status = 2;      // the host hands out mBestTcw and the best mask
    }
    a.out[j] = o;
  }
}
