// cms_sim3_opt_kernels.hip -- Optimizer::OptimizeSim3 (src/Optimizer.cpp:888-1091) on the device: ONE launch for all jobs of a call, one
// workgroup of 256 threads per job, both optimize() rounds with the Levenberg accept / reject loop and the two classifications inside the kernel
// (the shape of k_pose_optimize_g, cms_pose_opt.hip).  Loop closing is a rare event: there is one variant, with the pairs' persistent errors in
// global memory.
//
//   thread 0          owns the Levenberg state (a CmsS3oLM of its own, as k_pose_optimize_g keeps its state), the exponential of a trial and the
//                     7 x 7 solve; what the other threads need of it -- the estimate, the trial, the trial's inverse -- it copies to LDS
//   threads 0..13     make the fourteen perturbed estimates of a numeric linearisation (CmsS3oLin in LDS), one each
//   all threads       share the edge passes: thread t takes pairs t, t + 256, ... in ascending order, so its 36 running sums ARE slot t of the
//                     core's summation contract.  The slots are folded as cms_s3o_tree says: a xor butterfly inside each wavefront (the same
//                     additions as the tree's, addition commutes), then (w0 + w1) + (w2 + w3) through LDS.  A trial's chi2 takes the same way
//
// In the as-written mode a pair costs 2 + 28 error evaluations per linearisation.  By design one wavefront per SIMD: a job is one 256-thread workgroup.
// The device is held to the host build of cms_sim3_opt_core.h bit for bit (tests/test_gpu_sim3_opt.py): every operation is an IEEE-rounded
// + - * / sqrt of the core (-ffp-contract=off), no device library function is called, and this file adds no arithmetic of its own.
// Why the Levenberg state is NOT in LDS: with `__shared__ CmsS3oLM` the compiler's binary is deterministic and not the host's function; an empty
// asm with a memory clobber behind cms_s3o_lm_begin -- no instruction -- gives the host's bits, so does the private state.  The LDS form is right at -O1 and wrong at -O2 / -O3, also with -fno-strict-aliasing
// (DESIGN.md "OptimizeSim3"); host g++, host clang and the numpy restatement agree with the right one.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cms_sim3_opt_core.h"

struct CmsS3oJobDev {
  int N, corr0, fix_scale, jacobian;
  float th2; int pad;
  double R[9], t[3], s;
};
struct CmsS3oOutDev {
  int n_inliers, n_correspondences, n_bad, its[2], pad;
  double q[4], t[3], s;
};
struct CmsS3oArgs {
  int F, njobs;
  const CmsS3oJobDev* jobs;
  const float* x1; const float* x2; const float* kp1; const float* kp2; const float* is1; const float* is2;
  double* err;          // 4 per correspondence: the persistent _error of e12 | e21
  uint8_t* keep;        // per correspondence; also "the pair's edges are still in the graph"
  CmsS3oOutDev* out;
};

// the fold of cms_s3o_tree over the workgroup's slots; the result is valid in every thread
__device__ __forceinline__ double s3o_block_sum1(double v, double* sh4) {
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
  __syncthreads();                       // previous readers of sh4 are done
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh4[0] + sh4[1]) + (sh4[2] + sh4[3]);
}
__device__ __forceinline__ int s3o_block_sum_int(int v, int* sh4) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh4[0] + sh4[1] + sh4[2] + sh4[3];
}

extern "C" __global__ void __launch_bounds__(256) k_sim3_optimize(CmsS3oArgs a) {
  CmsS3oLM lm;                                               // thread 0's own, as k_pose_optimize_g keeps its Levenberg state; unused elsewhere
  __shared__ CmsS3oLin lin;
  __shared__ CmsS3 s_S, s_trial, s_tinv;                     // what the other threads see of it: the estimate, the trial, the trial's inverse
  __shared__ double sh36[4][CMS_SIM3_OPT_ACC], sum[CMS_SIM3_OPT_ACC], sh4[4];
  __shared__ int s_ctl[2], s_int[4];
  const int j = blockIdx.x, tid = threadIdx.x;
  if (j >= a.njobs) return;
  const CmsS3oJobDev& J = a.jobs[j];
  const int N = J.N, F = a.F, mode = J.jacobian, fix_scale = J.fix_scale;
  const size_t c0 = (size_t)J.corr0;
  const float th2 = J.th2;
  const double delta = cms_s3o_huber_delta(th2);
  CmsS3oOutDev* out = a.out + j;
  for (int k = tid; k < N; k += 256) a.keep[c0 + k] = 1;
  if (tid == 0) {
    CmsS3 S0;
    cms_s3o_from_Rts(J.R, J.t, J.s, &S0);
    lm.S = S0; lm.trial = S0; lm.fix_scale = fix_scale; s_S = S0;
    lm.lambda = 0; lm.ni = 2; lm.currentChi = 0; lm.iniChi = 0; lm.rho = 0; lm.scale = 0; lm.nBad = 0; lm.qmax = 0; lm.ok2 = 0;
  }
  __syncthreads();
  int its[2] = {0, 0}, nBad = 0, n_in = 0;
  bool early = false;
  for (int round = 0; round < 2; ++round) {
    const int iterations = round == 0 ? 5 : cms_s3o_more_iterations(nBad);
    int done = 0;
    for (int it = 0; it < iterations && N > 0; ++it) {
      // ---- what the linearisation shares: the estimate, its inverse, the fourteen perturbed estimates
      if (tid == 0) cms_s3o_lin_base(lm.S, &lin);
      if (mode == CMS_SIM3_OPT_AS_WRITTEN && tid < 14) cms_s3o_lin_perturb(s_S, fix_scale, tid, &lin);
      __syncthreads();
      // ---- computeActiveErrors + activeRobustChi2 + buildSystem
      double acc[CMS_SIM3_OPT_ACC];
#pragma unroll
      for (int i = 0; i < CMS_SIM3_OPT_ACC; ++i) acc[i] = 0;
      for (int k = tid; k < N; k += 256) {
        const size_t c = c0 + (size_t)k;
        if (!a.keep[c]) continue;
        CmsS3oPair p;
        cms_s3o_pair_setup(F, a.x1 + 3 * c, a.x2 + 3 * c, a.kp1 + 2 * c, a.kp2 + 2 * c, a.is1[c], a.is2[c], &p);
        double e[4], J12[14], J21[14];
        cms_s3o_errors(F, p, lin.S, lin.Sinv, e);
        for (int i = 0; i < 4; ++i) a.err[4 * c + i] = e[i];
        cms_s3o_pair_jac(F, mode, fix_scale, p, lin, J12, J21);
        cms_s3o_edge_accumulate(J12, e, p.om1, delta, acc);
        cms_s3o_edge_accumulate(J21, e + 2, p.om2, delta, acc);
      }
#pragma unroll
      for (int i = 0; i < CMS_SIM3_OPT_ACC; ++i) {
        double v = acc[i];
        for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
        acc[i] = v;
      }
      __syncthreads();                   // previous readers of sh36 / sum are done
      if ((tid & 63) == 0) {
#pragma unroll
        for (int i = 0; i < CMS_SIM3_OPT_ACC; ++i) sh36[tid >> 6][i] = acc[i];
      }
      __syncthreads();
      if (tid < CMS_SIM3_OPT_ACC) sum[tid] = (sh36[0][tid] + sh36[1][tid]) + (sh36[2][tid] + sh36[3][tid]);
      __syncthreads();
      if (tid == 0) cms_s3o_lm_begin(&lm, sum, it);
      for (;;) {   // do { } while (rho < 0 && qmax < 10)
        if (tid == 0) {
          cms_s3o_lm_trial(&lm);
          s_trial = lm.trial;
          cms_s3o_inverse(lm.trial, &s_tinv);
        }
        __syncthreads();
        // ---- computeActiveErrors at the trial: the stored errors ARE the trial's from here on (kept on rejection, g2o)
        double chi = 0;
        for (int k = tid; k < N; k += 256) {
          const size_t c = c0 + (size_t)k;
          if (!a.keep[c]) continue;
          CmsS3oPair p;
          cms_s3o_pair_setup(F, a.x1 + 3 * c, a.x2 + 3 * c, a.kp1 + 2 * c, a.kp2 + 2 * c, a.is1[c], a.is2[c], &p);
          double e[4];
          cms_s3o_errors(F, p, s_trial, s_tinv, e);
          for (int i = 0; i < 4; ++i) a.err[4 * c + i] = e[i];
          cms_s3o_pair_chi(p, e, delta, &chi);
        }
        const double tempChi = s3o_block_sum1(chi, sh4);
        if (tid == 0) { s_ctl[0] = cms_s3o_lm_judge(&lm, tempChi) ? 1 : 0; s_S = lm.S; }
        __syncthreads();
        if (!s_ctl[0]) break;
      }
      ++done;
      if (tid == 0) s_ctl[1] = cms_s3o_lm_stop(&lm) ? 1 : 0;
      __syncthreads();
      if (s_ctl[1]) break;
    }
    its[round] = done;
    // ---- :1036-1053 / :1070-1084 on the stored errors (each thread reads what it wrote itself)
    int bad = 0;
    for (int k = tid; k < N; k += 256) {
      const size_t c = c0 + (size_t)k;
      if (!a.keep[c]) continue;
      CmsS3oPair p;
      cms_s3o_pair_setup(F, a.x1 + 3 * c, a.x2 + 3 * c, a.kp1 + 2 * c, a.kp2 + 2 * c, a.is1[c], a.is2[c], &p);
      double e[4];
      for (int i = 0; i < 4; ++i) e[i] = a.err[4 * c + i];
      if (cms_s3o_pair_is_bad(p, e, th2)) { a.keep[c] = 0; ++bad; }
    }
    bad = s3o_block_sum_int(bad, s_int);
    if (round == 0) {
      nBad = bad;
      if (N - nBad < 10) { early = true; break; }      // :1061
    } else {
      n_in = N - nBad - bad;
    }
  }
  if (tid == 0) {
    CmsS3 S;
    if (early) cms_s3o_from_Rts(J.R, J.t, J.s, &S); else S = lm.S;
    out->n_inliers = early ? 0 : n_in; out->n_correspondences = N; out->n_bad = nBad; out->its[0] = its[0]; out->its[1] = its[1]; out->pad = 0;
    for (int i = 0; i < 4; ++i) out->q[i] = cms_s3o_canon(S.q[i]);
    for (int i = 0; i < 3; ++i) out->t[i] = cms_s3o_canon(S.t[i]);
    out->s = cms_s3o_canon(S.s);
  }
}
