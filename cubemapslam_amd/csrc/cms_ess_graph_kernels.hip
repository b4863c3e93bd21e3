// cms_ess_graph_kernels.hip -- Optimizer::OptimizeEssentialGraph (src/Optimizer.cpp:623-886) on the device: ONE launch for all jobs of a call, one
// workgroup of 1024 threads per job, the whole optimize(iterations) with the Levenberg accept / reject loop inside the kernel (the shape of
// k_sim3_optimize), and k_sim3_correct_points, one thread per map point.
//
//   every phase        is a function of (work record, task index) of cms_ess_graph_core.h; the kernel spreads a phase's tasks over the workgroup
//                      (task t, t + 1024, ...) and separates dependent phases by a barrier, the host loop runs the tasks one after the other.  A
//                      task writes only its own words, so the order of the tasks of a phase does not matter and this file adds no arithmetic
//   edge-parallel      measurements, errors, the fourteen Jacobian columns of an edge's two vertices
//   vertex-parallel    perturbed estimates, the gathers of the diagonal / off-diagonal sums and of b (one task per entry), trial estimates
//   the factorisation  one barrier-separated step per pivot: thread 0 factors the 7 x 7 diagonal block in LDS, the rows of the column's blocks are
//                      scaled (7 tasks per block), the trailing blocks take their outer products (49 tasks per block pair).  A pivot whose column
//                      is empty costs no barrier
//   substitution       by rows, forwards and backwards; seven lanes (forwards) or seven per block (backwards) per row
//   sums               chi2 and the scale sum: thread t < 256 IS slot t (items t, t + 256, ...), folded as cms_s3o_tree says by a xor butterfly in
//                      each of the first four wavefronts and (w0 + w1) + (w2 + w3) through LDS
//   thread 0           owns the Levenberg scalars in registers (a CmsS3oLM of its own, as k_sim3_optimize keeps it and for its reason); what the
//                      others need -- lambda, the solve's verdict, accept / again / stop -- it hands over through LDS
// The envelope, the Jacobians and the vectors live in the handle's global scratch; LDS holds the reduction words, the pivot block and the control
// words: nothing in LDS is sized by a job's N.  No cooperative launch, no inter-workgroup waits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cms_ess_graph_core.h"

#define CMS_EG_THREADS 1024

// v[0..n) through the slots and the tree; the result is valid in every thread.  Starts with a barrier: v was written by other threads
__device__ __forceinline__ double eg_slot_sum(const double* v, int n, double* sh4) {
  __syncthreads();
  const int tid = threadIdx.x;
  double s = 0;
  if (tid < CMS_SIM3_OPT_SLOTS)
    for (int k = tid; k < n; k += CMS_SIM3_OPT_SLOTS) s += v[k];
  for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
  if ((tid & 63) == 0 && tid < CMS_SIM3_OPT_SLOTS) sh4[tid >> 6] = s;
  __syncthreads();
  const double r = (sh4[0] + sh4[1]) + (sh4[2] + sh4[3]);
  __syncthreads();                       // sh4 may be written again
  return r;
}

extern "C" __global__ void __launch_bounds__(CMS_EG_THREADS) k_ess_graph_optimize(const CmsEgWork* works, int njobs) {
  CmsS3oLM lm;                           // thread 0's own; unused elsewhere
  __shared__ double sh4[4], s_piv[49], s_D[7], s_RD[7], s_lambda;
  __shared__ int s_ctl[4];               // again, accepted, solve ok, stop
  if ((int)blockIdx.x >= njobs) return;
  const CmsEgWork w = works[blockIdx.x];
  const int tid = threadIdx.x, N = w.N, E = w.E, Nf = w.Nf;
  const long long nH = 49 * w.B;
  for (int v = tid; v < N; v += CMS_EG_THREADS) { w.S[v] = w.Scw[v]; w.T[v] = w.Scw[v]; }
  for (int e = tid; e < E; e += CMS_EG_THREADS) cms_eg_phase_measure(w, e);
  __syncthreads();
  for (int e = tid; e < E; e += CMS_EG_THREADS) cms_eg_phase_error(w, w.S, e);
  const double chi0 = eg_slot_sum(w.chi, E, sh4);
  int done = 0, trials = 0, flags = 0;
  if (tid == 0) {
    lm.lambda = w.lambda_init; lm.ni = 2; lm.currentChi = chi0; lm.iniChi = chi0; lm.rho = 0; lm.scale = 0; lm.nBad = 0; lm.qmax = 0; lm.ok2 = 0; lm.fix_scale = w.fix_scale;
    lm.S = w.Scw[0]; lm.trial = w.Scw[0];
  }
  for (int it = 0; it < w.iterations && Nf > 0 && E > 0; ++it) {
    for (int t = tid; t < 14 * N; t += CMS_EG_THREADS) cms_eg_phase_perturb(w, t);
    for (int e = tid; e < E; e += CMS_EG_THREADS) cms_eg_phase_error(w, w.S, e);
    for (long long t = tid; t < nH; t += CMS_EG_THREADS) w.H[t] = 0;
    const double c = eg_slot_sum(w.chi, E, sh4);       // (its barriers also stand behind the perturbed estimates and the zeroed H)
    for (int t = tid; t < 14 * E; t += CMS_EG_THREADS) cms_eg_phase_jacobian(w, t);
    __syncthreads();
    for (int t = tid; t < 49 * Nf; t += CMS_EG_THREADS) cms_eg_phase_assemble(w, t);
    if (tid == 0) cms_eg_lm_begin(&lm, c, it, w.lambda_init);
    for (;;) {
      if (tid == 0) s_lambda = lm.lambda;
      __syncthreads();                   // also behind the assembly
      const double lambda = s_lambda;
      for (long long t = tid; t < nH; t += CMS_EG_THREADS) w.L[t] = w.H[t];
      for (int t = tid; t < 7 * Nf; t += CMS_EG_THREADS) w.x[t] = w.b[t];
      __syncthreads();
      for (int t = tid; t < 7 * Nf; t += CMS_EG_THREADS) cms_eg_phase_damp(w, lambda, t);
      __syncthreads();
      // ---- the factorisation, pivot by pivot
      bool ok = true;
      for (int j = 0; j < Nf; ++j) {
        if (tid == 0) {
          double* Ljj = cms_eg_block(w.L, w, j, j);
          for (int i = 0; i < 49; ++i) s_piv[i] = Ljj[i];
          if (!cms_eg_factor7(s_piv, s_D, s_RD)) ok = false;
          for (int i = 0; i < 49; ++i) Ljj[i] = s_piv[i];
          for (int i = 0; i < 7; ++i) { w.D[7 * j + i] = s_D[i]; w.RD[7 * j + i] = s_RD[i]; }
        }
        const int ncol = w.colp[j + 1] - w.colp[j];
        if (ncol == 0) continue;
        __syncthreads();
        for (int t = tid; t < 7 * ncol; t += CMS_EG_THREADS) cms_eg_phase_scale(w, j, s_piv, s_D, s_RD, t);
        __syncthreads();
        const long long nt = 49LL * ncol * ncol;
        for (long long t = tid; t < nt; t += CMS_EG_THREADS) cms_eg_phase_trail(w, j, s_D, ncol, t);
        __syncthreads();
      }
      if (tid == 0) s_ctl[2] = ok ? 1 : 0;
      __syncthreads();
      // ---- substitution by rows
      for (int i = 0; i < Nf; ++i) {
        if (w.first[i] < i) {
          if (tid < 7) cms_eg_phase_fwd_off(w, i, tid);
          __syncthreads();
        }
        if (tid == 0) cms_eg_phase_fwd_diag(w, i);
        __syncthreads();
      }
      for (int t = tid; t < 7 * Nf; t += CMS_EG_THREADS) cms_eg_phase_dscale(w, t);
      __syncthreads();
      for (int k = Nf - 1; k >= 0; --k) {
        if (tid == 0) cms_eg_phase_back_diag(w, k);
        const int nt = 7 * (k - w.first[k]);
        __syncthreads();
        if (nt == 0) continue;
        for (int t = tid; t < nt; t += CMS_EG_THREADS) cms_eg_phase_back_off(w, k, t);
        __syncthreads();
      }
      const int ok2 = s_ctl[2];
      if (!ok2) {
        flags |= CMS_EG_FLAG_SOLVE;
        for (int t = tid; t < 7 * Nf; t += CMS_EG_THREADS) w.x[t] = 0;
        __syncthreads();
      }
      for (int f = tid; f < Nf; f += CMS_EG_THREADS) cms_eg_phase_trial(w, lambda, f);
      const double scale = eg_slot_sum(w.sc, Nf, sh4);
      for (int e = tid; e < E; e += CMS_EG_THREADS) cms_eg_phase_error(w, w.T, e);
      const double tc = eg_slot_sum(w.chi, E, sh4);
      if (tid == 0) {
        bool accepted;
        s_ctl[0] = cms_eg_lm_judge(&lm, tc, scale, ok2, &accepted) ? 1 : 0;
        s_ctl[1] = accepted ? 1 : 0;
      }
      ++trials;
      __syncthreads();
      const int again = s_ctl[0];
      if (s_ctl[1])
        for (int v = tid; v < N; v += CMS_EG_THREADS) if (v != w.fixed) w.S[v] = w.T[v];
      __syncthreads();
      if (!again) break;
    }
    ++done;
    if (tid == 0) { s_ctl[3] = cms_s3o_lm_stop(&lm) ? 1 : 0; if (s_ctl[3]) flags |= cms_eg_stop_flags(&lm); }
    __syncthreads();
    if (s_ctl[3]) break;
  }
  __syncthreads();
  for (int v = tid; v < N; v += CMS_EG_THREADS) cms_eg_phase_out(w, v);
  if (tid == 0) {
    CmsEgOut o;
    o.chi2_initial = cms_s3o_canon(chi0); o.chi2_final = cms_s3o_canon(lm.currentChi); o.lambda_final = cms_s3o_canon(lm.lambda);
    o.iterations_run = done; o.trials_run = trials; o.flags = flags; o.pad = 0;
    *w.out = o;
  }
}

struct CmsEgPointArgs {
  int n;
  const float* pos_in; const int* ref; const CmsS3* S_old; const CmsS3* S_new; float* pos_out;
};
extern "C" __global__ void __launch_bounds__(256) k_sim3_correct_points(CmsEgPointArgs a) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= a.n) return;
  const int r = a.ref[k];
  if (r < 0) { for (int i = 0; i < 3; ++i) a.pos_out[3 * k + i] = a.pos_in[3 * k + i]; return; }
  cms_eg_correct_point(a.pos_in + 3 * k, a.S_old[r], a.S_new[r], a.pos_out + 3 * k);
}
