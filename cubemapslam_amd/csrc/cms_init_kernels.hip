// cms_init_kernels.hip -- Initializer::InitializeWithRays (src/Initializer.cpp:53-521) on the device, three launches per call over all jobs (four with
// the gather).  The matches of a call lie job after job in parallel arrays (ray and key point of either frame, key point index of frame 1):
//
//   k_init_gather       cms_init_two_view_frames only: key point and key ray of frame 2 of every match from the context's resident frame rows
//   k_init_hypotheses   one lane per (job, iteration): the eight draws resolved by the reference's swap-and-pop, ComputeE21 of cms_init_core.h on the
//                       eight ray pairs, E stored as nine floats.  32 lanes per workgroup; the 8 x 9 system and its right vectors (72 + 81 floats
//                       per lane) live in LDS, 153 dwords apart -- odd, so the lanes of a workgroup fall on different banks -- and the nine column
//                       norms (doubles) in a block of their own, 18 dwords apart
//   k_init_check        one wavefront per (job, iteration): CheckEssiential, lanes stride over the matches, the 64-bit ballot is the mask word; the
//                       terms of a word go through LDS and the first lane adds them in match order, first-view term before second-view term
//   k_init_select       one workgroup per job: the first iteration of maximal score under >, DecomposeE, then the four CheckRT passes with one
//                       thread per match (vP3D, vbGood, nGood, and the cosine at sorted index min(50, nGood-1) found by a bitwise descent over the
//                       ordered keys of cms_init_core.h).  ReconstructE's decision is taken on the host
//
// The device is held to the host build of cms_init_core.h bit for bit (tests/test_gpu_init.py): every operation of the core is an IEEE-rounded
// + - * / sqrt on both sides (-ffp-contract=off), and the kernels add no arithmetic of their own.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cms_init_core.h"
#include "cms_types.h"

#define CMS_INIT_HYP_LANES 32
#define CMS_INIT_LANE_FLOATS 153      // 72 (At) + 81 (Vt): odd
#define CMS_INIT_SELECT_THREADS 256

struct CmsInitJobDev {
  int N, H, n1;
  int m0;               // first match in the call's arrays
  int hyp0;             // first hypothesis in the call's arrays
  int key0;             // first key point of frame 1 in the call's candidate arrays
  int words;            // mask words per hypothesis: (N + 63) / 64
  long long word0;      // first word of the job's hypothesis masks
  float sigma, th2;
};
struct CmsInitOutDev {
  int best, n_inliers, nGood[4];
  float score, cosines[4], R1[9], R2[9], t[3];
};
struct CmsInitRunArgs {
  int F, njobs, nhyp;
  float cos_fov;
  const CmsInitJobDev* jobs;
  const int* hyp_job;                  // job of every hypothesis
  const int* draws;                    // 8 per hypothesis
  const int* m_first;                  // key point of frame 1 of every match
  const float* m_ray1; const float* m_kp1; const float* m_ray2; const float* m_kp2;
  float* hyp_E;                        // 9 per hypothesis
  float* hyp_score;
  unsigned long long* hyp_mask;
  unsigned* cos_keys;                  // one per match: the pass's ordered cosine keys
  float* cand_p3d;                     // per job 4 x 3*n1 floats, from 12*key0
  uint8_t* cand_good;                  // per job 4 x n1 bytes, from 4*key0
  CmsInitOutDev* out;
};

// cms_init_two_view_frames: mvKeys2 / mvKeyRays2 of every match from the context's resident rows (Initializer.cpp:58-59)
struct CmsInitGatherArgs {
  int nmatch, kp_cap;
  const int* m_job;                    // job of every match
  const int* job_row;                  // frame row of every job
  const int* m_second;                 // key point of frame 2, checked against the row's count (<= kp_cap) on the host
  const CmsKeyPoint* kps; const float* rays;
  float* m_ray2; float* m_kp2;
};
extern "C" __global__ void __launch_bounds__(256) k_init_gather(CmsInitGatherArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.nmatch) return;
  int k = a.m_second[i];
  k = k < 0 ? 0 : (k >= a.kp_cap ? a.kp_cap - 1 : k);
  const size_t r = (size_t)a.job_row[a.m_job[i]] * a.kp_cap + (size_t)k;
  const CmsKeyPoint kp = a.kps[r];
  a.m_kp2[2 * (size_t)i] = kp.x; a.m_kp2[2 * (size_t)i + 1] = kp.y;
  for (int q = 0; q < 3; ++q) a.m_ray2[3 * (size_t)i + q] = a.rays[3 * r + q];
}

extern "C" __global__ void __launch_bounds__(CMS_INIT_HYP_LANES) k_init_hypotheses(CmsInitRunArgs a) {
  __shared__ float s_mat[CMS_INIT_HYP_LANES * CMS_INIT_LANE_FLOATS];
  __shared__ double s_w[CMS_INIT_HYP_LANES * 9];
  const int g = blockIdx.x * CMS_INIT_HYP_LANES + threadIdx.x;
  if (g >= a.nhyp) return;
  const CmsInitJobDev& J = a.jobs[a.hyp_job[g]];
  float* At = s_mat + (size_t)threadIdx.x * CMS_INIT_LANE_FLOATS;
  float* Vt = At + 72;
  double* W = s_w + (size_t)threadIdx.x * 9;
  int idx[8];
  cms_init_resolve_draws(J.N, a.draws + 8 * (size_t)g, idx);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i = idx[j] < 0 ? 0 : (idx[j] >= J.N ? J.N - 1 : idx[j]);      // the host has checked the draws; never index beyond the job
    const size_t c = (size_t)J.m0 + (size_t)i;
    float r1[3], r2[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) { r1[q] = a.m_ray1[3 * c + q]; r2[q] = a.m_ray2[3 * c + q]; }
    cms_init_fill_row(j, r1, r2, At);
  }
  float E[9];
  cms_init_e21_from_rows(At, Vt, W, E, nullptr);
  float* o = a.hyp_E + 9 * (size_t)g;
#pragma unroll
  for (int k = 0; k < 9; ++k) o[k] = E[k];
}

extern "C" __global__ void __launch_bounds__(64) k_init_check(CmsInitRunArgs a) {
  __shared__ float s_term[128];
  const int g = blockIdx.x, lane = threadIdx.x;
  const CmsInitJobDev& J = a.jobs[a.hyp_job[g]];
  float E[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) E[k] = a.hyp_E[9 * (size_t)g + k];
  unsigned long long* mask = a.hyp_mask + J.word0 + (long long)(g - J.hyp0) * J.words;
  float score = 0;      // the first lane's
  for (int w = 0; w < J.words; ++w) {
    const int i = w * 64 + lane;
    bool in = false, add1 = false, add2 = false;
    float t1 = 0.0f, t2 = 0.0f;
    if (i < J.N) {
      const size_t c = (size_t)J.m0 + (size_t)i;
      float r1[3], r2[3], k1[2], k2[2];
#pragma unroll
      for (int q = 0; q < 3; ++q) { r1[q] = a.m_ray1[3 * c + q]; r2[q] = a.m_ray2[3 * c + q]; }
      k1[0] = a.m_kp1[2 * c]; k1[1] = a.m_kp1[2 * c + 1]; k2[0] = a.m_kp2[2 * c]; k2[1] = a.m_kp2[2 * c + 1];
      in = cms_init_check_terms(a.F, E, J.sigma, r1, r2, k1, k2, &t1, &add1, &t2, &add2);
    }
    const unsigned long long m = __ballot(in), m1 = __ballot(add1), m2 = __ballot(add2);
    s_term[2 * lane] = t1; s_term[2 * lane + 1] = t2;
    __syncthreads();
    if (lane == 0) {
      mask[w] = m;
      const int n = J.N - w * 64 < 64 ? J.N - w * 64 : 64;
      for (int q = 0; q < n; ++q) {
        if ((m1 >> q) & 1ull) score += s_term[2 * q];
        if ((m2 >> q) & 1ull) score += s_term[2 * q + 1];
      }
    }
    __syncthreads();
  }
  if (lane == 0) a.hyp_score[g] = score;
}

extern "C" __global__ void __launch_bounds__(CMS_INIT_SELECT_THREADS) k_init_select(CmsInitRunArgs a) {
  __shared__ float s_R1[9], s_R2[9], s_t[3], s_score;
  __shared__ int s_best, s_nGood, s_count, s_inliers, s_outGood[4];
  __shared__ float s_outCos[4];
  const int j = blockIdx.x, tid = threadIdx.x;
  const CmsInitJobDev& J = a.jobs[j];
  float* cand_p3d = a.cand_p3d + 12 * (size_t)J.key0;
  uint8_t* cand_good = a.cand_good + 4 * (size_t)J.key0;
  unsigned* keys = a.cos_keys + J.m0;
  if (tid == 0) {
    // FindEssential's `currentScore>score`, from 0.0: the first iteration of maximal score; NaN never wins
    float score = 0.0f;
    int best = -1;
    for (int h = 0; h < J.H; ++h) {
      const float cs = a.hyp_score[J.hyp0 + h];
      if (cs > score) { score = cs; best = h; }
    }
    s_best = best; s_score = score; s_inliers = 0;
    if (best >= 0) {
      float E[9], R1[9], R2[9], t[3];
#pragma unroll
      for (int k = 0; k < 9; ++k) E[k] = a.hyp_E[9 * (size_t)(J.hyp0 + best) + k];
      cms_init_decompose_e(E, R1, R2, t);
#pragma unroll
      for (int k = 0; k < 9; ++k) { s_R1[k] = R1[k]; s_R2[k] = R2[k]; }
#pragma unroll
      for (int k = 0; k < 3; ++k) s_t[k] = t[k];
    } else {
      for (int k = 0; k < 9; ++k) { s_R1[k] = 0.0f; s_R2[k] = 0.0f; }
      for (int k = 0; k < 3; ++k) s_t[k] = 0.0f;
    }
    for (int h = 0; h < 4; ++h) { s_outGood[h] = 0; s_outCos[h] = 0.0f; }
  }
  // vbGood = vector<bool>(n1, false), vP3D.resize(n1): an entry never written is (0,0,0)
  for (int i = tid; i < 12 * J.n1; i += CMS_INIT_SELECT_THREADS) cand_p3d[i] = 0.0f;
  for (int i = tid; i < 4 * J.n1; i += CMS_INIT_SELECT_THREADS) cand_good[i] = 0;
  __syncthreads();
  const int best = s_best;
  if (best >= 0) {
    const unsigned long long* bm = a.hyp_mask + J.word0 + (long long)best * J.words;
    {
      int cnt = 0;
      for (int w = tid; w < J.words; w += CMS_INIT_SELECT_THREADS) cnt += __popcll(bm[w]);
      if (cnt) atomicAdd(&s_inliers, cnt);
    }
    for (int h = 0; h < 4; ++h) {
      float R[9], t[3], O2[3];
#pragma unroll
      for (int k = 0; k < 9; ++k) R[k] = (h & 1) ? s_R2[k] : s_R1[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) t[k] = h >= 2 ? -s_t[k] : s_t[k];
      cms_init_o2(R, t, O2);
      if (tid == 0) { s_nGood = 0; s_count = 0; }
      __syncthreads();
      float* vP3D = cand_p3d + (size_t)h * 3 * (size_t)J.n1;
      uint8_t* vbGood = cand_good + (size_t)h * (size_t)J.n1;
      int mine = 0;
      for (int i = tid; i < J.N; i += CMS_INIT_SELECT_THREADS) {
        unsigned key = 0xffffffffu;      // not counted: behind every counted cosine
        if ((bm[i >> 6] >> (i & 63)) & 1ull) {
          const size_t c = (size_t)J.m0 + (size_t)i;
          float r1[3], r2[3], k1[2], k2[2], p[3], cosp;
          int good;
#pragma unroll
          for (int q = 0; q < 3; ++q) { r1[q] = a.m_ray1[3 * c + q]; r2[q] = a.m_ray2[3 * c + q]; }
          k1[0] = a.m_kp1[2 * c]; k1[1] = a.m_kp1[2 * c + 1]; k2[0] = a.m_kp2[2 * c]; k2[1] = a.m_kp2[2 * c + 1];
          if (cms_init_check_rt_match(a.F, a.cos_fov, J.th2, R, t, O2, r1, r2, k1, k2, p, &cosp, &good)) {
            int f = a.m_first[c];
            f = f < 0 ? 0 : (f >= J.n1 ? J.n1 - 1 : f);      // the host built it from the job's own indices; never write beyond the job
            vP3D[3 * (size_t)f] = p[0]; vP3D[3 * (size_t)f + 1] = p[1]; vP3D[3 * (size_t)f + 2] = p[2];
            if (good) vbGood[f] = 1;
            key = cms_init_cos_key(cosp);
            ++mine;
          }
        }
        keys[i] = key;
      }
      if (mine) atomicAdd(&s_nGood, mine);
      __syncthreads();
      const int nGood = s_nGood;
      float cos_sel = 0.0f;
      if (nGood > 0) {
        // the key at sorted index k: the largest v with #(key < v) <= k, one bit after the other (every thread reads its own keys back)
        const int k = nGood - 1 < 50 ? nGood - 1 : 50;
        unsigned prefix = 0;
        for (int bit = 31; bit >= 0; --bit) {
          const unsigned cand = prefix | (1u << bit);
          int below = 0;
          for (int i = tid; i < J.N; i += CMS_INIT_SELECT_THREADS) below += keys[i] < cand ? 1 : 0;
          if (below) atomicAdd(&s_count, below);
          __syncthreads();
          if (s_count <= k) prefix = cand;
          __syncthreads();
          if (tid == 0) s_count = 0;
          __syncthreads();
        }
        cos_sel = cms_init_cos_from_key(prefix);
      }
      if (tid == 0) { s_outGood[h] = nGood; s_outCos[h] = cos_sel; }
      __syncthreads();
    }
  }
  __syncthreads();
  if (tid == 0) {
    CmsInitOutDev* o = a.out + j;
    o->best = best; o->score = s_score; o->n_inliers = best >= 0 ? s_inliers : 0;
    for (int h = 0; h < 4; ++h) { o->nGood[h] = s_outGood[h]; o->cosines[h] = s_outCos[h]; }
    for (int k = 0; k < 9; ++k) { o->R1[k] = s_R1[k]; o->R2[k] = s_R2[k]; }
    for (int k = 0; k < 3; ++k) o->t[k] = s_t[k];
  }
}
