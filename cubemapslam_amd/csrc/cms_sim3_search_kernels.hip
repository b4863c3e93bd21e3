// cms_sim3_search_kernels.hip -- ORBMatcher::SearchBySim3 (src/ORBMatcher.cpp:1365-1586) on resident key frames, behind cms_kfstore_search_by_sim3
// (cms_api_sim3_search.hip).  An ENTRY is one key point of one side of one job: job j has n1 + n2 entries, key frame 1's first.
//   k_sim3s_project   one thread per entry: the entry's map point through its own key frame's pose and the similarity into the OTHER key frame
//                     (csrc/cms_sim3_search_core.h, the host build's source too), PredictScale as k_fuse_project computes it, and the window
//                     (qx, qy, qr; qr < 0 = dropped) with the slot whose grid it searches
//   (window query)    cms_area_kernels.hip against the store's grids, no level filter: KeyFrame::GetFeaturesInArea(u, v, radius), its order
//   k_sim3s_scan      eight lanes per entry over its candidates: octave in {level - 1, level}, Hamming distance, key = dist << 20 | position, so
//                     the first minimum in list order wins; accepted when dist <= TH_HIGH (100).  A sibling of k_fuse_scan without its
//                     reprojection gate and with the other threshold
//   k_sim3s_agree     one thread per key point of key frame 1: idx2 = vnMatch1[i1] where vnMatch2[vnMatch1[i1]] == i1 (:1567-1583); the jobs' counts
//                     by wave ballot, one integer atomic add per job present in a wavefront
// The split follows the shapes the project already has (the window launcher, the eight-lane scan); it was not chosen by measurement.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cms_sim3_search_core.h"

struct CmsSim3sJobDev {
  int slot1, slot2, n1, n2, off1, off2;
  float R1w[9], t1w[3], R2w[9], t2w[3];      // the slots' poses
  CmsSim3sMotion m;                          // composed once per job, on the host, by cms_sim3s_compose
};
struct CmsSim3sArgs {
  int n_ent, njobs;
  const CmsSim3sJobDev* job; const int* ent_off;      // ent_off[njobs + 1]: first entry of every job
  const uint8_t* skip; const float* pos; const float* min_dist; const float* max_dist;      // the call's map-point records
  float th, log_scale; int nlevels, F, bounds_scaled, z_as_written; float sf[16];
  float* qx; float* qy; float* qr; int* qmin; int* qmax; int* level;
  int* qslot;      // the store slot whose grid the entry searches (the OTHER key frame's)
  int* rec;        // the entry's map-point record
};

// the job of entry / key point i: the last one whose first is <= i (empty jobs are skipped by the search), as k_fuse_expand_jobs does
__device__ __forceinline__ int sim3s_job_of(const int* __restrict__ first, int njobs, int i) {
  int lo = 0, hi = njobs;
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (first[mid] <= i) lo = mid; else hi = mid; }
  return lo;
}

extern "C" __global__ void __launch_bounds__(256) k_sim3s_project(CmsSim3sArgs a) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n_ent) return;
  const int j = sim3s_job_of(a.ent_off, a.njobs, e);
  const CmsSim3sJobDev* jb = a.job + j;
  const int local = e - a.ent_off[j];
  const bool second = local >= jb->n1;                         // an entry of key frame 2: direction 2 -> 1
  const int r = second ? jb->off2 + (local - jb->n1) : jb->off1 + local;
  float u = -1.0f, v = -1.0f, qr = -1.0f; int lvl = -1;
  if (!a.skip[r]) {
    const float P[3] = {a.pos[3 * (size_t)r], a.pos[3 * (size_t)r + 1], a.pos[3 * (size_t)r + 2]};
    float dist3D, maxd;
    const int why = second ? cms_sim3s_project(a.F, jb->R2w, jb->t2w, jb->m.sR12, jb->m.t12, P, a.z_as_written, a.bounds_scaled, a.min_dist[r], a.max_dist[r], &u, &v, &dist3D, &maxd)
                           : cms_sim3s_project(a.F, jb->R1w, jb->t1w, jb->m.sR21, jb->m.t21, P, 0, a.bounds_scaled, a.min_dist[r], a.max_dist[r], &u, &v, &dist3D, &maxd);
    if (why == CMS_SIM3S_KEEP) {
      const float ratio = maxd / dist3D;                       // MapPoint::PredictScale, as k_fuse_project
      int ns = (int)ceilf((float)log((double)ratio) / a.log_scale);
      if (ns < 0) ns = 0; else if (ns >= a.nlevels) ns = a.nlevels - 1;
      lvl = ns; qr = __fmul_rn(a.th, a.sf[ns]);
    }
  }
  a.qx[e] = u; a.qy[e] = v; a.qr[e] = qr; a.qmin[e] = -1; a.qmax[e] = -1; a.level[e] = lvl;
  a.qslot[e] = second ? jb->slot1 : jb->slot2; a.rec[e] = r;
}

struct CmsSim3sScanArgs {
  int n_ent; const int* level; const int* rec; const int* qslot; const uint4* mp_desc;
  const int* cand_off; const int* cand_idx;      // the window query's lists: rows of the store (slot x maxf + key point)
  int cap;                                       // entries of cand_idx that exist: the scan is enqueued before the host has seen the total
  const CmsKeyPoint* kp; const uint4* t_desc; int maxf;
  int* match;                                    // per entry: key point of the searched key frame, or -1
};
extern "C" __global__ void __launch_bounds__(256) k_sim3s_scan(CmsSim3sScanArgs a) {
  const int gl = threadIdx.x & 7;
  const int e = (blockIdx.x * blockDim.x + threadIdx.x) >> 3;
  const bool live = e < a.n_ent;
  const int ee = live ? e : 0;
  const int c0 = live ? a.cand_off[ee] : 0, c1 = live ? min(a.cand_off[ee + 1], a.cap) : 0;
  const int lvl = a.level[ee];
  uint32_t key = 0xFFFFFFFFu;                        // dist << 20 | position: the first minimum in list order wins
  if (c1 > c0) {
    const size_t mi = (size_t)a.rec[ee];
    const uint4 d0 = a.mp_desc[2 * mi], d1 = a.mp_desc[2 * mi + 1];
    for (int c = c0 + gl; c < c1; c += 8) {
      const size_t row = (size_t)a.cand_idx[c];
      const int oct = a.kp[row].octave;
      if (oct < lvl - 1 || oct > lvl) continue;
      const uint32_t d = (uint32_t)tri_hamming256(d0, d1, a.t_desc[2 * row], a.t_desc[2 * row + 1]);
      key = min(key, (d << 20) | (uint32_t)(c - c0));
    }
  }
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) key = min(key, (uint32_t)__shfl_xor((int)key, o, 8));
  if (live && gl == 0) {
    // no surviving candidate: bestDist stays INT_MAX and INT_MAX <= TH_HIGH is false
    const bool hit = key != 0xFFFFFFFFu && (key >> 20) <= 100u;
    a.match[e] = hit ? a.cand_idx[c0 + (int)(key & 0xFFFFFu)] - a.qslot[e] * a.maxf : -1;
  }
}

struct CmsSim3sAgreeArgs {
  int n1_total, njobs;
  const CmsSim3sJobDev* job; const int* ent_off; const int* n1_off;      // n1_off[njobs + 1]: first idx2 entry of every job
  const int* match; int* idx2; int* n_found;                             // n_found zeroed before the launch
};
extern "C" __global__ void __launch_bounds__(256) k_sim3s_agree(CmsSim3sAgreeArgs a) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int mine = -1;                                     // the job this lane adds one match to
  if (t < a.n1_total) {
    const int j = sim3s_job_of(a.n1_off, a.njobs, t);
    const int i1 = t - a.n1_off[j], e0 = a.ent_off[j], n1 = a.job[j].n1, n2 = a.job[j].n2;
    const int m = a.match[e0 + i1];
    const bool ok = m >= 0 && m < n2 && a.match[e0 + n1 + m] == i1;
    a.idx2[t] = ok ? m : -1;
    if (ok) mine = j;
  }
  unsigned long long todo = __ballot(mine >= 0);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int jl = __shfl(mine, leader);
    const unsigned long long same = __ballot(mine == jl);
    if (lane == leader) atomicAdd(&a.n_found[jl], (int)__popcll(same));
    todo &= ~same;
  }
}
