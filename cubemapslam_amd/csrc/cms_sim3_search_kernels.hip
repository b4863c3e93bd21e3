// cms_sim3_search_kernels.hip -- ORBMatcher::SearchBySim3 (src/ORBMatcher.cpp:1365-1586) on resident key frames, behind cms_kfstore_search_by_sim3
// (cms_api_sim3_search.hip).  An ENTRY is one key point of one side of one job: job j has n1 + n2 entries, key frame 1's first.
//   k_sim3s_project   one thread per entry: the entry's map point through its own key frame's pose and the similarity into the OTHER key frame
//                     (csrc/cms_sim3_search_core.h, the host build's source too), track_predict_scale, and the window
//                     (qx, qy, qr; qr < 0 = dropped) with the slot whose grid it searches
//   (window query)    cms_area_kernels.hip against the store's grids, no level filter: KeyFrame::GetFeaturesInArea(u, v, radius), its order
//   k_sim3s_scan      cms_window_scan (cms_tri_kernels.hip) without the reprojection gate, accepted when dist <= TH_HIGH (100), the index alone
//   k_sim3s_agree     one thread per key point of key frame 1: idx2 = vnMatch1[i1] where vnMatch2[vnMatch1[i1]] == i1 (:1567-1583); the jobs' counts
//                     by wave ballot, one integer atomic add per job present in a wavefront
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

extern "C" __global__ void __launch_bounds__(256) k_sim3s_project(CmsSim3sArgs a) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n_ent) return;
  const int j = cms_job_of(a.ent_off, a.njobs, e);
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
      lvl = track_predict_scale(maxd, dist3D, a.log_scale, a.nlevels); qr = __fmul_rn(a.th, a.sf[lvl]);
    }
  }
  a.qx[e] = u; a.qy[e] = v; a.qr[e] = qr; a.qmin[e] = -1; a.qmax[e] = -1; a.level[e] = lvl;
  a.qslot[e] = second ? jb->slot1 : jb->slot2; a.rec[e] = r;
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
    const int j = cms_job_of(a.n1_off, a.njobs, t);
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
