// cms_sim3_proj_kernels.hip -- ORBMatcher::SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th) (src/ORBMatcher.cpp:796-903) and the search half
// of ORBMatcher::Fuse(KeyFrame*, Scw, vpPoints, th, vpReplacePoint) (:1246-1363) on resident key frames, behind cms_kfstore_search_by_projection_sim3
// and cms_kfstore_fuse_search_sim3 (cms_api_sim3_proj.hip).  An ENTRY is one map point of the set one job searches: job j has as many entries as its
// set has points, in the set's order.
//   k_sim3p_project   one thread per entry: the point through the job's decomposed Scw (csrc/cms_sim3_proj_core.h, the host build's source too):
//                     the window (qx, qy, qr; qr < 0 = dropped), the predicted level and the drop code.  The set is shared: the entry reads the
//                     point's record through `rec`, as CmsFuseArgs::src does
//   (window query)    cms_area_kernels.hip against the store's grids, no level filter: KeyFrame::GetFeaturesInArea(u, v, radius), its order
//   k_sim3p_scan      Fuse's scan (:1323-1342): cms_window_scan (cms_tri_kernels.hip) without the reprojection gate, accepted when dist <= TH_LOW (50)
//   k_sim3p_greedy    SearchByProjection's scan (:870-898), one workgroup per job.  The reference's loop is sequential: `if(vpMatched[idx]) continue;`
//                     skips key points taken on entry and key points an earlier iMP of the same call took.  Resolved in rounds the way
//                     k_search_local does: an entry is decided in the round in which it is the lowest undecided claimant of every free candidate
//                     it has -- then every earlier entry that could take one of them has spoken.  Entries decided in one round have disjoint free
//                     candidates, and the lowest undecided entry always qualifies, so the loop ends.  Pair distances are computed once; a pair
//                     whose octave fails the level gate is no candidate at all (the reference tests vpMatched first and the level second, but a
//                     gated key point is never taken by this entry, so the order does not show).  The claim tables (taken flags and lowest
//                     claimant per key point of the job's key frame) live in LDS: 4096 key points at most, which the host checks
// k_search_local itself is left as it is: its map-point descriptors and claim rows are indexed per frame of a context's batch, these entries read
// a shared set through `rec` and claim key points of a store slot.  The split was not chosen by measurement.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cms_sim3_proj_core.h"
#include "cms_sim3_proj_job_check.h"      // CMS_SIM3P_KPMAX

struct CmsSim3pJobDev {
  int slot, n, set0, taken0;      // set0: first record of the job's set; taken0: first byte of the job's taken flags
  CmsSim3pPose ps;                // decomposed once per job, on the host, by cms_sim3p_decompose
};
struct CmsSim3pArgs {
  int n_ent, njobs;
  const CmsSim3pJobDev* job; const int* ent_off;      // ent_off[njobs + 1]: first entry of every job
  const uint8_t* skip;                                // per entry
  const float* pos; const float* normal; const float* min_dist; const float* max_dist;      // per record of the sets
  float th, log_scale; int nlevels, F, bounds_scaled; float sf[16];
  float* qx; float* qy; float* qr; int* qmin; int* qmax; int* level;
  int* qslot;      // the store slot whose grid the entry searches
  int* rec;        // the entry's map-point record
  int* why;        // the drop code (CMS_SIM3P_*; -1: skipped)
};

extern "C" __global__ void __launch_bounds__(256) k_sim3p_project(CmsSim3pArgs a) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= a.n_ent) return;
  const int j = cms_job_of(a.ent_off, a.njobs, e);
  const CmsSim3pJobDev* jb = a.job + j;
  const int r = jb->set0 + (e - a.ent_off[j]);
  float u = -1.0f, v = -1.0f, qr = -1.0f, dist; int lvl = -1, why = -1;
  if (!a.skip[e]) {
    const float P[3] = {a.pos[3 * (size_t)r], a.pos[3 * (size_t)r + 1], a.pos[3 * (size_t)r + 2]};
    const float N[3] = {a.normal[3 * (size_t)r], a.normal[3 * (size_t)r + 1], a.normal[3 * (size_t)r + 2]};
    why = cms_sim3p_project(a.F, &jb->ps, P, N, a.bounds_scaled, a.min_dist[r], a.max_dist[r], a.th, a.log_scale, a.nlevels, a.sf, &u, &v, &dist, &lvl, &qr);
  }
  if (jb->n == 0) qr = -1.0f;                      // a key frame without key points: no window
  a.qx[e] = u; a.qy[e] = v; a.qr[e] = qr; a.qmin[e] = -1; a.qmax[e] = -1; a.level[e] = lvl;
  a.qslot[e] = jb->slot; a.rec[e] = r; a.why[e] = why;
}

struct CmsSim3pGreedyArgs {
  const CmsSim3pJobDev* job; const int* ent_off;
  const int* level; const int* rec; const uint4* mp_desc;
  const int* cand_off; const int* cand_idx; int cap;
  const int* total;               // *total > cap: the lists were cut short -- do nothing, the host repeats the call
  const CmsKeyPoint* kp; const uint4* t_desc; int maxf;
  const uint8_t* taken;           // per job n bytes from job.taken0: vpMatched[idx] != NULL on entry (read only)
  uint16_t* pair_dist;            // one entry per candidate pair (scratch); 0xFFFF: the octave fails the level gate
  int* match;                     // per entry: key point taken or -1 (device memory: the rounds' state)
  int* out;                       // where the decided entries go at the end (match itself, or the caller's pinned array)
  int* n_matches;                 // per job
  int* rounds;                    // per job: rounds the greedy needed
};
#define CMS_SIM3P_GATED 0xFFFFu
extern "C" __global__ void __launch_bounds__(1024) k_sim3p_greedy(CmsSim3pGreedyArgs a) {
  __shared__ int min_open[CMS_SIM3P_KPMAX];           // lowest undecided entry that still wants key point k
  __shared__ uint8_t s_taken[CMS_SIM3P_KPMAX];        // vpMatched[k] != NULL, on entry and as the call goes on
  __shared__ int s_count;
  const int j = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  if (*a.total > a.cap) return;
  const CmsSim3pJobDev jb = a.job[j];
  const int e0 = a.ent_off[j], e1 = a.ent_off[j + 1];
  const int row0 = jb.slot * a.maxf;
  const int nk = min(a.maxf, CMS_SIM3P_KPMAX);
  for (int k = tid; k < nk; k += nt) s_taken[k] = k < jb.n ? (uint8_t)(a.taken[(size_t)jb.taken0 + k] != 0) : (uint8_t)0;
  if (tid == 0) s_count = 0;
  // ---- distances of all pairs of this job, 4 lanes per entry
  {
    const int sub = tid & 3;
    for (int e = e0 + (tid >> 2); e < e1; e += nt >> 2) {
      const int c0 = a.cand_off[e], c1 = a.cand_off[e + 1];
      if (c0 == c1) continue;
      const int lvl = a.level[e];
      const size_t mi = (size_t)a.rec[e];
      const uint4 q0 = a.mp_desc[2 * mi], q1 = a.mp_desc[2 * mi + 1];
      for (int c = c0 + sub; c < c1; c += 4) {
        const size_t row = (size_t)a.cand_idx[c];
        const int oct = a.kp[row].octave;
        a.pair_dist[c] = (oct < lvl - 1 || oct > lvl) ? (uint16_t)CMS_SIM3P_GATED : (uint16_t)tri_hamming256(q0, q1, a.t_desc[2 * row], a.t_desc[2 * row + 1]);
      }
    }
  }
  for (int e = e0 + tid; e < e1; e += nt) a.match[e] = a.cand_off[e] == a.cand_off[e + 1] ? -1 : -2;   // -2 = undecided
  __syncthreads();
  int round = 0, mine = 0;
  for (;;) {
    for (int k = tid; k < nk; k += nt) min_open[k] = 0x7FFFFFFF;
    __syncthreads();
    for (int e = e0 + tid; e < e1; e += nt) {
      if (a.match[e] != -2) continue;
      for (int c = a.cand_off[e]; c < a.cand_off[e + 1]; ++c) {
        if (a.pair_dist[c] == CMS_SIM3P_GATED) continue;
        const int k = a.cand_idx[c] - row0;
        if (!s_taken[k]) atomicMin(&min_open[k], e);
      }
    }
    __syncthreads();
    // which of my entries are the lowest claimant of every free candidate they have?  (decided before anybody writes a claim; a ready entry is
    // marked -3 in its own match entry, which only its owner thread reads)
    int open = 0;
    for (int e = e0 + tid; e < e1; e += nt) {
      if (a.match[e] != -2) continue;
      bool ok = true;
      for (int c = a.cand_off[e]; c < a.cand_off[e + 1] && ok; ++c) {
        if (a.pair_dist[c] == CMS_SIM3P_GATED) continue;
        const int k = a.cand_idx[c] - row0;
        ok = s_taken[k] || min_open[k] == e;
      }
      if (ok) a.match[e] = -3; else ++open;
    }
    __syncthreads();
    for (int e = e0 + tid; e < e1; e += nt) {
      if (a.match[e] != -3) continue;
      int bestDist = 256, bestIdx = -1;               // :870-892 over the candidates in GetFeaturesInArea's order
      for (int c = a.cand_off[e]; c < a.cand_off[e + 1]; ++c) {
        const int dist = a.pair_dist[c];
        if (dist == CMS_SIM3P_GATED) continue;
        const int k = a.cand_idx[c] - row0;
        if (s_taken[k]) continue;
        if (dist < bestDist) { bestDist = dist; bestIdx = k; }
      }
      const int m = bestDist <= 50 ? bestIdx : -1;    // TH_LOW
      if (m >= 0) { s_taken[m] = 1; ++mine; }
      a.match[e] = m;
    }
    ++round;
    if (__syncthreads_count(open > 0) == 0 || round > e1 - e0) break;      // (every round decides at least the lowest undecided entry)
  }
  if (a.out != a.match)
    for (int e = e0 + tid; e < e1; e += nt) a.out[e] = a.match[e];
  if (mine) atomicAdd(&s_count, mine);
  __syncthreads();
  if (tid == 0) { a.n_matches[j] = s_count; a.rounds[j] = round; }
}
