// cms_ba_window_kernels.hip -- the local BA window from the resident stores (csrc/cms_ba_window_core.h states the rules; host side in
// cms_api_ba_window.hip).  gfx950, wave64.  Included by cms_lib.hip behind cms_covis_kernels.hip (CmsCovisDev, covis_find, k_covis_local_points),
// cms_tri_kernels.hip (CmsTriKF) and cms_mappoint_kernels.hip (CmsMpTable).
//
// All jobs of a call go through four launches:
//   k_covis_local_points   one workgroup per job: the local points into the scratch list pid (never cut: its stride is the local rows' features)
//   k_baw_count            a grid over (point chunk, job), one thread per point: the edges the point keeps, and whether its table row has a position
//   k_baw_frames           one workgroup per job, the members' first-point keys and the candidates in LDS (8 bytes per member): the fixed list by rank
//                          of (first point, member), the window index of every window member, kf_member / fixed / poses, the exclusive prefix sum of
//                          the edge counts, the job's counts
//   k_baw_fill             the grid of k_baw_count again: point_id, points and the edges.  Edge e of point p is written at (prefix of p) + (its rank
//                          among p's kept observations by member position), so the order is a function of (p, member) alone
// Where a segment of the index lies and the order inside it depend on how atomics landed at the build; nothing here does: counts are sums, the
// first-point key is an integer minimum, and an observation's place comes from its member position.  Every output is a plain vector store of a value
// that is defined bit for bit; nothing is written at or beyond a cap.
// Resources (hipcc's kernel-resource-usage): k_baw_count 22, k_baw_frames 51, k_baw_fill 40 VGPRs, eight waves per SIMD each, no scratch (the
// quaternion is written through selects, not a runtime index); k_baw_frames takes 8 bytes of dynamic LDS per member, 128 KB at 16 384 members.
#include "cms_ba_window_core.h"

struct CmsBawArgs {
  CmsCovisDev d;
  const CmsTriKF* kf; const CmsKeyPoint* st_kp; const float* st_rays; int st_maxf;      // the store's slots
  CmsMpTable t;
  int njobs, F; float cos_fov; float inv_sigma2[16];
  const int* loc_off; const int* loc_members; const int* first_member;                  // the jobs: members loc_members[loc_off[j], loc_off[j + 1])
  int cap_kf, cap_points, cap_edges;
  // scratch, per job: the local points (stride pid_stride), their number, edges kept per point and their prefix (stride pid_stride), the window
  // index per member (stride M)
  int pid_stride; const int* pid; const int* npts; int* ecount; int* eoff; int* widx;
  int* missing;                  // per job: 1 + the list position of a local point without a position, 0: none
  CmsBaWindowCounts* counts;
  int* kf_member; int* point_id; double* poses; uint8_t* fixed; double* points;
  int* e_pose; int* e_point; double* e_obs; double* e_invsig2; int8_t* e_face; int* e_feat;
};

// the face of observation e (an entry of the index's segments), -1: no edge
__device__ __forceinline__ int baw_obs_face(const CmsBawArgs& a, int e, size_t* row) {
  const size_t r = (size_t)a.d.slot[a.d.obs[e].x] * a.st_maxf + (size_t)a.d.obs_feat[e];
  *row = r;
  return cms_baw_edge_face(a.F, a.cos_fov, a.st_kp[r].x, a.st_kp[r].y, a.st_rays[3 * r + 2]);
}

extern "C" __global__ void __launch_bounds__(256) k_baw_count(const CmsBawArgs a) {
  const int j = blockIdx.y, p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.npts[j]) return;
  const int id = a.pid[(size_t)j * a.pid_stride + p];
  if (id >= a.t.max_points || a.t.ref[id] < 0) a.missing[j] = 1 + p;      // (any of them: the host names the job)
  const int u = covis_find(a.d, id);      // (>= 0: the id comes from a member's row)
  int n = 0;
  if (u < 0) { a.ecount[(size_t)j * a.pid_stride + p] = 0; return; }
  const int e0 = a.d.off[u], e1 = e0 + a.d.cnt[u];
  size_t row;
  for (int e = e0; e < e1; ++e) n += baw_obs_face(a, e, &row) >= 0 ? 1 : 0;
  a.ecount[(size_t)j * a.pid_stride + p] = n;
}

// LDS: s_first[M], then s_cand[M].  s_first[m]: -1 - k for the local member at list position k, the least list position of a local point the member
// observes otherwise, 0x7FFFFFFF: none
extern "C" __global__ void __launch_bounds__(1024) k_baw_frames(const CmsBawArgs a) {
  extern __shared__ int s_mem[];
  __shared__ int s_ncand, s_wave[16];
  int* s_first = s_mem;
  int* s_cand = s_mem + a.d.M;
  const int j = blockIdx.x, M = a.d.M, q0 = a.loc_off[j], nl = a.loc_off[j + 1] - q0, P = a.npts[j], fm = a.first_member[j];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  const int* pid = a.pid + (size_t)j * a.pid_stride;
  int* widx = a.widx + (size_t)j * M;
  for (int m = threadIdx.x; m < M; m += blockDim.x) s_first[m] = 0x7FFFFFFF;
  if (threadIdx.x == 0) s_ncand = 0;
  __syncthreads();
  for (int k = threadIdx.x; k < nl; k += blockDim.x) s_first[a.loc_members[q0 + k]] = -1 - k;
  __syncthreads();
  for (int p = threadIdx.x; p < P; p += blockDim.x) {
    const int u = covis_find(a.d, pid[p]);
    if (u < 0) continue;
    const int e0 = a.d.off[u], e1 = e0 + a.d.cnt[u];
    for (int e = e0; e < e1; ++e) { const int m = a.d.obs[e].x; if (s_first[m] >= 0) atomicMin(&s_first[m], p); }      // (a local member's entry stays negative)
  }
  __syncthreads();
  for (int m = threadIdx.x; m < M; m += blockDim.x) {
    const int v = s_first[m];
    if (v >= 0 && v != 0x7FFFFFFF) s_cand[atomicAdd(&s_ncand, 1)] = m;      // (in any order: the rank below does not depend on it)
  }
  __syncthreads();
  const int nf = s_ncand, K = nl + nf;
  // window key frame k: the locals as listed, a fixed member at n_local + its rank by key
  for (int i = threadIdx.x; i < K; i += blockDim.x) {
    int m, k;
    if (i < nl) { m = a.loc_members[q0 + i]; k = i; }
    else {
      m = s_cand[i - nl];
      const unsigned long long key = cms_baw_fixed_key(s_first[m], m);
      int rank = 0;
      for (int c = 0; c < nf; ++c) { const int b = s_cand[c]; rank += cms_baw_fixed_key(s_first[b], b) < key ? 1 : 0; }
      k = nl + rank;
    }
    widx[m] = k;
    if (k < a.cap_kf) {
      const size_t at = (size_t)j * a.cap_kf + k;
      const CmsTriKF& kf = a.kf[a.d.slot[m]];
      float R[9], t[3];
      for (int c = 0; c < 9; ++c) R[c] = kf.Rcw[c];
      for (int c = 0; c < 3; ++c) t[c] = kf.tcw[c];
      double pose[7];
      cms_baw_pose(R, t, pose);
      a.kf_member[at] = m;
      a.fixed[at] = cms_baw_is_fixed(k, nl, m, fm) ? 1 : 0;
      for (int c = 0; c < 7; ++c) a.poses[7 * at + c] = pose[c];
    }
  }
  // the exclusive prefix sum of the points' edge counts, 1024 points a round
  const int* ecount = a.ecount + (size_t)j * a.pid_stride;
  int* eoff = a.eoff + (size_t)j * a.pid_stride;
  int base = 0;
  for (int p0 = 0; p0 < P; p0 += blockDim.x) {
    const int p = p0 + threadIdx.x;
    const int v = p < P ? ecount[p] : 0;
    int incl = v;
    for (int o = 1; o < 64; o <<= 1) { const int up = __shfl_up(incl, o); if (lane >= o) incl += up; }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < nwaves; ++w) { const int c = s_wave[w]; all += c; if (w < wave) before += c; }
    if (p < P) eoff[p] = base + before + incl - v;
    base += all;
    __syncthreads();
  }
  if (threadIdx.x == 0) a.counts[j] = CmsBaWindowCounts{K, nl, P, base};
}

// one thread per point.  Its observations in ascending member position: as many times as it has observations, the least member above the last one
// (a point has a handful of observations; a wavefront per point would idle most of its lanes)
extern "C" __global__ void __launch_bounds__(256) k_baw_fill(const CmsBawArgs a) {
  const int j = blockIdx.y, p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.npts[j]) return;
  const int id = a.pid[(size_t)j * a.pid_stride + p];
  if (p < a.cap_points) {
    const size_t at = (size_t)j * a.cap_points + p;
    a.point_id[at] = id;
    const bool has = id < a.t.max_points;      // (a row outside the table is never read; the call fails with `missing`)
    for (int c = 0; c < 3; ++c) a.points[3 * at + c] = has ? (double)a.t.pos[3 * (size_t)id + c] : 0.0;
  }
  int at_e = a.eoff[(size_t)j * a.pid_stride + p];
  if (a.ecount[(size_t)j * a.pid_stride + p] == 0) return;
  const int u = covis_find(a.d, id);
  if (u < 0) return;
  const int e0 = a.d.off[u], e1 = e0 + a.d.cnt[u];
  const int* widx = a.widx + (size_t)j * a.d.M;
  int last = -1;
  for (int step = e0; step < e1; ++step) {
    int m = 0x7FFFFFFF, em = -1;
    for (int e = e0; e < e1; ++e) { const int x = a.d.obs[e].x; if (x > last && x < m) { m = x; em = e; } }
    if (em < 0) break;      // (cannot happen: the members of a segment are distinct)
    last = m;
    size_t row;
    const int face = baw_obs_face(a, em, &row);
    if (face < 0) continue;
    if (at_e < a.cap_edges) {
      const size_t at = (size_t)j * a.cap_edges + at_e;
      double uv[2];
      cms_baw_edge_obs(a.F, a.st_kp[row].x, a.st_kp[row].y, uv);
      a.e_pose[at] = widx[m]; a.e_point[at] = p; a.e_face[at] = (int8_t)face; a.e_feat[at] = a.d.obs_feat[em];
      a.e_obs[2 * at] = uv[0]; a.e_obs[2 * at + 1] = uv[1];
      a.e_invsig2[at] = (double)a.inv_sigma2[a.d.obs[em].y & 15];
    }
    ++at_e;
  }
}
