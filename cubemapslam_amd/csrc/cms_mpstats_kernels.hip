// cms_mpstats_kernels.hip -- map-point statistics on the resident stores (csrc/cms_mpstats_core.h states the rules; host side in
// cms_api_mpstats.hip).  gfx950, wave64.  Included by cms_lib.hip behind cms_covis_kernels.hip (CmsCovisDev, covis_find), cms_mappoint_kernels.hip
// (CmsMpTable, mp_row_clear) and cms_tri_kernels.hip (CmsTriKF).  Plain HIP: global atomicAdd, wave shuffles, LDS.
//
// Resources (hipcc's kernel-resource-usage):
//   k_mp_gather_stats     10 VGPRs, no LDS, no scratch, eight waves per SIMD
//   k_mp_count             4 VGPRs, no LDS, no scratch, eight waves per SIMD: one load or two and an atomic per entry.  The loads go to mapped host
//                         memory; at 384 000 entries the kernel and the wait for it are under 0.07 ms of the call's 1.17 (profiles/mpstats.md)
//   k_mp_culling          18 VGPRs, no LDS, no scratch, eight waves per SIMD: one wavefront per id; the verdict is four loads behind covis_find, the
//                         application strides the id's segment with dependent loads (observation -> member's slot -> mp row)
//   k_covis_tracked       14 VGPRs, no LDS, no scratch, eight waves per SIMD: one wavefront per job
//   k_kf_scene_median     22 VGPRs, no static LDS, no scratch, eight waves per SIMD by registers; dynamic LDS of 4 bytes per feature of the longest
//                         named row + 16 (8 KB at 2 000 features, 64 KB at 16 383).  One WORKGROUP of 256 per slot: a wavefront per slot would spare
//                         the two barriers of a probe, but a call names ~21 slots on a chip of 256 CUs, so the call is as long as one slot's 32 probes,
//                         and four wavefronts walk a row of 2 000 keys four times faster; with 21 groups on the chip occupancy is no concern
#include "cms_mpstats_core.h"

// ---- cms_mpstore_fetch_stats: the three columns of rows named by id
extern "C" __global__ void __launch_bounds__(256) k_mp_gather_stats(const CmsMpTable t, int n, const int* __restrict__ ids, int* __restrict__ visible, int* __restrict__ found,
                                                                    int* __restrict__ first_kf) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int id = ids[i];
  if (id < 0 || id >= t.max_points) return;
  visible[i] = t.visible[id]; found[i] = t.found[id]; first_kf[i] = t.first_kf[id];
}

// ---- cms_mpstore_count: one thread per entry of all jobs (a job is a range of entries and nothing more to the kernel).  ids and flag are read from
// a pinned block
extern "C" __global__ void __launch_bounds__(256) k_mp_count(int* __restrict__ column, int max_points, const int* __restrict__ ids, const uint8_t* __restrict__ flag, int count_if,
                                                             int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int id = ids[i];
  if (id < 0 || id >= max_points) return;      // -1: no point (the host has refused anything else outside the table)
  if (flag && (flag[i] != 0) != (count_if != 0)) return;
  atomicAdd(&column[id], 1);
}

// ---- cms_mpstore_culling: one wavefront per id.  Lane 0's verdict is the wave's; for a bad point the lanes stride the id's segment of the index and
// write -1 where the observing slot's row still names the id, then the table row is emptied
struct CmsMpCulling {
  CmsCovisDev d; CmsMpTable t;
  int* st_mp; int st_maxf;
  int njobs, n; const int* off; const int* ids; const int* current_kf;
  int th_obs, apply;
  uint8_t* verdict;
};
extern "C" __global__ void __launch_bounds__(256) k_mp_culling(const CmsMpCulling a) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (i >= a.n) return;           // (the whole wave)
  const int id = a.ids[i];
  if (id < 0 || id >= a.t.max_points) return;      // (the host has checked)
  int j = 0;
  while (j + 1 < a.njobs && a.off[j + 1] <= i) ++j;      // the job of entry i: a handful of jobs
  const int u = a.d.M > 0 ? covis_find(a.d, id) : -1;
  const int n_obs = u < 0 ? 0 : a.d.cnt[u];
  int v = CMS_MP_ALREADY_BAD;
  if (a.t.ref[id] >= 0) v = cms_mpstats_verdict(a.t.found[id], a.t.visible[id], a.t.first_kf[id], n_obs, a.current_kf[j], a.th_obs);
  if (lane == 0) a.verdict[i] = (uint8_t)v;
  if (!a.apply || (v != CMS_MP_BAD_RATIO && v != CMS_MP_BAD_FEW_OBS)) return;
  if (u >= 0) {
    const int e0 = a.d.off[u];
    for (int e = lane; e < n_obs; e += 64) {
      const int m = a.d.obs[e0 + e].x, f = a.d.obs_feat[e0 + e];
      if (f < 0 || f >= a.st_maxf) continue;
      int* p = a.st_mp + (size_t)a.d.slot[m] * a.st_maxf + (size_t)f;
      if (*p == id) *p = -1;      // (an entry changed since the build is left alone)
    }
  }
  // every lane has read the row's counters above; the wave runs in lockstep, so lane 0's stores come after them
  if (lane == 0) mp_row_clear(a.t, id);
}

// ---- cms_covis_tracked_map_points: one wavefront per job, lanes stride the member's snapshot row
extern "C" __global__ void __launch_bounds__(256) k_covis_tracked(const CmsCovisDev d, int njobs, const int* __restrict__ job_member, const int* __restrict__ min_obs,
                                                                  int* __restrict__ count) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (j >= njobs) return;
  const int m = job_member[j], need = min_obs[j];
  int c = 0;
  for (int f = lane; f < d.n[m]; f += 64) {
    const int u = d.snap_u[(size_t)m * d.maxf + f];
    if (u >= 0 && (need <= 0 || d.cnt[u] >= need)) ++c;
  }
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if (lane == 0) count[j] = c;
}

// ---- cms_kfstore_scene_median_depth: one workgroup per slot.  The depth keys of the row are computed once into LDS (0xFFFFFFFF where the feature
// takes no part: the largest key, so it never lowers an answer), then the key is bisected, every probe counting with a wave and an LDS reduction
struct CmsKfMedian {
  const CmsTriKF* kf; const int* st_mp; int st_maxf;
  CmsMpTable t;
  const int* slots; int q;
  int cap;                        // keys the LDS block holds: the longest named row as the host knows it
  float* depth; int* n_depths;
};
__device__ __forceinline__ int mpstats_block_sum(int v, int* s_part) {      // the sum over a workgroup of 256; s_part: 4 ints
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();      // (the previous sum has been read)
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  return s_part[0] + s_part[1] + s_part[2] + s_part[3];
}
extern "C" __global__ void __launch_bounds__(256) k_kf_scene_median(const CmsKfMedian a) {
  extern __shared__ uint32_t s_key[];      // [4]: the partial sums, [4 + f]: the keys
  int* s_part = reinterpret_cast<int*>(s_key);
  uint32_t* key = s_key + 4;
  const int slot = a.slots[blockIdx.x];
  const CmsTriKF& k = a.kf[slot];
  const int n = min(k.n, a.cap);
  float Rcw[9], tcw[3];
  for (int c = 0; c < 9; ++c) Rcw[c] = k.Rcw[c];
  for (int c = 0; c < 3; ++c) tcw[c] = k.tcw[c];
  const int* row = a.st_mp + (size_t)slot * a.st_maxf;
  int mine = 0;
  for (int f = threadIdx.x; f < n; f += blockDim.x) {
    const int id = row[f];
    uint32_t kk = 0xFFFFFFFFu;
    if (id >= 0 && id < a.t.max_points && a.t.ref[id] >= 0) {      // a row with a position
      const float X[3] = {a.t.pos[3 * (size_t)id], a.t.pos[3 * (size_t)id + 1], a.t.pos[3 * (size_t)id + 2]};
      kk = cms_mpstats_depth_key(cms_mpstats_depth(Rcw, tcw, X));
      ++mine;
    }
    key[f] = kk;
  }
  const int nd = mpstats_block_sum(mine, s_part);      // (its barriers also publish the keys)
  if (nd == 0) {
    if (threadIdx.x == 0) { a.depth[blockIdx.x] = -1.0f; a.n_depths[blockIdx.x] = 0; }
    return;
  }
  const int idx = cms_mpstats_depth_index(nd, a.q);
  uint32_t lo = 0u, hi = 0xFFFFFFFFu;      // the smallest v with #(key <= v) > idx
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    int c = 0;
    for (int f = threadIdx.x; f < n; f += blockDim.x) c += key[f] <= mid;
    if (mpstats_block_sum(c, s_part) > idx) hi = mid; else lo = mid + 1u;
  }
  if (threadIdx.x == 0) { a.depth[blockIdx.x] = cms_mpstats_depth_from_key(lo); a.n_depths[blockIdx.x] = nd; }
}
