// cms_mappoint_kernels.hip -- the map-point table next to the key-frame store (csrc/cms_mappoint_core.h states the rules; host side in
// cms_api_mappoints.hip).  gfx950, wave64.  Included by cms_lib.hip behind cms_covis_kernels.hip (CmsCovisDev, covis_find) and cms_tri_kernels.hip
// (CmsTriKF, tri_hamming256).
//
// A row is indexed by the map point's id.  k_mp_refresh fills rows from the observation index and the store's slots, one wavefront per map point.
// The order inside an index segment depends on the order in which atomics landed when the index was built; no result here does: the descriptor's
// tie goes by the member position inside the key, and the normal is summed by walking the members in ascending position.
// Resources of k_mp_refresh (hipcc's kernel-resource-usage): 76 VGPRs, six waves per SIMD, no LDS, no scratch (no per-thread array has a runtime
// index); the kernel waits on dependent loads (segment -> member's slot -> descriptor row), so waves per SIMD are what hides them.
#include "cms_mappoint_core.h"
#include "cms_mpstats_core.h"

struct CmsMpTable {
  int max_points;
  float* pos; float* normal;      // [max_points x 3]
  float* min_dist; float* max_dist;
  uint4* desc;                    // [max_points x 2]
  int* ref;                       // mpRefKF as a store slot, -1: an empty row
  int2* best;                     // (member, feature) the descriptor was taken from, (-1, -1): none
  int* visible; int* found;       // mnVisible, mnFound (cms_mpstats_core.h); an empty row: 1, 1
  int* first_kf;                  // mnFirstKFid, -1: an empty row
};

// ---- cms_mpstore_set / cms_mpstore_erase: six words per record read from a pinned block: id, flags, pos[3], ref.  A statistics record
// (cms_mpstore_set_stats / add_stats) carries first_kf, visible, found in the three position words: absolute values, or with CMS_MP_REC_ADD the
// amounts to add (nothing else adds to the row meanwhile: the store's stream is behind every counting call)
#define CMS_MP_REC_POS 1
#define CMS_MP_REC_REF 2
#define CMS_MP_REC_ERASE 4
#define CMS_MP_REC_FIRST_KF 8
#define CMS_MP_REC_VISIBLE 16
#define CMS_MP_REC_FOUND 32
#define CMS_MP_REC_ADD 64
// the erase state of a row (cms_mpstore_create fills the table with it)
__device__ __forceinline__ void mp_row_clear(const CmsMpTable& t, int id) {
  for (int k = 0; k < 3; ++k) { t.pos[3 * (size_t)id + k] = 0.0f; t.normal[3 * (size_t)id + k] = 0.0f; }
  t.min_dist[id] = 0.0f; t.max_dist[id] = 0.0f;
  t.desc[2 * (size_t)id] = make_uint4(0, 0, 0, 0); t.desc[2 * (size_t)id + 1] = make_uint4(0, 0, 0, 0);
  t.ref[id] = -1; t.best[id] = make_int2(-1, -1);
  t.visible[id] = CMS_MP_EMPTY_VISIBLE; t.found[id] = CMS_MP_EMPTY_FOUND; t.first_kf[id] = CMS_MP_EMPTY_FIRST_KF;
}
extern "C" __global__ void __launch_bounds__(256) k_mp_set(const CmsMpTable t, const int* __restrict__ rec, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int* r = rec + 6 * (size_t)i;
  const int id = r[0], flags = r[1];
  if (id < 0 || id >= t.max_points) return;      // (the host has checked; a row outside the table is never written)
  if (flags & CMS_MP_REC_ERASE) { mp_row_clear(t, id); return; }
  if (flags & (CMS_MP_REC_FIRST_KF | CMS_MP_REC_VISIBLE | CMS_MP_REC_FOUND)) {
    const int add = flags & CMS_MP_REC_ADD;
    if (flags & CMS_MP_REC_FIRST_KF) t.first_kf[id] = r[2];
    if (flags & CMS_MP_REC_VISIBLE) t.visible[id] = add ? t.visible[id] + r[3] : r[3];
    if (flags & CMS_MP_REC_FOUND) t.found[id] = add ? t.found[id] + r[4] : r[4];
    return;
  }
  if (flags & CMS_MP_REC_POS) for (int k = 0; k < 3; ++k) t.pos[3 * (size_t)id + k] = __int_as_float(r[2 + k]);
  if (flags & CMS_MP_REC_REF) t.ref[id] = r[5];
}

// ---- rows named by id into arrays of n entries (any destination may be NULL): cms_mpstore_fetch and the two consumers' staged blocks
struct CmsMpGather {
  CmsMpTable t;
  int n; const int* ids;
  float* pos; float* normal; float* min_dist; float* max_dist; uint4* desc; int* best_member; int* best_feature;
};
extern "C" __global__ void __launch_bounds__(256) k_mp_gather(const CmsMpGather a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const int id = a.ids[i];
  if (id < 0 || id >= a.t.max_points) return;
  if (a.pos) for (int k = 0; k < 3; ++k) a.pos[3 * (size_t)i + k] = a.t.pos[3 * (size_t)id + k];
  if (a.normal) for (int k = 0; k < 3; ++k) a.normal[3 * (size_t)i + k] = a.t.normal[3 * (size_t)id + k];
  if (a.min_dist) a.min_dist[i] = a.t.min_dist[id];
  if (a.max_dist) a.max_dist[i] = a.t.max_dist[id];
  if (a.desc) { a.desc[2 * (size_t)i] = a.t.desc[2 * (size_t)id]; a.desc[2 * (size_t)i + 1] = a.t.desc[2 * (size_t)id + 1]; }
  if (a.best_member) a.best_member[i] = a.t.best[id].x;
  if (a.best_feature) a.best_feature[i] = a.t.best[id].y;
}

// ---- cms_mpstore_refresh: one wavefront per map point
struct CmsMpRefresh {
  CmsCovisDev d;                  // the index: segments of (member, octave) with the feature beside them, the members' slots
  const CmsTriKF* kf;             // the store's slot records (Ow)
  const uint4* st_desc; int st_maxf;
  CmsMpTable t;
  int n; const int* ids; int what;
  float sf[16]; int nlevels;
  uint8_t* status;
};
extern "C" __global__ void __launch_bounds__(256) k_mp_refresh(const CmsMpRefresh a) {
  const int lane = threadIdx.x & 63;
  const int p = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (p >= a.n) return;           // (the whole wave)
  const int id = a.ids[p];
  const int u = covis_find(a.d, id);
  if (u < 0) { if (lane == 0) a.status[p] = CMS_MP_NO_OBSERVATION; return; }
  const int e0 = a.d.off[u], N = a.d.cnt[u];
  const int2* obs = a.d.obs + e0;
  const int* feat = a.d.obs_feat + e0;
  // the observation whose member lives in the reference slot (a slot is a member once: at most one lane finds it)
  const int ref = a.t.ref[id];
  int ref_oct = -1;
  for (int i = lane; i < N; i += 64) { const int2 o = obs[i]; if (a.d.slot[o.x] == ref) ref_oct = o.y & 15; }
  for (int o = 32; o > 0; o >>= 1) ref_oct = max(ref_oct, __shfl_xor(ref_oct, o));
  if ((a.what & CMS_MP_NORMAL_DEPTH) && ref_oct < 0) { if (lane == 0) a.status[p] = CMS_MP_NO_REFERENCE; return; }

  if (a.what & CMS_MP_DESCRIPTOR) {
    // lane i owns observations i, i + 64, ...: the median of a row of the distance matrix by bisection on the value (distances are integers in
    // [0, 256]; the smallest v with #(d <= v) > idx is sorted[idx]), each probe recomputing the row from the slots' descriptors, as k_distinctive does
    const int idx = cms_mp_median_index(N);
    int best = 0x7FFFFFFF;
    for (int i = lane; i < N; i += 64) {
      const int mi = obs[i].x;
      const size_t ri = (size_t)a.d.slot[mi] * a.st_maxf + (size_t)feat[i];
      const uint4 a0 = a.st_desc[2 * ri], a1 = a.st_desc[2 * ri + 1];
      int lo = 0, hi = 256;
#pragma unroll 1
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        int cnt = 0;
#pragma clang loop unroll(disable)      // (unrolled, by itself or by a count of 2, the compiler keeps 16 rows in flight: 202-229 VGPRs, two waves per SIMD)
        for (int k = 0; k < N; ++k) {
          const size_t rk = (size_t)a.d.slot[obs[k].x] * a.st_maxf + (size_t)feat[k];
          cnt += tri_hamming256(a0, a1, a.st_desc[2 * rk], a.st_desc[2 * rk + 1]) <= mid;
        }
        if (cnt > idx) hi = mid; else lo = mid + 1;
      }
      best = min(best, cms_mp_best_key(lo, mi));
    }
    for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o));
    const int mbest = cms_mp_best_key_member(best);
    for (int i = lane; i < N; i += 64)
      if (obs[i].x == mbest) {      // (an id is in a member's row once: one lane)
        const size_t ri = (size_t)a.d.slot[mbest] * a.st_maxf + (size_t)feat[i];
        a.t.desc[2 * (size_t)id] = a.st_desc[2 * ri]; a.t.desc[2 * (size_t)id + 1] = a.st_desc[2 * ri + 1];
        a.t.best[id] = make_int2(mbest, feat[i]);
      }
  }

  if (a.what & CMS_MP_NORMAL_DEPTH) {
    // the members in ascending position: N times the smallest member above the last one.  Every lane carries the same running sum
    const float P[3] = {a.t.pos[3 * (size_t)id], a.t.pos[3 * (size_t)id + 1], a.t.pos[3 * (size_t)id + 2]};
    float nrm[3] = {0.0f, 0.0f, 0.0f};
    int last = -1;
    for (int step = 0; step < N; ++step) {
      int m = 0x7FFFFFFF;
      for (int i = lane; i < N; i += 64) { const int x = obs[i].x; if (x > last && x < m) m = x; }
      for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
      if (m == 0x7FFFFFFF) break;      // (cannot happen: N distinct members)
      const float* Ow = a.kf[a.d.slot[m]].Ow;
      const float ow[3] = {Ow[0], Ow[1], Ow[2]};
      cms_mp_normal_add(nrm, P, ow);
      last = m;
    }
    if (lane == 0) {
      float out[3], mn, mx;
      cms_mp_normal_finish(nrm, N, out);
      const float* Or = a.kf[ref].Ow;
      const float orf[3] = {Or[0], Or[1], Or[2]};
      cms_mp_bounds(P, orf, a.sf[ref_oct], a.sf[a.nlevels - 1], &mn, &mx);
      a.t.normal[3 * (size_t)id] = out[0]; a.t.normal[3 * (size_t)id + 1] = out[1]; a.t.normal[3 * (size_t)id + 2] = out[2];
      a.t.min_dist[id] = mn; a.t.max_dist[id] = mx;
    }
  }
  if (lane == 0) a.status[p] = CMS_MP_DONE;
}
