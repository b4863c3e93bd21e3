// cms_covis_kernels.hip -- the observation index over resident key frames and its four queries (csrc/cms_covis_core.h states the rules; host side in
// cms_api_covis.hip).  gfx950, wave64.
//
// The index is an open-addressing table over the map-point ids (2^bits >= twice the members' features, integer CAS, linear probing) with one
// segment of (member, octave) observations per id, the feature index in a parallel array (cms_mappoint_kernels.hip reads it).  Where a segment lies and the order inside it depend on the order in which atomics land; no
// result does: the queries only COUNT over segments, and the rank in `order` is a function of (weight, member position).
#include "cms_covis_core.h"

struct CmsCovisDev {
  int M, maxf, bits;
  const int* n;          // [M] features per member
  const int* snap_u;     // [M x maxf] the table entry of the feature's id, -1: no id
  const int* snap_oct;   // [M x maxf]
  const int* key;        // [2^bits] the id, -1: free
  const int* cnt;        // [2^bits] Observations(id)
  const int* off;        // [2^bits] where the id's segment starts in obs
  const int* uix;        // [2^bits] a dense number per id (the culling scratch is indexed by it)
  const int2* obs;       // (member, octave)
  const int* obs_feat;   // the observation's feature index in its member's row, parallel to obs
  const int* slot;       // [M] the store slot of a member
};

// ---- build
// an id twice in one row?  One workgroup per member sorts the row in LDS (bitonic, padded to P = 2^k) and looks at neighbours.
extern "C" __global__ void __launch_bounds__(256) k_covis_rowcheck(const int* __restrict__ slot, const int* __restrict__ n, const int* __restrict__ st_mp, int st_maxf, int P,
                                                                   int* flag) {
  extern __shared__ int s_row[];
  const int m = blockIdx.x, nm = n[m];
  const int* row = st_mp + (size_t)slot[m] * st_maxf;
  for (int i = threadIdx.x; i < P; i += blockDim.x) {
    const int v = i < nm ? row[i] : -1;
    s_row[i] = v < 0 ? 0x7FFFFFFF : v;
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < P; i += blockDim.x) {
        const int x = i ^ j;
        if (x > i) {
          const int a = s_row[i], b = s_row[x];
          if ((a > b) == ((i & k) == 0)) { s_row[i] = b; s_row[x] = a; }
        }
      }
      __syncthreads();
    }
  for (int i = threadIdx.x + 1; i < P; i += blockDim.x)
    if (s_row[i] == s_row[i - 1] && s_row[i] != 0x7FFFFFFF) *flag = 1;
}

struct CmsCovisBuild {
  int M, maxf, bits, st_maxf;
  const int* slot; const int* n;            // [M]
  const int* st_mp; const CmsKeyPoint* st_kp;
  int* snap_u; int* snap_oct; int* key; int* cnt; int* off; int* uix; int* cur; int2* obs; int* obs_feat;
  int* counters;                            // [0]: observations placed, [1]: ids numbered
};
// the snapshot of the members' rows, every live id into the table.  blockIdx.y = member
extern "C" __global__ void __launch_bounds__(256) k_covis_insert(const CmsCovisBuild a) {
  const int m = blockIdx.y, f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= a.n[m]) return;
  const size_t src = (size_t)a.slot[m] * a.st_maxf + (size_t)f, dst = (size_t)m * a.maxf + (size_t)f;
  const int id = a.st_mp[src];
  a.snap_oct[dst] = a.st_kp[src].octave;
  int u = -1;
  if (id >= 0) {
    const uint32_t mask = (1u << a.bits) - 1u;
    uint32_t p = cms_covis_hash(id, a.bits);
    for (;;) {      // (the table is at most half full: a free entry is met)
      const int prev = atomicCAS(&a.key[p], -1, id);
      if (prev == -1 || prev == id) break;
      p = (p + 1u) & mask;
    }
    atomicAdd(&a.cnt[p], 1);
    u = (int)p;
  }
  a.snap_u[dst] = u;
}
// a segment and a dense number per id
extern "C" __global__ void __launch_bounds__(256) k_covis_alloc(const CmsCovisBuild a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (1u << a.bits)) return;
  const int c = a.cnt[p];
  if (c > 0) { a.off[p] = atomicAdd(&a.counters[0], c); a.uix[p] = atomicAdd(&a.counters[1], 1); }
}
extern "C" __global__ void __launch_bounds__(256) k_covis_fill(const CmsCovisBuild a) {
  const int m = blockIdx.y, f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= a.n[m]) return;
  const size_t dst = (size_t)m * a.maxf + (size_t)f;
  const int u = a.snap_u[dst];
  if (u < 0) return;
  const int e = a.off[u] + atomicAdd(&a.cur[u], 1);      // (cur[u] stays below cnt[u]: one add per observation counted)
  a.obs[e] = make_int2(m, a.snap_oct[dst]);
  a.obs_feat[e] = f;
}

// the table entry of an id, -1: the index does not know it
__device__ __forceinline__ int covis_find(const CmsCovisDev& d, int id) {
  const uint32_t mask = (1u << d.bits) - 1u;
  uint32_t p = cms_covis_hash(id, d.bits);
  for (;;) {
    const int k = d.key[p];
    if (k == id) return (int)p;
    if (k == -1) return -1;
    p = (p + 1u) & mask;
  }
}

// ---- keyframeCounter (Tracking.cpp:885-901): one workgroup per frame, the members' counters in LDS
extern "C" __global__ void __launch_bounds__(1024) k_covis_votes(const CmsCovisDev d, const int* __restrict__ id_off, const int* __restrict__ ids, int* __restrict__ votes) {
  extern __shared__ int s_hist[];
  const int j = blockIdx.x;
  for (int m = threadIdx.x; m < d.M; m += blockDim.x) s_hist[m] = 0;
  __syncthreads();
  for (int q = id_off[j] + threadIdx.x; q < id_off[j + 1]; q += blockDim.x) {
    const int u = covis_find(d, ids[q]);
    if (u < 0) continue;
    const int e0 = d.off[u], e1 = e0 + d.cnt[u];
    for (int e = e0; e < e1; ++e) atomicAdd(&s_hist[d.obs[e].x], 1);
  }
  __syncthreads();
  for (int m = threadIdx.x; m < d.M; m += blockDim.x) votes[(size_t)j * d.M + m] = s_hist[m];
}

// ---- KFcounter and mvpOrderedConnectedKeyFrames (KeyFrame.cpp:317-394): one workgroup per key frame.  LDS: M counters, then M candidates
extern "C" __global__ void __launch_bounds__(1024) k_covis_connections(const CmsCovisDev d, const int* __restrict__ job_member, int th, int* __restrict__ weights,
                                                                       int* __restrict__ order, int* __restrict__ n_connected) {
  extern __shared__ int s_mem[];
  __shared__ int s_ncand, s_max;
  int* s_hist = s_mem;
  int* s_cand = s_mem + d.M;
  const int j = blockIdx.x, m0 = job_member[j];
  for (int m = threadIdx.x; m < d.M; m += blockDim.x) s_hist[m] = 0;
  if (threadIdx.x == 0) { s_ncand = 0; s_max = 0; }
  __syncthreads();
  for (int f = threadIdx.x; f < d.n[m0]; f += blockDim.x) {
    const int u = d.snap_u[(size_t)m0 * d.maxf + f];
    if (u < 0) continue;
    const int e0 = d.off[u], e1 = e0 + d.cnt[u];
    for (int e = e0; e < e1; ++e) { const int m = d.obs[e].x; if (m != m0) atomicAdd(&s_hist[m], 1); }
  }
  __syncthreads();
  for (int m = threadIdx.x; m < d.M; m += blockDim.x) {
    const int w = s_hist[m];
    weights[(size_t)j * d.M + m] = w;
    if (w > 0) {
      atomicMax(&s_max, cms_covis_max_key(w, m));
      if (w >= th) s_cand[atomicAdd(&s_ncand, 1)] = m;      // (in any order: the rank below does not depend on it)
    }
  }
  __syncthreads();
  const int nc = s_ncand;
  int* ord = order + (size_t)j * d.M;
  int n_out = nc;
  if (nc == 0) {      // nobody reaches th: the one of maximal weight, the earliest such; nobody at all: an empty KFcounter
    n_out = s_max > 0 ? 1 : 0;
    if (threadIdx.x == 0 && n_out) ord[0] = cms_covis_max_key_pos(s_max);
  } else {
    for (int i = threadIdx.x; i < nc; i += blockDim.x) {
      const int a = s_cand[i], wa = s_hist[a];
      int rank = 0;
      for (int k = 0; k < nc; ++k) { const int b = s_cand[k]; rank += cms_covis_before(s_hist[b], b, wa, a) ? 1 : 0; }
      ord[rank] = a;
    }
  }
  for (int i = n_out + threadIdx.x; i < d.M; i += blockDim.x) ord[i] = -1;
  if (threadIdx.x == 0) n_connected[j] = n_out;
}

// ---- KeyFrameCulling (LocalMapping.cpp:569-618): one workgroup per chain, its candidates one after the other.  dec (one int per id and chain,
// all zero on entry and again on exit) counts the observations an id has lost to the chain's removed members, -1: the id has become bad; the index is not written.
extern "C" __global__ void __launch_bounds__(1024) k_covis_culling(const CmsCovisDev d, const int* __restrict__ chain_off, const int* __restrict__ job_member,
                                                                   const uint8_t* __restrict__ erasable, int th_obs, int* dec_all, size_t dec_stride, int* __restrict__ n_mps,
                                                                   int* __restrict__ n_redundant, uint8_t* __restrict__ redundant) {
  __shared__ uint8_t s_removed[CMS_COVIS_MAX_MEMBERS];
  __shared__ int s_nm, s_nr, s_erase;
  const int c = blockIdx.x;
  int* dec = dec_all + (size_t)c * dec_stride;
  for (int m = threadIdx.x; m < d.M; m += blockDim.x) s_removed[m] = 0;
  if (threadIdx.x == 0) { s_nm = 0; s_nr = 0; s_erase = 0; }
  __syncthreads();
  for (int j = chain_off[c]; j < chain_off[c + 1]; ++j) {
    const int m0 = job_member[j], nf = d.n[m0];
    const size_t r0 = (size_t)m0 * d.maxf;
    int nm = 0, nr = 0;
    for (int f = threadIdx.x; f < nf; f += blockDim.x) {
      const int u = d.snap_u[r0 + f];
      if (u < 0) continue;
      const int lost = dec[d.uix[u]];
      if (lost < 0) continue;
      ++nm;
      if (!(d.cnt[u] - lost > th_obs)) continue;
      const int octave = d.snap_oct[r0 + f];
      int n_obs = 0;
      const int e0 = d.off[u], e1 = e0 + d.cnt[u];
      for (int e = e0; e < e1 && n_obs < th_obs; ++e) {
        const int2 o = d.obs[e];
        if (o.x == m0 || s_removed[o.x]) continue;
        if (cms_covis_octave_ok(o.y, octave)) ++n_obs;
      }
      if (n_obs >= th_obs) ++nr;
    }
    if (nm) atomicAdd(&s_nm, nm);
    if (nr) atomicAdd(&s_nr, nr);
    __syncthreads();
    if (threadIdx.x == 0) {
      const bool red = cms_covis_redundant(s_nr, s_nm);
      n_mps[j] = s_nm; n_redundant[j] = s_nr; redundant[j] = red ? 1 : 0;
      s_erase = (red && erasable[j]) ? 1 : 0;
      s_nm = 0; s_nr = 0;
      if (s_erase) s_removed[m0] = 1;
    }
    __syncthreads();
    if (s_erase) {      // SetBadFlag: every live id of the row loses one observation (an id is in a row once: no two threads meet)
      for (int f = threadIdx.x; f < nf; f += blockDim.x) {
        const int u = d.snap_u[r0 + f];
        if (u < 0) continue;
        const int x = d.uix[u], lost = dec[x];
        if (lost < 0) continue;
        dec[x] = cms_covis_point_dies(d.cnt[u] - (lost + 1)) ? -1 : lost + 1;
      }
      __threadfence_block();
    }
    __syncthreads();
  }
  // leave the scratch as it was found, all zero: only the ids of the chain's own rows were touched, so the caller clears it once, not per call
  for (int j = chain_off[c]; j < chain_off[c + 1]; ++j) {
    const int m0 = job_member[j], nf = d.n[m0];
    for (int f = threadIdx.x; f < nf; f += blockDim.x) {
      const int u = d.snap_u[(size_t)m0 * d.maxf + f];
      if (u >= 0) dec[d.uix[u]] = 0;
    }
  }
}

// ---- UpdateLocalPoints (Tracking.cpp:857-877): one workgroup per frame.  An id is taken at its first (member of the list, feature); a row holds an id
// once, so a feature is a first occurrence exactly when no EARLIER member of the list observes its id.  The write position is an ordered count.
extern "C" __global__ void __launch_bounds__(1024) k_covis_local_points(const CmsCovisDev d, const int* __restrict__ kf_off, const int* __restrict__ kf_members, int cap,
                                                                        int* __restrict__ ids_out, int* __restrict__ n_out) {
  extern __shared__ int s_listpos[];
  __shared__ int s_wave[16];
  const int j = blockIdx.x, q0 = kf_off[j], nk = kf_off[j + 1] - q0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  for (int m = threadIdx.x; m < d.M; m += blockDim.x) s_listpos[m] = -1;
  __syncthreads();
  for (int k = threadIdx.x; k < nk; k += blockDim.x) s_listpos[kf_members[q0 + k]] = k;
  __syncthreads();
  int base = 0;
  for (int k = 0; k < nk; ++k) {
    const int m0 = kf_members[q0 + k], nf = d.n[m0];
    for (int f0 = 0; f0 < nf; f0 += blockDim.x) {
      const int f = f0 + threadIdx.x;
      int u = -1;
      if (f < nf) u = d.snap_u[(size_t)m0 * d.maxf + f];
      bool first = u >= 0;
      if (first) {
        const int e0 = d.off[u], e1 = e0 + d.cnt[u];
        for (int e = e0; e < e1; ++e) { const int lp = s_listpos[d.obs[e].x]; if (lp >= 0 && lp < k) { first = false; break; } }
      }
      const unsigned long long mask = __ballot(first);
      if (lane == 0) s_wave[wave] = __popcll(mask);
      __syncthreads();
      int before = 0, all = 0;
      for (int w = 0; w < nwaves; ++w) { const int c = s_wave[w]; all += c; if (w < wave) before += c; }
      const int pos = base + before + __popcll(mask & ((1ull << lane) - 1ull));
      if (first && pos < cap) ids_out[(size_t)j * cap + pos] = d.key[u];
      base += all;
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) n_out[j] = base;
}

// ---- cms_kfstore_update_map_points: (slot, feature, id) triples read from a pinned block
extern "C" __global__ void __launch_bounds__(256) k_kf_update_map_points(int* mp, int maxf, const int* __restrict__ triples, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  mp[(size_t)triples[3 * i] * maxf + triples[3 * i + 1]] = triples[3 * i + 2];
}
