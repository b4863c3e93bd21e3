// cms_kfdb_kernels.hip -- KeyFrameDatabase::DetectRelocalizationCandidates / DetectLoopCandidates (src/KeyFrameDatabase.cpp:81-314) and the score()
// loop of LoopClosing::DetectLoop (src/LoopClosing.cpp:125-138) on resident BowVectors.  The numeric definition is csrc/cms_kfdb_core.h, shared with
// the host build; the contract is bit equality with CmsKfdbHost::detect (tests/test_gpu_kfdb.py).  Included by cms_lib.hip behind
// cms_vocab_kernels.hip (voc_sort, voc_scan, CMS_VOC_THREADS).
//
// The entries of a call are the database's slots in add order: entry e is the slot with the e-th smallest add sequence number, so an entry's index
// is the second half of the list key.  Q queries x E entries:
//   k_kfdb_common   a workgroup per (query, 4 entries), the query's word ids staged once in LDS (sized to the call's longest query), a wavefront per
//                   entry: lanes stride over the entry's words and binary-search the LDS copy; ballot + popcount gives the common words, a wave
//                   minimum the smallest common word.  Entries of another group and, in loop mode, the connected ones write 0.  The query's
//                   maxCommonWords is an integer atomic maximum (the order of integer maxima changes nothing).
//   k_kfdb_score    the same grid, only pairs over the threshold work: a lane per entry word finds its partner and makes the term, then EVERY lane adds
//                   the found terms in ascending lane order (terms broadcast lane by lane: ONE sequential double sum, as k_vocab_build's norm).
//   k_kfdb_carry    a thread per entry walks the call's queries in job order and leaves, per query, the reloc_score that query's accumulation
//                   sees; at the end the persistent value.  "As if one query after the other" for one launch.
//   k_kfdb_select   a workgroup per query: bitonic sort of the sharing list's keys in LDS (voc_sort), per list position the float accumulation over
//                   the <= 10 covisibles in stored order, a maximum, the 0.75f cut, first occurrence per best key frame (an integer atomic minimum
//                   of list positions), an ordered compaction (voc_scan).
// No kernel uses scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include "cms_kfdb_core.h"

#define CMS_KFDB_WAVES 4                       // entries per workgroup of k_kfdb_common / k_kfdb_score
#define CMS_KFDB_MAX_ENTRIES 16384             // the select kernel's LDS sort: 16384 x 8 B = 128 KB of the CU's 160 KB
#define CMS_KFDB_SKIP 0xFFFFFFFEFFFFFFFFull    // a list position that is not in lScoreAndMatch

struct CmsKfdbDevQuery {
  int mode, group, nwords, n_conn;
  const int* word_id; const double* word_val;      // ascending ids
  const int* conn;                                 // LOOP: entry indices of the connected key frames that are in the database
  float min_score;
};
struct CmsKfdbDevEntry { int slot, group, nwords, reset; };      // reset: added since the last call (reloc_score starts at 0.0f)
struct CmsKfdbArgs {
  int Q, E, maxf, cap;
  const CmsKfdbDevQuery* q; const CmsKfdbDevEntry* ent;
  const int* covis;                                // E x CMS_KFDB_COVIS entry indices, -1: none / not in the database
  const int* word_id; const double* word_val;      // the store's BowVectors, maxf per slot
  int* maxc;                                       // [Q] zeroed by the upload
  int* common; int* first; float* score; float* seen; int* firstpos;      // [Q x E]
  float* reloc;                                    // [slots] persistent
  int* cand; int* ncand;                           // [Q x cap], [Q]
};

__device__ __forceinline__ void kfdb_stage_query(int* qs, const CmsKfdbDevQuery& q) {
  for (int i = (int)threadIdx.x; i < q.nwords; i += (int)blockDim.x) qs[i] = q.word_id[i];
  __syncthreads();
}

// the ordered sum of L1 terms over the common words of (query, entry) by one wavefront; every lane returns the same double
__device__ __forceinline__ double kfdb_wave_sum(const int* qs, int qn, const double* qv, const int* ew, const double* ev, int n, int lane) {
  double s = 0.0;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    double x = 0.0;
    bool f = false;
    if (i < n) {
      const int id = ew[i];
      const int p = cms_kfdb_lower_bound(qs, qn, id);
      if (p < qn && qs[p] == id) { f = true; x = cms_kfdb_l1_term(qv[p], ev[i]); }
    }
    unsigned long long m = __ballot(f);
    while (m) {      // (wave-uniform: ascending lanes are ascending word ids)
      const int j = __ffsll((long long)m) - 1;
      s += __shfl(x, j, 64);
      m &= m - 1;
    }
  }
  return s;
}

__global__ void __launch_bounds__(64 * CMS_KFDB_WAVES) k_kfdb_common(CmsKfdbArgs a) {
  extern __shared__ int kfdb_qs[];
  const int qi = (int)blockIdx.y;
  const CmsKfdbDevQuery q = a.q[qi];
  kfdb_stage_query(kfdb_qs, q);
  const int e = (int)blockIdx.x * CMS_KFDB_WAVES + (int)threadIdx.x / 64, lane = (int)threadIdx.x & 63;
  if (e >= a.E) return;
  const CmsKfdbDevEntry en = a.ent[e];
  bool take = en.group == q.group;
  if (take && q.mode == CMS_KFDB_LOOP) {
    bool hit = false;
    for (int i = lane; i < q.n_conn; i += 64) hit = hit || q.conn[i] == e;
    if (__ballot(hit)) take = false;
  }
  int cnt = 0, first = INT_MAX;
  if (take) {
    const int* ew = a.word_id + (size_t)en.slot * a.maxf;
    for (int base = 0; base < en.nwords; base += 64) {
      const int i = base + lane;
      bool f = false;
      if (i < en.nwords) {
        const int id = ew[i];
        const int p = cms_kfdb_lower_bound(kfdb_qs, q.nwords, id);
        f = p < q.nwords && kfdb_qs[p] == id;
        if (f && id < first) first = id;
      }
      cnt += __popcll(__ballot(f));
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const int o = __shfl_xor(first, m, 64);
      first = o < first ? o : first;
    }
  }
  if (lane == 0) {
    const size_t idx = (size_t)qi * a.E + e;
    a.common[idx] = cnt; a.first[idx] = cnt > 0 ? first : -1;
    if (cnt > 0) atomicMax(a.maxc + qi, cnt);
  }
}

__global__ void __launch_bounds__(64 * CMS_KFDB_WAVES) k_kfdb_score(CmsKfdbArgs a) {
  extern __shared__ int kfdb_qs[];
  const int qi = (int)blockIdx.y;
  const CmsKfdbDevQuery q = a.q[qi];
  kfdb_stage_query(kfdb_qs, q);
  const int e = (int)blockIdx.x * CMS_KFDB_WAVES + (int)threadIdx.x / 64, lane = (int)threadIdx.x & 63;
  if (e >= a.E) return;
  const size_t idx = (size_t)qi * a.E + e;
  float si = -1.0f;
  if (a.common[idx] > cms_kfdb_min_common(a.maxc[qi])) {
    const CmsKfdbDevEntry en = a.ent[e];
    const double s = kfdb_wave_sum(kfdb_qs, q.nwords, q.word_val, a.word_id + (size_t)en.slot * a.maxf, a.word_val + (size_t)en.slot * a.maxf, en.nwords, lane);
    si = cms_kfdb_score_float(cms_kfdb_l1_finish(s));
  }
  if (lane == 0) a.score[idx] = si;
}

__global__ void __launch_bounds__(256) k_kfdb_carry(CmsKfdbArgs a) {
  const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (e >= a.E) return;
  const CmsKfdbDevEntry en = a.ent[e];
  float r = en.reset ? 0.0f : a.reloc[en.slot];
  for (int qi = 0; qi < a.Q; ++qi) {
    const size_t idx = (size_t)qi * a.E + e;
    if (a.q[qi].mode == CMS_KFDB_RELOC && a.common[idx] > cms_kfdb_min_common(a.maxc[qi])) r = a.score[idx];      // pKFi->mRelocScore=si (:255)
    a.seen[idx] = r;
  }
  a.reloc[en.slot] = r;
}

__global__ void __launch_bounds__(CMS_VOC_THREADS) k_kfdb_select(CmsKfdbArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long kfdb_keys[];
  __shared__ unsigned scan_buf[CMS_VOC_THREADS];
  __shared__ float red[CMS_VOC_THREADS];
  const int qi = (int)blockIdx.x, tid = (int)threadIdx.x, E = a.E;
  const CmsKfdbDevQuery q = a.q[qi];
  const size_t base = (size_t)qi * E;
  const bool loop = q.mode == CMS_KFDB_LOOP;
  const int minc = cms_kfdb_min_common(a.maxc[qi]);
  int P = CMS_VOC_THREADS;
  while (P < E) P <<= 1;
  const int C = P / CMS_VOC_THREADS, i0 = tid * C;
  // lKFsSharingWords in the reference's order
  for (int i = tid; i < P; i += CMS_VOC_THREADS) {
    unsigned long long key = CMS_KFDB_NOKEY;
    if (i < E) {
      if (a.common[base + i] > 0) key = cms_kfdb_list_key(a.first[base + i], i);
      __hip_atomic_store(a.firstpos + base + i, INT_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    kfdb_keys[i] = key;
  }
  __syncthreads();
  voc_sort(kfdb_keys, P);
  // lScoreAndMatch -> lAccScoreAndMatch (:153-178, :267-292), a list position per step; the key's place takes (accScore, pBestKF)
  float best_acc = loop ? q.min_score : 0.0f;
  for (int p = i0; p < i0 + C; ++p) {
    const unsigned long long key = kfdb_keys[p];
    if (key == CMS_KFDB_NOKEY) break;      // (the list sorts in front)
    const int e = (int)(unsigned)(key & 0xFFFFFFFFull);
    const float si = a.score[base + e];
    if (!(a.common[base + e] > minc) || (loop && !(si >= q.min_score))) { kfdb_keys[p] = CMS_KFDB_SKIP; continue; }
    float acc = si, best = si;
    int who = e;
    for (int c = 0; c < CMS_KFDB_COVIS; ++c) {
      const int r = a.covis[(size_t)e * CMS_KFDB_COVIS + c];
      if (r < 0) continue;
      const int cr = a.common[base + r];
      if (cr == 0 || (loop && !(cr > minc))) continue;      // mnRelocQuery==F->mnId (:278); mnLoopQuery==pKF->mnId && mnLoopWords>minCommonWords (:164)
      const float v = loop ? a.score[base + r] : a.seen[base + r];
      acc += v;
      if (v > best) { who = r; best = v; }
    }
    kfdb_keys[p] = ((unsigned long long)__float_as_uint(acc) << 32) | (unsigned)who;
    if (acc > best_acc) best_acc = acc;
  }
  red[tid] = best_acc;
  __syncthreads();
  for (int d = CMS_VOC_THREADS / 2; d >= 1; d >>= 1) {
    if (tid < d && red[tid + d] > red[tid]) red[tid] = red[tid + d];
    __syncthreads();
  }
  const float retain = cms_kfdb_retain(red[0]);
  // the first list position per best key frame among the retained
  for (int p = i0; p < i0 + C; ++p) {
    const unsigned long long key = kfdb_keys[p];
    if (key == CMS_KFDB_NOKEY) break;
    if ((unsigned)key == 0xFFFFFFFFu) continue;
    if (__uint_as_float((unsigned)(key >> 32)) > retain) atomicMin(a.firstpos + base + (unsigned)key, p);
  }
  __syncthreads();
  unsigned mine = 0;
  for (int p = i0; p < i0 + C; ++p) {
    const unsigned long long key = kfdb_keys[p];
    if (key == CMS_KFDB_NOKEY) break;
    if ((unsigned)key == 0xFFFFFFFFu) continue;
    if (__uint_as_float((unsigned)(key >> 32)) > retain && __hip_atomic_load(a.firstpos + base + (unsigned)key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == p) ++mine;
  }
  unsigned total;
  unsigned at = voc_scan(mine, scan_buf, &total);
  for (int p = i0; p < i0 + C; ++p) {
    const unsigned long long key = kfdb_keys[p];
    if (key == CMS_KFDB_NOKEY) break;
    if ((unsigned)key == 0xFFFFFFFFu) continue;
    if (__uint_as_float((unsigned)(key >> 32)) > retain && __hip_atomic_load(a.firstpos + base + (unsigned)key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == p) {
      if ((int)at < a.cap) a.cand[(size_t)qi * a.cap + at] = a.ent[(unsigned)key].slot;
      ++at;
    }
  }
  if (tid == 0) a.ncand[qi] = (int)total;
}

// LoopClosing::DetectLoop's score() loop (:125-138): a wavefront per pair of slots, v1 = slot a
struct CmsKfdbPairs { int n, maxf; const int* slot_a; const int* slot_b; const int* word_id; const double* word_val; const int* nwords; double* score; };
__global__ void __launch_bounds__(64 * CMS_KFDB_WAVES) k_kfdb_pair_score(CmsKfdbPairs a) {
  const int i = (int)blockIdx.x * CMS_KFDB_WAVES + (int)threadIdx.x / 64, lane = (int)threadIdx.x & 63;
  if (i >= a.n) return;
  const size_t sa = (size_t)a.slot_a[i] * a.maxf, sb = (size_t)a.slot_b[i] * a.maxf;
  const double s = kfdb_wave_sum(a.word_id + sa, a.nwords[a.slot_a[i]], a.word_val + sa, a.word_id + sb, a.word_val + sb, a.nwords[a.slot_b[i]], lane);
  if (lane == 0) a.score[i] = cms_kfdb_l1_finish(s);
}
