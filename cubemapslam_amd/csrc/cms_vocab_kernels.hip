// cms_vocab_kernels.hip -- ORBVocabulary::transform(descriptors, BowVector, FeatureVector, levelsup) on the device (DBoW2 TemplatedVocabulary.h:1127-1259,
// BowVector.cpp:34-84): k_vocab_descend walks every feature of every requested row down the tree in one launch, k_vocab_build turns a row's
// per-feature results into its two vectors (one workgroup per row).  The numeric definition is csrc/cms_vocab_core.h, shared with the host build; the
// contract is bit equality with cms_vocab_transform_host (tests/test_gpu_vocab.py).
//
// Descent: one feature per group of G lanes (G = 16 for k <= 16, 32 up to the format's k = 20).  Lane c takes child c: two uint4 loads, XOR and
// popcount, then a minimum over cms_vocab_key(distance, child) across the group -- the lowest child wins a tie, as the reference's strict `<` does.
// L dependent gathers per feature, so the kernel is latency bound: 256-thread workgroups, few registers, many features in flight per compute unit.
// The node table (35 MB for ORBvoc.txt's 1.08 M nodes) is read-only and lives in the Infinity Cache between calls; its top levels stay in L2.
//
// Build: keys (node id << 14 | feature) of the features whose word has weight > 0 are sorted in LDS (bitonic, 64-bit keys: 21 + 14 bits), segment
// heads give node_id / node_off, the sorted order is node_feat (features ascend inside a node because the key carries the index).  The words are
// sorted the same way; a head lane takes its word's count from the distance to the next head and adds w to itself count - 1 times (addWeight).
// The norm is summed by ONE wave in ascending word order, every lane making the same additions on values broadcast lane by lane -- sequential as
// BowVector::normalize is.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cms_vocab_core.h"

#define CMS_VOC_THREADS 256
#define CMS_VOC_FEAT_BITS 14

// one row of work: n descriptors in, the per-feature results and the two vectors out (arrays of n entries, node_off n + 1, counts 3)
struct CmsVocRow {
  const uint32_t* desc;            // n x 8 words, 32-byte aligned
  int n;
  int* feat_word;                  // word id, or ~word id when the word's weight is <= 0 (the feature enters neither vector)
  int* feat_nid;                   // node id at level L - levelsup
  int* word_id; double* word_val;  // BowVector, ascending word id
  int* node_id; int* node_off; int* node_feat;      // FeatureVector as CSR, ascending node id
  int* feat_node;                  // may be NULL: feature -> index of its node in node_id, -1 for none (the key-frame store's feat_node)
  int* counts;                     // words, nodes, features listed
};

template <int G>
__global__ void __launch_bounds__(CMS_VOC_THREADS) k_vocab_descend(CmsVocabView v, const CmsVocRow* __restrict__ rows, int levelsup) {
  const CmsVocRow r = rows[blockIdx.y];
  const int f = blockIdx.x * (CMS_VOC_THREADS / G) + (int)threadIdx.x / G;
  const int c = (int)threadIdx.x % G;
  if (f >= r.n) return;      // (a whole group leaves together)
  const uint4* fd = reinterpret_cast<const uint4*>(r.desc + 8 * (size_t)f);
  const uint4 a = fd[0], b = fd[1];
  const uint32_t fw[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  const int nid_level = v.L - levelsup;
  int node = 0, level = 0, nid_out = nid_level <= 0 ? 0 : -1;
  uint32_t inf = v.info[0];
  do {
    ++level;
    const int first = (int)(inf >> 5), nc = (int)(inf & 31u);
    uint32_t key = 0xFFFFFFFFu;
    if (c < nc) {
      const uint4* cd = reinterpret_cast<const uint4*>(v.desc + 8 * (size_t)(first + c));
      const uint4 p = cd[0], q = cd[1];
      const uint32_t cw[8] = {p.x, p.y, p.z, p.w, q.x, q.y, q.z, q.w};
      key = cms_vocab_key(cms_vocab_distance(fw, cw), c);
    }
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)key, m, G);
      key = o < key ? o : key;
    }
    node = first + (int)(key & 0xFFu);
    if (level == nid_level) nid_out = v.file_id[node];
    inf = v.info[node];
  } while (inf & 31u);
  if (c == 0) {
    if (nid_out < 0) nid_out = v.file_id[node];      // a leaf above the nid level
    const int w = v.word[node];
    r.feat_word[f] = v.word_weight[w] > 0 ? w : ~w;
    r.feat_nid[f] = nid_out;
  }
}

// ascending bitonic sort of P (a power of two >= CMS_VOC_THREADS) 64-bit keys in LDS by the whole workgroup
__device__ __forceinline__ void voc_sort(unsigned long long* keys, int P) {
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = (int)threadIdx.x; t < P / 2; t += CMS_VOC_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
        const unsigned long long x = keys[i], y = keys[p];
        if ((x > y) == ((i & k) == 0)) { keys[i] = y; keys[p] = x; }
      }
      __syncthreads();
    }
}
// exclusive scan of one packed pair of counts per thread (heads << 16 | valid, each < 2^14 in total); *total receives the sum
__device__ __forceinline__ unsigned voc_scan(unsigned mine, unsigned* buf, unsigned* total) {
  const int t = (int)threadIdx.x;
  buf[t] = mine;
  __syncthreads();
  for (int d = 1; d < CMS_VOC_THREADS; d <<= 1) {
    const unsigned add = t >= d ? buf[t - d] : 0u;
    __syncthreads();
    buf[t] += add;
    __syncthreads();
  }
  *total = buf[CMS_VOC_THREADS - 1];
  const unsigned excl = buf[t] - mine;
  __syncthreads();
  return excl;
}

#define CMS_VOC_NOKEY 0xFFFFFFFFFFFFFFFFull

__global__ void __launch_bounds__(CMS_VOC_THREADS) k_vocab_build(CmsVocabView v, const CmsVocRow* __restrict__ rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long voc_keys[];
  __shared__ unsigned scan_buf[CMS_VOC_THREADS];
  __shared__ double norm_sh;
  __shared__ int first_head[CMS_VOC_THREADS];
  const CmsVocRow r = rows[blockIdx.x];
  const int n = r.n, tid = (int)threadIdx.x;
  int P = CMS_VOC_THREADS;
  while (P < n) P <<= 1;
  const int C = P / CMS_VOC_THREADS, i0 = tid * C;

  // ---- FeatureVector: fv.addFeature(nid, i_feature) for every feature that is not stopped
  for (int i = tid; i < P; i += CMS_VOC_THREADS) {
    unsigned long long key = CMS_VOC_NOKEY;
    if (i < n) {
      if (r.feat_word[i] >= 0) key = ((unsigned long long)(unsigned)r.feat_nid[i] << CMS_VOC_FEAT_BITS) | (unsigned)i;
      else if (r.feat_node) r.feat_node[i] = -1;
    }
    voc_keys[i] = key;
  }
  __syncthreads();
  voc_sort(voc_keys, P);
  unsigned mine = 0;
  for (int i = i0; i < i0 + C; ++i) {
    const unsigned long long key = voc_keys[i];
    if (key == CMS_VOC_NOKEY) break;      // (the listed features sort in front)
    const bool head = i == 0 || (voc_keys[i - 1] >> CMS_VOC_FEAT_BITS) != (key >> CMS_VOC_FEAT_BITS);
    mine += head ? 0x10001u : 1u;
  }
  unsigned total;
  unsigned h = voc_scan(mine, scan_buf, &total) >> 16;
  const int nnodes = (int)(total >> 16), nvalid = (int)(total & 0xFFFFu);
  for (int i = i0; i < i0 + C; ++i) {
    const unsigned long long key = voc_keys[i];
    if (key == CMS_VOC_NOKEY) break;
    const bool head = i == 0 || (voc_keys[i - 1] >> CMS_VOC_FEAT_BITS) != (key >> CMS_VOC_FEAT_BITS);
    if (head) { r.node_id[h] = (int)(key >> CMS_VOC_FEAT_BITS); r.node_off[h] = i; ++h; }
    const int feat = (int)(key & ((1u << CMS_VOC_FEAT_BITS) - 1u));
    r.node_feat[i] = feat;
    if (r.feat_node) r.feat_node[feat] = (int)h - 1;
  }
  if (tid == 0) { r.node_off[nnodes] = nvalid; r.counts[1] = nnodes; r.counts[2] = nvalid; }
  __syncthreads();

  // ---- BowVector: v.addWeight / v.addIfNotExist(id, w), then the division by v.size() or BowVector::normalize
  for (int i = tid; i < P; i += CMS_VOC_THREADS) voc_keys[i] = (i < n && r.feat_word[i] >= 0) ? (unsigned long long)(unsigned)r.feat_word[i] : CMS_VOC_NOKEY;
  __syncthreads();
  voc_sort(voc_keys, P);
  mine = 0;
  int first = -1;      // the first head of this thread's chunk
  for (int i = i0; i < i0 + C; ++i) {
    const unsigned long long key = voc_keys[i];
    if (key == CMS_VOC_NOKEY) break;
    if (i == 0 || voc_keys[i - 1] != key) { if (first < 0) first = i; ++mine; }
  }
  first_head[tid] = first;      // (published by the scan's barriers)
  h = voc_scan(mine, scan_buf, &total);
  const int nwords = (int)total;
  bool l2 = false;
  const bool must = cms_vocab_must_normalize(v.scoring, &l2);
  const bool add = v.weighting == CMS_VOC_TF || v.weighting == CMS_VOC_TF_IDF;
  // a word's count is the distance from its head to the next head: inside the chunk, else the first head of a later chunk, else the end of the keys
  int head = -1;
  for (int i = i0; i <= i0 + C; ++i) {
    const bool in_chunk = i < i0 + C && voc_keys[i] != CMS_VOC_NOKEY;
    const bool is_head = in_chunk && (i == 0 || voc_keys[i - 1] != voc_keys[i]);
    if (head >= 0 && (is_head || !in_chunk)) {
      int end = i;
      if (!is_head) {
        end = nvalid;
        for (int t = tid + 1; t < CMS_VOC_THREADS; ++t)
          if (first_head[t] >= 0) { end = first_head[t]; break; }
      }
      const unsigned long long key = voc_keys[head];
      double val = cms_vocab_word_value(v.weighting, v.word_weight[(int)key], end - head);
      if (add && !must) val /= (double)nwords;      // :1164-1170
      r.word_id[h] = (int)key; r.word_val[h] = val; ++h;
      head = -1;
    }
    if (!in_chunk) break;
    if (is_head) head = i;
  }
  if (tid == 0) r.counts[0] = nwords;
  if (!must) return;
  __syncthreads();      // the values written above are read back by the first wave (same workgroup)
  if (tid < 64) {
    double norm = 0.0;
    for (int base = 0; base < nwords; base += 64) {
      const double x = base + tid < nwords ? cms_vocab_norm_term(l2, r.word_val[base + tid]) : 0.0;      // (+ 0.0 leaves the sum as it is)
#pragma unroll
      for (int j = 0; j < 64; ++j) norm += __shfl(x, j, 64);
    }
    if (l2) norm = sqrt(norm);
    if (tid == 0) norm_sh = norm;
  }
  __syncthreads();
  const double norm = norm_sh;
  if (norm > 0.0)
    for (int i = tid; i < nwords; i += CMS_VOC_THREADS) r.word_val[i] /= norm;
}

// the key-frame store's commit: the computed vectors of one slot go from the call's scratch into the slot's layout (cms_api_tri.hip), and the
// BowVector into the store's per-slot arrays
struct CmsVocCommit {
  CmsVocRow src;
  int* o_fn; int* o_nid; int* o_noff; int* o_nfeat; int* o_kf_nnodes;
  int* o_word_id; double* o_word_val; int* o_nwords;
};
__global__ void __launch_bounds__(CMS_VOC_THREADS) k_vocab_commit(const CmsVocCommit* __restrict__ items) {
  const CmsVocCommit a = items[blockIdx.x];
  const int tid = (int)threadIdx.x, nwords = a.src.counts[0], nnodes = a.src.counts[1], nfeat = a.src.counts[2];
  for (int i = tid; i < a.src.n; i += CMS_VOC_THREADS) a.o_fn[i] = a.src.feat_node[i];
  for (int i = tid; i < nnodes; i += CMS_VOC_THREADS) a.o_nid[i] = a.src.node_id[i];
  for (int i = tid; i <= nnodes; i += CMS_VOC_THREADS) a.o_noff[i] = a.src.node_off[i];
  for (int i = tid; i < nfeat; i += CMS_VOC_THREADS) a.o_nfeat[i] = a.src.node_feat[i];
  for (int i = tid; i < nwords; i += CMS_VOC_THREADS) { a.o_word_id[i] = a.src.word_id[i]; a.o_word_val[i] = a.src.word_val[i]; }
  if (tid == 0) { *a.o_kf_nnodes = nnodes; *a.o_nwords = nwords; }
}
