// cms_bow_kernels.hip -- ORBMatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches) (src/ORBMatcher.cpp:409-539),
// the matcher of Tracking::TrackReferenceKeyFrame (Tracking.cpp:567-618) and of Tracking::Relocalization's candidate loop (:995-1040).
// Included by cms_lib.hip after cms_track_kernels.hip (track_rot_bin, track_three_maxima) and cms_tri_kernels.hip (tri_hamming256).
// The (KeyFrame*, KeyFrame*) overload of LoopClosing (:541-674) is k_search_by_bow_kf at the end of the file.
//
// One workgroup of 16 wavefronts per job (one key frame against one frame).  The reference walks the two FeatureVectors as sorted maps and only node ids present
// in both take part; DBoW2 puts every feature into exactly one node (the host rejects a frame FeatureVector that lists a feature twice), so the
// common nodes are independent of each other and each wavefront takes whole nodes.  Inside a node the key frame's features are walked in list
// order -- a frame feature taken by one of them is skipped by the later ones -- with the 64 lanes sharing each scan over the node's frame
// features: the two smallest keys dist << 16 | position are the sequential scan's best / second best (the first minimum in list order wins, an
// equal distance becomes the second best).  The rotation histogram (ComputeThreeMaxima, :905-946) and the filter follow in the same launch.
#define CMS_BOW_THREADS 1024
#define CMS_BOW_WAVES (CMS_BOW_THREADS / 64)

struct CmsBowJob {
  // key frame: features (key points, descriptors, map-point slot >= 0 <=> GetMapPoint(i) != NULL, skip != 0 <=> isBad(); skip may be NULL) and
  // mFeatVec as CSR (node ids ascending, node_off relative to node_feat)
  const CmsKeyPoint* kf_kp; const uint4* kf_desc; const int* kf_mp; const uint8_t* kf_skip;
  const int* kf_nid; const int* kf_noff; const int* kf_nfeat; int kf_nnodes;
  // frame: n key points / descriptors on the device and F.mFeatVec as CSR
  int n, f_nnodes;
  const CmsKeyPoint* f_kp; const uint4* f_desc;
  const int* f_nid; const int* f_noff; const int* f_nfeat;
  int* kf_idx;       // n entries: key-frame feature whose map point frame feature i receives, or -1
  int* n_matches;    // nmatches after the histogram filter
};

extern "C" __global__ void __launch_bounds__(CMS_BOW_THREADS) k_search_by_bow(const CmsBowJob* __restrict__ jobs, float nnratio, int check_orientation) {
  __shared__ uint8_t s_bin[CMS_AREA_MAXKP + 1];   // per frame feature: 0 = free, else 1 + rotation bin of its match
  __shared__ int hist[32];                        // bins 0..29; 31 collects angles outside [0, 360) (never among the kept bins)
  __shared__ int keep[3];
  __shared__ int s_n;
  const CmsBowJob a = jobs[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < a.n; i += CMS_BOW_THREADS) { s_bin[i] = 0; a.kf_idx[i] = -1; }
  if (tid < 32) hist[tid] = 0;
  if (tid == 0) s_n = 0;
  __syncthreads();
  // each lane of a wavefront pairs one key-frame node with the frame's node of the same id (lower_bound, like k_tri_search), then the wavefront
  // works through the pairs it found.  Nodes are dealt out round robin (wavefront w takes nodes w, w + 16, ...): the walk inside a node is a chain of
  // dependent loads, so the time is set by the longest list of nodes one wavefront gets
  for (int base = 0; base < a.kf_nnodes; base += CMS_BOW_THREADS) {
    const int e = base + lane * CMS_BOW_WAVES + wave;
    int fe = -1;
    if (e < a.kf_nnodes) {
      const int node = a.kf_nid[e];
      int lo = 0, hi = a.f_nnodes;
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (a.f_nid[mid] < node) lo = mid + 1; else hi = mid; }
      if (lo < a.f_nnodes && a.f_nid[lo] == node) fe = lo;
    }
    unsigned long long todo = __ballot(fe >= 0);
    while (todo) {
      const int l = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int fnode = __shfl(fe, l), knode = __shfl(e, l);
      const int k0 = a.kf_noff[knode], k1 = a.kf_noff[knode + 1], f0 = a.f_noff[fnode], f1 = a.f_noff[fnode + 1];
      for (int k = k0; k < k1; ++k) {                     // ORBMatcher.cpp:437-502, in list order
        const int ikf = a.kf_nfeat[k];
        if (a.kf_mp[ikf] < 0 || (a.kf_skip && a.kf_skip[ikf])) continue;
        const uint4 d0 = a.kf_desc[2 * (size_t)ikf], d1 = a.kf_desc[2 * (size_t)ikf + 1];
        unsigned b1 = 0xFFFFFFFFu, b2 = 0xFFFFFFFFu;
        for (int p = f0 + lane; p < f1; p += 64) {
          const int iF = a.f_nfeat[p];
          if (s_bin[iF]) continue;                      // vpMapPointMatches[realIdxF] already set
          const unsigned key = ((unsigned)tri_hamming256(d0, d1, a.f_desc[2 * (size_t)iF], a.f_desc[2 * (size_t)iF + 1]) << 16) | (unsigned)(p - f0);
          if (key < b1) { b2 = b1; b1 = key; } else if (key < b2) b2 = key;
        }
        for (int o = 32; o > 0; o >>= 1) {
          const unsigned o1 = __shfl_xor(b1, o), o2 = __shfl_xor(b2, o);
          const unsigned lo = min(b1, o1), hi = max(b1, o1);
          b2 = min(hi, min(b2, o2)); b1 = lo;
        }
        const int bestDist1 = b1 == 0xFFFFFFFFu ? 256 : (int)(b1 >> 16), bestDist2 = b2 == 0xFFFFFFFFu ? 256 : (int)(b2 >> 16);
        if (bestDist1 <= 50 && (float)bestDist1 < __fmul_rn(nnratio, (float)bestDist2) && lane == 0) {      // TH_LOW, mfNNratio
          const int iF = a.f_nfeat[f0 + (int)(b1 & 0xFFFFu)];
          int bin = track_rot_bin(a.kf_kp[ikf].angle, a.f_kp[iF].angle);
          if ((unsigned)bin >= 30u) bin = 31;
          s_bin[iF] = (uint8_t)(bin + 1);
          a.kf_idx[iF] = ikf;
          if (check_orientation) atomicAdd(&hist[bin], 1);
        }
      }
    }
  }
  __syncthreads();
  if (tid == 0 && check_orientation) track_three_maxima(hist, keep);
  __syncthreads();
  int mine = 0;
  for (int i = tid; i < a.n; i += CMS_BOW_THREADS) {
    const int v = s_bin[i];
    if (!v) continue;
    if (check_orientation && v - 1 != keep[0] && v - 1 != keep[1] && v - 1 != keep[2]) { a.kf_idx[i] = -1; continue; }      // ORBMatcher.cpp:517-535
    ++mine;
  }
  if (mine) atomicAdd(&s_n, mine);
  __syncthreads();
  if (tid == 0) *a.n_matches = s_n;
}

// ORBMatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12) (src/ORBMatcher.cpp:541-674), the matcher of
// LoopClosing::ComputeSim3 (LoopClosing.cpp:264).  A contract of its own, not a parameter of the kernel above: BOTH sides are filtered by map point
// (mp >= 0, not bad), the threshold is strict (best < TH_LOW), a flag per key-frame-2 feature (vbMatched2) marks what has been taken, and the result
// is indexed by key frame 1's key points.  One workgroup per job, both key frames read from the store's arrays; nodes dealt to wavefronts and paired
// by binary search as above, the walk over key frame 1's features of a node sequential, the 64 lanes sharing each scan over the node's
// key-frame-2 features.  The store accepts any CSR, so an entry of a node's list takes part only if that node is the one the slot's feat_node
// records for the feature (for a FeatureVector of DBoW2 -- every feature in one node, once -- always): a feature then belongs to one node, hence to
// one wavefront, and s_taken / s_m1 are written without a race.  A key-frame-1 feature that holds a match is not matched again (a node that lists
// it twice).
struct CmsBowKfJob {
  // per side: features of the slot (key points, descriptors, map-point slot, feat_node), skip != 0 <=> isBad() (may be NULL), mFeatVec as CSR
  const CmsKeyPoint* kp1; const uint4* desc1; const int* mp1; const int* fn1; const uint8_t* skip1; const int* nid1; const int* noff1; const int* nfeat1;
  const CmsKeyPoint* kp2; const uint4* desc2; const int* mp2; const int* fn2; const uint8_t* skip2; const int* nid2; const int* noff2; const int* nfeat2;
  int n1, nnodes1, n2, nnodes2;
  int* idx2;         // n1 entries: key-frame-2 feature whose map point key point i of key frame 1 receives, or -1
  int* n_matches;    // nmatches after the histogram filter
};

extern "C" __global__ void __launch_bounds__(CMS_BOW_THREADS) k_search_by_bow_kf(const CmsBowKfJob* __restrict__ jobs, float nnratio, int check_orientation) {
  __shared__ uint8_t s_taken[CMS_AREA_MAXKP + 1];   // vbMatched2, per key-frame-2 feature
  __shared__ uint8_t s_m1[CMS_AREA_MAXKP + 1];      // per key-frame-1 feature: 0 = no match, else 1 + rotation bin of its match
  __shared__ int hist[32];                          // bins 0..29; 31 collects angles outside [0, 360) (never among the kept bins)
  __shared__ int keep[3];
  __shared__ int s_n;
  const CmsBowKfJob a = jobs[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < a.n2; i += CMS_BOW_THREADS) s_taken[i] = 0;
  for (int i = tid; i < a.n1; i += CMS_BOW_THREADS) { s_m1[i] = 0; a.idx2[i] = -1; }
  if (tid < 32) hist[tid] = 0;
  if (tid == 0) s_n = 0;
  __syncthreads();
  for (int base = 0; base < a.nnodes1; base += CMS_BOW_THREADS) {
    const int e = base + lane * CMS_BOW_WAVES + wave;
    int e2 = -1;
    if (e < a.nnodes1) {
      const int node = a.nid1[e];
      int lo = 0, hi = a.nnodes2;
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (a.nid2[mid] < node) lo = mid + 1; else hi = mid; }
      if (lo < a.nnodes2 && a.nid2[lo] == node) e2 = lo;
    }
    unsigned long long todo = __ballot(e2 >= 0);
    while (todo) {
      const int l = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int node2 = __shfl(e2, l), node1 = __shfl(e, l);
      const int k0 = a.noff1[node1], k1 = a.noff1[node1 + 1], f0 = a.noff2[node2], f1 = a.noff2[node2 + 1];
      for (int k = k0; k < k1; ++k) {                     // ORBMatcher.cpp:573-638, in list order
        const int i1 = a.nfeat1[k];
        if (a.fn1[i1] != node1 || s_m1[i1]) continue;
        if (a.mp1[i1] < 0 || (a.skip1 && a.skip1[i1])) continue;
        const uint4 d0 = a.desc1[2 * (size_t)i1], d1 = a.desc1[2 * (size_t)i1 + 1];
        unsigned b1 = 0xFFFFFFFFu, b2 = 0xFFFFFFFFu;
        for (int p = f0 + lane; p < f1; p += 64) {
          const int i2 = a.nfeat2[p];
          if (s_taken[i2] || a.fn2[i2] != node2 || a.mp2[i2] < 0 || (a.skip2 && a.skip2[i2])) continue;      // vbMatched2[idx2] || !pMP2, isBad()
          const unsigned key = ((unsigned)tri_hamming256(d0, d1, a.desc2[2 * (size_t)i2], a.desc2[2 * (size_t)i2 + 1]) << 16) | (unsigned)(p - f0);
          if (key < b1) { b2 = b1; b1 = key; } else if (key < b2) b2 = key;
        }
        for (int o = 32; o > 0; o >>= 1) {
          const unsigned o1 = __shfl_xor(b1, o), o2 = __shfl_xor(b2, o);
          const unsigned lo = min(b1, o1), hi = max(b1, o1);
          b2 = min(hi, min(b2, o2)); b1 = lo;
        }
        const int bestDist1 = b1 == 0xFFFFFFFFu ? 256 : (int)(b1 >> 16), bestDist2 = b2 == 0xFFFFFFFFu ? 256 : (int)(b2 >> 16);
        if (bestDist1 < 50 && (float)bestDist1 < __fmul_rn(nnratio, (float)bestDist2) && lane == 0) {      // TH_LOW (strict), mfNNratio
          const int i2 = a.nfeat2[f0 + (int)(b1 & 0xFFFFu)];
          int bin = track_rot_bin(a.kp1[i1].angle, a.kp2[i2].angle);
          if ((unsigned)bin >= 30u) bin = 31;
          s_taken[i2] = 1;
          s_m1[i1] = (uint8_t)(bin + 1);
          a.idx2[i1] = i2;
          if (check_orientation) atomicAdd(&hist[bin], 1);
        }
      }
    }
  }
  __syncthreads();
  if (tid == 0 && check_orientation) track_three_maxima(hist, keep);
  __syncthreads();
  int mine = 0;
  for (int i = tid; i < a.n1; i += CMS_BOW_THREADS) {
    const int v = s_m1[i];
    if (!v) continue;
    if (check_orientation && v - 1 != keep[0] && v - 1 != keep[1] && v - 1 != keep[2]) { a.idx2[i] = -1; continue; }      // ORBMatcher.cpp:653-671
    ++mine;
  }
  if (mine) atomicAdd(&s_n, mine);
  __syncthreads();
  if (tid == 0) *a.n_matches = s_n;
}
