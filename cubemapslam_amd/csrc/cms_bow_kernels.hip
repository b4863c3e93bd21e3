// cms_bow_kernels.hip -- ORBMatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches) (src/ORBMatcher.cpp:409-539),
// the matcher of Tracking::TrackReferenceKeyFrame (Tracking.cpp:567-618) and of Tracking::Relocalization's candidate loop (:995-1040).
// Included by cms_lib.hip after cms_track_kernels.hip (track_rot_bin, track_three_maxima) and cms_tri_kernels.hip (tri_hamming256).
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
