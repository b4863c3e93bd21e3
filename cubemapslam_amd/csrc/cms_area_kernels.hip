// cms_area_kernels.hip -- Frame::AssignFeaturesToGrid / PosInGrid (src/Frame.cpp:158-176, 728-744) and Frame::GetFeaturesInArea
// (src/Frame.cpp:36-72, 251-716) on the device: the key points of a frame never leave HBM between extraction and matching.
//
//   k_area_grid    one workgroup per frame: every key point gets the key (cell << 14 | index); a rank sort in LDS (keys are
//                  unique, n <= 16383: the 3 x nFeatures extractor of the initialisation included) lists the indices cell-major with
//                  ascending index inside a cell -- the order the
//                  reference's per-cell vectors have -- and a start offset is written for each of the 5 x 50 x 50 cells.
//   k_area_query   eight lanes per query: cms_area_rects() (the reference's 41 unfolding cases as a table, cms_area_table.h)
//                  yields up to three cell rectangles; the lanes take their cell columns in turn and keep AddCells' order (ix outer,
//                  iy inner, level and canvas-distance test).  The ONLY search of nearly every query: it leaves the query's count, its
//                  first CMS_AREA_TMP candidates (final values, in output order) and one sum of counts per workgroup.
//   k_area_lists   one workgroup per tile of CMS_AREA_TILE queries: the tile's first offset from the partial sums in front of it, a
//                  scan of the tile's counts in LDS -> CSR offsets and total, then the tile's lists: copied from the first-hits buffer,
//                  or, for the rare query with more than CMS_AREA_TMP candidates, searched again (cms_area_search in fill mode).
//                  Index arithmetic: cms_area_offsets.h.  Two launches per query call, ordered by the stream alone.
// The CSR lists feed k_hamming_best2 directly; candidate order (which decides Hamming ties) equals the reference's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cms_types.h"
#include "cms_area_table.h"
#include "cms_area_offsets.h"

#define CMS_AREA_CELLS (5 * CMS_AREA_G * CMS_AREA_G)
#define CMS_AREA_MAXKP 16383

extern "C" __global__ void __launch_bounds__(1024)
k_area_grid(const CmsKeyPoint* __restrict__ kps, const int* __restrict__ kp_cnt, int kp_cap, int F, float inv,
            uint16_t* __restrict__ sorted_idx, int* __restrict__ cell_start, int* __restrict__ n_valid_out) {
  extern __shared__ uint32_t area_lds[];                 // keys [kp_cap + 1] | sorted [kp_cap + 1]
  uint32_t* keys = area_lds;
  uint32_t* sorted = area_lds + (kp_cap + 1);
  __shared__ int s_nvalid;
  const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const int n = min(kp_cnt[b], min(kp_cap, CMS_AREA_MAXKP));      // the LDS arrays hold kp_cap + 1 entries each
  const CmsKeyPoint* kp = kps + (size_t)b * kp_cap;
  if (tid == 0) s_nvalid = 0;
  __syncthreads();
  for (int i = tid; i < n; i += T) {
    const float x = kp[i].x, y = kp[i].y;
    const double fi = (double)(x / (float)F), fj = (double)(y / (float)F);     // FaceInCubemap(cv::Point2f) (CamModelGeneral.h:445-456)
    int f = -1;
    if (fi >= 0 && fi < 1 && fj >= 1 && fj < 2) f = 1;
    else if (fi >= 1 && fi < 2 && fj >= 0 && fj < 1) f = 3;
    else if (fi >= 1 && fi < 2 && fj >= 1 && fj < 2) f = 0;
    else if (fi >= 1 && fi < 2 && fj >= 2 && fj < 3) f = 4;
    else if (fi >= 2 && fi < 3 && fj >= 1 && fj < 2) f = 2;
    uint32_t key = 0xFFFFC000u | (uint32_t)i;                                   // not on a face: sorted behind every cell
    if (f >= 0) {
      const int px = (int)(x * inv) % CMS_AREA_G, py = (int)(y * inv) % CMS_AREA_G;     // PosInGrid (Frame.cpp:734-742), mnMinX = 0
      key = ((uint32_t)((f * CMS_AREA_G + px) * CMS_AREA_G + py) << 14) | (uint32_t)i;
      atomicAdd(&s_nvalid, 1);
    }
    keys[i] = key;
  }
  __syncthreads();
  for (int i = tid; i < n; i += T) {
    const uint32_t k = keys[i];
    int r = 0;
    for (int q = 0; q < n; ++q) r += keys[q] < k ? 1 : 0;
    sorted[r] = k;
  }
  __syncthreads();
  const int nv = s_nvalid;
  uint16_t* si = sorted_idx + (size_t)b * kp_cap;
  int* cs = cell_start + (size_t)b * (CMS_AREA_CELLS + 1);
  for (int s = tid; s < nv; s += T) {
    const int c = (int)(sorted[s] >> 14), prev = s ? (int)(sorted[s - 1] >> 14) : -1;
    si[s] = (uint16_t)(sorted[s] & 0x3FFFu);
    for (int cc = prev + 1; cc <= c; ++cc) cs[cc] = s;
  }
  const int last = nv ? (int)(sorted[nv - 1] >> 14) : -1;
  for (int cc = last + 1 + tid; cc <= CMS_AREA_CELLS; cc += T) cs[cc] = nv;
  if (tid == 0) n_valid_out[b] = nv;
}

struct CmsAreaArgs {
  const CmsKeyPoint* kp;        // the frame's key points
  const uint16_t* sorted_idx;   // cell-major index list of the frame
  const int* cell_start;        // CMS_AREA_CELLS + 1 offsets into sorted_idx
  const float* qx; const float* qy; const float* qr; const int* qmin; const int* qmax;
  const int* q_frame;           // optional: frame of the batch a query addresses (nullptr: all queries address `kp`'s frame)
  int kp_cap;                   // frame stride of kp / sorted_idx (cell_start: CMS_AREA_CELLS + 1) when q_frame is given
  int nq, F; float inv;
  int* cnt;                     // candidates per query (written for every query; 0 for a "no window" query)
  int* off;                     // CSR offsets (nq + 1)
  int* idx; int cap; int idx_base;
  int* tmp;                     // nq x CMS_AREA_TMP: the search leaves the first hits of every query here (final values, in order); the list
                                // kernel only copies them for the queries that have no more than that (nearly all: ~2 candidates per window)
  int* psum;                    // one sum of counts per search workgroup (plain stores: nothing to clear between calls)
};
#define CMS_AREA_TMP 8

__device__ __forceinline__ int cms_area_pick(int k, int v0, int v1, int v2) { return k == 0 ? v0 : (k == 1 ? v1 : v2); }      // (values, not addresses)

// The search of one query by the eight lanes `gl` = 0..7 of its group (eight queries per wavefront): the lanes take the cell columns
// ix of a rectangle in turn, so the dependent loads of a query (cell offsets -> index list -> key point) run eight wide; a group-wide
// prefix sum of the per-column hit counts keeps the output in AddCells' order (ix outer, iy inner, index order inside a cell).
// FILL = false: the first CMS_AREA_TMP hits go to a.tmp.  FILL = true: all hits go to a.idx[base ..], in front of a.cap only.
// Returns the number of hits (the same in all lanes of the group; 0 for !in and for r < 0).  ALL 64 lanes of a wavefront call it
// together (loop bounds are made wavefront-uniform by shuffles); idle groups pass in = false.
template <bool FILL>
__device__ __forceinline__ int cms_area_search(const CmsAreaArgs& a, int qq, bool in, int gl, int base) {
  const float x = a.qx[qq], y = a.qy[qq], r = a.qr[qq];
  const bool live = in && !(r < 0.0f);                    // r < 0: "no window" (a map point outside the frustum), empty list
  const int minLevel = a.qmin[qq], maxLevel = a.qmax[qq];
  const bool check = (minLevel > 0) || (maxLevel >= 0);
  CmsAreaRectI rc[3] = {};                                 // written and read with constant indices only: registers, not scratch
  const int nr = live ? cms_area_rects(x, y, r, a.F, a.inv, rc) : 0;
  int n = 0;                                               // hits of the whole query so far (same in all lanes of the group)
  int* tmpq = a.tmp + (size_t)qq * CMS_AREA_TMP;
  const int fr = a.q_frame ? a.q_frame[qq] : 0;
  const CmsKeyPoint* kp = a.kp + (size_t)fr * a.kp_cap;
  const uint16_t* sorted_idx = a.sorted_idx + (size_t)fr * a.kp_cap;
  const int* cell_start = a.cell_start + (size_t)fr * (CMS_AREA_CELLS + 1);
  const int idx_base = a.idx_base + (a.q_frame ? fr * a.kp_cap : 0);
  // the groups of a wavefront walk different rectangle shapes: loop bounds are made group-uniform via shuffles inside the group
  for (int k = 0; k < 3; ++k) {
    const bool has = k < nr;
    const int x0 = has ? max(0, cms_area_pick(k, rc[0].x0, rc[1].x0, rc[2].x0)) : 0, x1 = has ? min(CMS_AREA_G - 1, cms_area_pick(k, rc[0].x1, rc[1].x1, rc[2].x1)) : -1;
    const int y0 = has ? max(0, cms_area_pick(k, rc[0].y0, rc[1].y0, rc[2].y0)) : 0, y1 = has ? min(CMS_AREA_G - 1, cms_area_pick(k, rc[0].y1, rc[1].y1, rc[2].y1)) : -1;        // AddCells' clamp
    const int face = has ? cms_area_pick(k, rc[0].face, rc[1].face, rc[2].face) : 0;
    const int ncol = (x1 >= x0 && y1 >= y0) ? x1 - x0 + 1 : 0;
    // every group of the wave iterates max-over-wave column chunks; idle groups just carry zeros through the shuffles
    int maxcol = ncol;
    for (int o = 32; o > 0; o >>= 1) maxcol = max(maxcol, __shfl_xor(maxcol, o));
    for (int cb = 0; cb < maxcol; cb += CMS_AREA_QL) {
      const int ix = x0 + cb + gl;
      const bool col = cb + gl < ncol;
      int s0 = 0, s1 = 0;
      if (col) {
        const int c0 = (face * CMS_AREA_G + ix) * CMS_AREA_G + y0;      // cells (ix, y0 .. y1) are consecutive in the list
        s0 = cell_start[c0]; s1 = cell_start[c0 + (y1 - y0) + 1];
      }
      // this lane's hits in its column; the first four are kept (a column rarely holds more)
      int h0 = 0, h1 = 0, h2 = 0, h3 = 0;                  // registers, not an indexed array (that would live in scratch)
      int nh = 0;
      for (int s = s0; s < s1; ++s) {
        const int j = sorted_idx[s];
        const CmsKeyPoint p = kp[j];
        if (check) {
          if (p.octave < minLevel) continue;
          if (maxLevel >= 0 && p.octave > maxLevel) continue;
        }
        if (fabsf(p.x - x) < r && fabsf(p.y - y) < r) {
          if (nh == 0) h0 = j; else if (nh == 1) h1 = j; else if (nh == 2) h2 = j; else if (nh == 3) h3 = j;
          ++nh;
        }
      }
      // exclusive prefix of nh over the 8 lanes of the group
      int incl = nh;
#pragma unroll
      for (int o = 1; o < CMS_AREA_QL; o <<= 1) { const int t = __shfl_up(incl, o, CMS_AREA_QL); if (gl >= o) incl += t; }
      const int tot = __shfl(incl, CMS_AREA_QL - 1, CMS_AREA_QL);
      if (!FILL && nh > 0) {                                // the first CMS_AREA_TMP hits of the query, already in output order
        int w = n + incl - nh;
        if (w < CMS_AREA_TMP) {
          if (nh <= 4) {
            tmpq[w] = idx_base + h0;
            if (nh > 1 && w + 1 < CMS_AREA_TMP) tmpq[w + 1] = idx_base + h1;
            if (nh > 2 && w + 2 < CMS_AREA_TMP) tmpq[w + 2] = idx_base + h2;
            if (nh > 3 && w + 3 < CMS_AREA_TMP) tmpq[w + 3] = idx_base + h3;
          } else {
            for (int s = s0; s < s1 && w < CMS_AREA_TMP; ++s) {
              const int j = sorted_idx[s];
              const CmsKeyPoint p = kp[j];
              if (check && (p.octave < minLevel || (maxLevel >= 0 && p.octave > maxLevel))) continue;
              if (fabsf(p.x - x) < r && fabsf(p.y - y) < r) { tmpq[w] = idx_base + j; ++w; }
            }
          }
        }
      }
      if (FILL && nh > 0) {
        int w = base + n + incl - nh;
        if (nh <= 4) {
          if (cms_area_fits(w, a.cap)) a.idx[w] = idx_base + h0;
          if (nh > 1 && cms_area_fits(w + 1, a.cap)) a.idx[w + 1] = idx_base + h1;
          if (nh > 2 && cms_area_fits(w + 2, a.cap)) a.idx[w + 2] = idx_base + h2;
          if (nh > 3 && cms_area_fits(w + 3, a.cap)) a.idx[w + 3] = idx_base + h3;
        } else {                                            // crowded column: walk it again instead of a bigger local list
          for (int s = s0; s < s1; ++s) {
            const int j = sorted_idx[s];
            const CmsKeyPoint p = kp[j];
            if (check && (p.octave < minLevel || (maxLevel >= 0 && p.octave > maxLevel))) continue;
            if (fabsf(p.x - x) < r && fabsf(p.y - y) < r) { if (cms_area_fits(w, a.cap)) a.idx[w] = idx_base + j; ++w; }
          }
        }
      }
      n += tot;
    }
  }
  return n;
}

// Launch 1: count + first hits of every query, and the sum of the workgroup's counts in psum[blockIdx.x].
extern "C" __global__ void __launch_bounds__(CMS_AREA_QT) k_area_query(CmsAreaArgs a) {
  __shared__ int part[CMS_AREA_QT / 64];
  const int gl = threadIdx.x & (CMS_AREA_QL - 1);
  const int q = (blockIdx.x * CMS_AREA_QT + threadIdx.x) / CMS_AREA_QL;
  const bool in = q < a.nq;
  const int n = cms_area_search<false>(a, in ? q : 0, in, gl, 0);
  if (in && gl == 0) a.cnt[q] = n;                            // 0 for a "no window" query
  int v = n;                                                  // the same in the 8 lanes of a group: these three steps add the 8 groups
  for (int o = CMS_AREA_QL; o < 64; o <<= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) { int t = 0; for (int w = 0; w < CMS_AREA_QT / 64; ++w) t += part[w]; a.psum[blockIdx.x] = t; }
}

// Launch 2: CSR offsets (off[0] = 0, off[q + 1] = sum cnt[0..q], *total = off[nq]) and the lists of one tile of queries.
extern "C" __global__ void __launch_bounds__(CMS_AREA_LT) k_area_lists(CmsAreaArgs a, int* __restrict__ total) {
  __shared__ int s_cnt[CMS_AREA_TILE], s_off[CMS_AREA_TILE];
  __shared__ int part[CMS_AREA_TILE_K * CMS_AREA_LW], pbefore[CMS_AREA_LW];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int tile = blockIdx.x, q0 = tile * CMS_AREA_TILE;
  // the counts in front of the tile: whole partial sums of launch 1
  int before = 0;
  {
    const int4* p4 = (const int4*)a.psum;
    const int n4 = cms_area_parts_before(tile) / 4;
    for (int b = tid; b < n4; b += CMS_AREA_LT) { const int4 v = p4[b]; before += (v.x + v.y) + (v.z + v.w); }
  }
  for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o);
  if (lane == 0) pbefore[wv] = before;
  int c[CMS_AREA_TILE_K], incl[CMS_AREA_TILE_K];
#pragma unroll
  for (int k = 0; k < CMS_AREA_TILE_K; ++k) {
    const int q = q0 + cms_area_tile_slot(tid, k);
    c[k] = q < a.nq ? a.cnt[q] : 0;
    int s = c[k];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(s, o); if (lane >= o) s += t; }
    incl[k] = s;
    if (lane == 63) part[k * CMS_AREA_LW + wv] = s;
  }
  __syncthreads();
  int tile_base = 0;
  for (int w = 0; w < CMS_AREA_LW; ++w) tile_base += pbefore[w];
#pragma unroll
  for (int k = 0; k < CMS_AREA_TILE_K; ++k) {
    const int ql = cms_area_tile_slot(tid, k), q = q0 + ql;
    const int mine = tile_base + cms_area_handover(part, k, wv) + incl[k];
    s_cnt[ql] = c[k]; s_off[ql] = mine - c[k];
    if (q < a.nq) a.off[q + 1] = mine;
    if (q == a.nq - 1 && total) *total = mine;
  }
  if (tile == 0 && tid == 0) a.off[0] = 0;
  __syncthreads();
  // the lists: eight lanes per query again, CMS_AREA_LG queries of the tile at a time.  First the copies (nearly every query): the first-hits
  // rows of four rounds are loaded before any is stored, so four loads are in flight per lane (a row is read whole; only its first cnt
  // entries were written by launch 1 and only those are stored)
  const int gl = tid & (CMS_AREA_QL - 1), g = tid / CMS_AREA_QL;
  const int nt = min(CMS_AREA_TILE, a.nq - q0);
  for (int t0 = 0; t0 < nt; t0 += 4 * CMS_AREA_LG) {
    int v[4], w[4]; bool ok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int ql = t0 + u * CMS_AREA_LG + g;
      const bool in = ql < nt;
      const int cq = in ? s_cnt[ql] : 0;
      w[u] = (in ? s_off[ql] : 0) + gl;
      ok[u] = cq <= CMS_AREA_TMP && gl < cq && cms_area_fits(w[u], a.cap);
      v[u] = a.tmp[(size_t)(in ? q0 + ql : q0) * CMS_AREA_TMP + gl];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) if (ok[u]) a.idx[w[u]] = v[u];
  }
  // then the few queries with more candidates than the first-hits buffer keeps: searched again, in fill mode
  for (int t0 = 0; t0 < nt; t0 += CMS_AREA_LG) {
    const int ql = t0 + g;
    const bool big = ql < nt && s_cnt[ql] > CMS_AREA_TMP;
    if (__ballot(big)) cms_area_search<true>(a, big ? q0 + ql : q0, big, gl, big ? s_off[ql] : 0);      // (wavefront-uniform branch: all 64 lanes search, the others idle)
  }
}
