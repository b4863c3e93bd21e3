// cms_area_offsets.h -- the index arithmetic of the window query's second launch (k_area_lists, cms_area_kernels.hip): which partial
// sums lie in front of a tile of queries, how the tile-local scan of the counts is handed from wavefront to wavefront, and the guard
// against the capacity of the candidate array.  Plain integer code that compiles for the device and, with CMS_AREA_HOST_EMU, for the
// host (tests/emu/area_offsets_emu.cpp replays it against a cumulative sum without a GPU).
//
// Launch 1 (k_area_query) runs CMS_AREA_WG_Q queries per workgroup and stores the sum of their counts in psum[blockIdx.x].
// Launch 2 (k_area_lists) runs one workgroup of CMS_AREA_LT threads per tile of CMS_AREA_TILE consecutive queries:
//   slot      thread `tid` holds the queries  k * CMS_AREA_LT + tid  of the tile, k = 0 .. CMS_AREA_TILE_K - 1 ("chunk" k: CMS_AREA_LT
//             consecutive queries, one per thread, so a wavefront holds 64 consecutive queries of a chunk);
//   in front  tile t's first offset is the sum of psum[0 .. t * CMS_AREA_TILE / CMS_AREA_WG_Q);
//   scan      every wavefront scans its 64 counts of a chunk and leaves the total in part[k * CMS_AREA_LW + wave]; the offset of a
//             query = the tile's base + the parts of all (chunk, wave) pairs in front of its own + its wavefront's inclusive scan.
// No workgroup reads anything another workgroup of the same launch wrote.
#ifndef CMS_AREA_OFFSETS_H
#define CMS_AREA_OFFSETS_H

#ifdef CMS_AREA_HOST_EMU
#define AREA_OFF_FN inline
#else
#define AREA_OFF_FN __host__ __device__ __forceinline__
#endif

#define CMS_AREA_QL 8                                        /* lanes per query in the search */
#define CMS_AREA_QT 256                                      /* threads of a search workgroup */
#define CMS_AREA_WG_Q (CMS_AREA_QT / CMS_AREA_QL)            /* queries per search workgroup = per partial sum */
#define CMS_AREA_LT 256                                      /* threads of a list workgroup */
#define CMS_AREA_LW (CMS_AREA_LT / 64)                       /* its wavefronts */
#define CMS_AREA_LG (CMS_AREA_LT / CMS_AREA_QL)               /* queries whose lists it writes at a time */
#define CMS_AREA_TILE_K 4                                    /* queries per thread in the tile-local scan */
#define CMS_AREA_TILE (CMS_AREA_LT * CMS_AREA_TILE_K)        /* queries per tile */
#define CMS_AREA_TILE_PARTS (CMS_AREA_TILE / CMS_AREA_WG_Q)  /* partial sums per tile (a multiple of 4: read as int4) */

AREA_OFF_FN int cms_area_search_grid(int nq) { return (nq + CMS_AREA_WG_Q - 1) / CMS_AREA_WG_Q; }     // = number of partial sums
AREA_OFF_FN int cms_area_tile_grid(int nq) { return (nq + CMS_AREA_TILE - 1) / CMS_AREA_TILE; }
// number of partial sums in front of tile t (tiles start on a search-workgroup boundary, so none is split)
AREA_OFF_FN int cms_area_parts_before(int tile) { return tile * CMS_AREA_TILE_PARTS; }
// position inside the tile of the query thread `tid` holds in chunk k
AREA_OFF_FN int cms_area_tile_slot(int tid, int k) { return k * CMS_AREA_LT + tid; }
// hand-over between wavefronts: the sum of the wavefront totals in front of (chunk k, wavefront wv)
AREA_OFF_FN int cms_area_handover(const int* part, int k, int wv) {
  int s = 0;
  for (int i = 0; i < k * CMS_AREA_LW + wv; ++i) s += part[i];
  return s;
}
// a candidate is stored only in front of the array's capacity (the offsets and the total do not depend on it)
AREA_OFF_FN bool cms_area_fits(int w, int cap) { return w < cap; }

#endif
