// Host replay of the window query's offset arithmetic (cubemapslam_amd/csrc/cms_area_offsets.h): launch 1's partial sums (one per search
// workgroup) and launch 2's per-tile work -- the partial sums in front of the tile, the wavefront scans with their hand-over, and the
// capacity guard on every list position -- thread by thread in the layout the kernel uses, so the arithmetic can be checked against a
// cumulative sum without a GPU.
#define CMS_AREA_HOST_EMU
#include "../../cubemapslam_amd/csrc/cms_area_offsets.h"
#include <stddef.h>
#include <vector>

extern "C" void area_offsets_consts(int* out) {
  out[0] = CMS_AREA_WG_Q; out[1] = CMS_AREA_TILE; out[2] = CMS_AREA_LT; out[3] = CMS_AREA_TILE_K; out[4] = CMS_AREA_TILE_PARTS;
}

// cnt[nq] -> off[nq + 1]; written[nwritten]: how often the list position w was stored to (positions at or beyond cap must stay 0).
// Returns *total as the kernel would leave it (-1: never written).
extern "C" int area_offsets_emu(int nq, const int* cnt, int* off, int cap, unsigned char* written, int nwritten) {
  // launch 1: one plain store per search workgroup
  std::vector<int> psum((size_t)cms_area_search_grid(nq), -12345);
  for (int wg = 0; wg < cms_area_search_grid(nq); ++wg) {
    int t = 0;
    for (int i = 0; i < CMS_AREA_WG_Q; ++i) { const int q = wg * CMS_AREA_WG_Q + i; if (q < nq) t += cnt[q]; }
    psum[(size_t)wg] = t;
  }
  // launch 2: tiles in an arbitrary order (here: last first) -- no tile may depend on another tile's results
  int total = -1;
  for (int tile = cms_area_tile_grid(nq) - 1; tile >= 0; --tile) {
    const int q0 = tile * CMS_AREA_TILE;
    int before = 0;
    if (cms_area_parts_before(tile) > (int)psum.size() || cms_area_parts_before(tile) % 4) return -2;      // read as int4, inside the array
    for (int b = 0; b < cms_area_parts_before(tile); ++b) before += psum[(size_t)b];
    int part[CMS_AREA_TILE_K * CMS_AREA_LW];
    std::vector<int> incl((size_t)CMS_AREA_TILE), c((size_t)CMS_AREA_TILE);
    for (int k = 0; k < CMS_AREA_TILE_K; ++k)
      for (int wv = 0; wv < CMS_AREA_LW; ++wv) {
        int s = 0;                                              // inclusive scan over the 64 lanes of the wavefront
        for (int lane = 0; lane < 64; ++lane) {
          const int tid = wv * 64 + lane, ql = cms_area_tile_slot(tid, k), q = q0 + ql;
          c[(size_t)ql] = q < nq ? cnt[q] : 0;
          s += c[(size_t)ql];
          incl[(size_t)ql] = s;
        }
        part[k * CMS_AREA_LW + wv] = s;
      }
    for (int tid = 0; tid < CMS_AREA_LT; ++tid)
      for (int k = 0; k < CMS_AREA_TILE_K; ++k) {
        const int ql = cms_area_tile_slot(tid, k), q = q0 + ql;
        const int mine = before + cms_area_handover(part, k, tid / 64) + incl[(size_t)ql];
        if (q < nq) off[q + 1] = mine;
        if (q == nq - 1) total = mine;
        const int cq = c[(size_t)ql], base = mine - cq;
        for (int j = 0; j < cq; ++j)
          if (cms_area_fits(base + j, cap)) { if (base + j < 0 || base + j >= nwritten) return -3; ++written[base + j]; }
      }
    if (tile == 0) off[0] = 0;
  }
  return total;
}
