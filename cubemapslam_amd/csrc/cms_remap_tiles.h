// cms_remap_tiles.h -- the 2-D tile table of k_remap_t*: plain host code, no HIP (a CPU test calls it through the C-ABI).
//
// The canvas is cut into tiles of tile_w x tile_h = 1024 pixels, one workgroup each.  On the side faces a canvas ROW maps to an arc
// through the fisheye image, a compact canvas TILE to a compact patch of it: per tile the table holds the source rectangle that covers
// every tap (X .. X + 1, Y .. Y + 1) of the tile's written LUT entries, which the kernel stages in LDS.
//
// Cells the reference never writes keep the LUT entry 0 (cms_build_lut; System.cpp:316-317): cv::remap then reads source pixel (0, 0) with
// weight 1.  They are 26 % of the Lafida cross and 46 % of the front camera's and would stretch every such tile's rectangle to the image
// origin, so they are left out of the rectangles; the kernel gives them the frame's pixel (0, 0), read once per frame.  (A WRITTEN entry
// can only be 0 when it maps to pixel (0, 0) with zero fractions: the same value.)
#ifndef CMS_REMAP_TILES_H
#define CMS_REMAP_TILES_H
#include <stdint.h>
#include <vector>
#include "../../include/cubemapslam_hip.h"

#define CMS_RT_PIXELS 1024         /* pixels per tile: 256 threads x 4 */
#define CMS_RT_DIRECT 1            /* flags: rectangle above the LDS budget, the tile gathers from global memory */
#define CMS_RT_DEAD 2              /* flags: every pixel lies in the corner blocks of the cross (kept at 0) */
#define CMS_RT_FRAMES 4            /* frames staged side by side (== CMS_REMAP_FPT): LDS bytes of a tile = 4 * CMS_RT_FRAMES * nd * rows */
#define CMS_RT_LDS_MAX 32768       /* LDS budget of a workgroup: 8 KB per frame (front camera, F = 650, 64 x 16: at most 5.2 KB) */

static inline bool cms_rt_shape_ok(int tile_w, int tile_h) {
  return (tile_w == 32 || tile_w == 64 || tile_w == 128) && tile_w * tile_h == CMS_RT_PIXELS;
}

// Live tiles first (row-major), then the dead ones (only a launch that rewrites the corner blocks walks those).  *lds_bytes = the largest
// staged tile (at least 64: a tile without written entries still addresses its first bytes).
static inline void cms_rt_build(int F, const uint32_t* lut, int lut_stride, int tile_w, int tile_h, int lds_budget,
                                std::vector<cms_remap_tile>& out, int* n_live, int* lds_bytes) {
  const int W = 3 * F, ntx = (W + tile_w - 1) / tile_w, nty = (W + tile_h - 1) / tile_h;
  std::vector<cms_remap_tile> dead;
  out.clear();
  int lds = 64;
  for (int ty = 0; ty < nty; ++ty)
    for (int tx = 0; tx < ntx; ++tx) {
      int xlo = 1 << 30, xhi = -1, ylo = 1 << 30, yhi = -1;
      bool any = false;
      for (int y = ty * tile_h; y < (ty + 1) * tile_h && y < W; ++y) {
        const bool mid_row = y >= F && y < 2 * F;
        for (int x = tx * tile_w; x < (tx + 1) * tile_w && x < W; ++x) {
          if (!mid_row && (x < F || x >= 2 * F)) continue;
          any = true;
          const uint32_t e = lut[(size_t)y * lut_stride + x];
          if (e == 0) continue;
          const int X = e & 0x7FF, Y = (e >> 11) & 0x7FF;
          if (X < xlo) xlo = X;
          if (X + 1 > xhi) xhi = X + 1;
          if (Y < ylo) ylo = Y;
          if (Y + 1 > yhi) yhi = Y + 1;
        }
      }
      cms_remap_tile t;
      t.tx = (uint16_t)tx; t.ty = (uint16_t)ty; t.x0 = t.y0 = t.nd = t.rows = t.flags = t.pad = 0;
      if (!any) { t.flags = CMS_RT_DEAD; dead.push_back(t); continue; }
      if (xhi >= 0) {
        t.x0 = (uint16_t)(xlo & ~3); t.y0 = (uint16_t)ylo;
        t.nd = (uint16_t)((xhi - t.x0) / 4 + 1); t.rows = (uint16_t)(yhi - ylo + 1);
        const int bytes = 4 * CMS_RT_FRAMES * t.nd * t.rows;
        if (bytes > lds_budget) t.flags = CMS_RT_DIRECT;
        else if (bytes > lds) lds = bytes;
      }
      out.push_back(t);
    }
  *n_live = (int)out.size();
  out.insert(out.end(), dead.begin(), dead.end());
  *lds_bytes = lds;
}
#endif
