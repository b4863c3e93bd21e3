// cms_cubemap_project.h -- CamModelGeneral::TransformRaysToCubemap, one source for the gfx950 kernels, the host side of the C-ABI and the
// host build of the PnP core (cms_pnp_core.h).  Compiles under hipcc and under g++ as it stands.
#ifndef CMS_CUBEMAP_PROJECT_H
#define CMS_CUBEMAP_PROJECT_H
#include "cms_detmath.h"      // CMS_HD

// CamModelGeneral::TransformRaysToCubemap (src/CamModelGeneral.cpp:95-154): face choice on float ratios, pixel through the double
// intrinsics (fx = fy = cx = cy = F / 2 are double members, so `_x * fx / _z + cx` is evaluated in double and narrowed on assignment)
CMS_HD int track_rays_to_cubemap(int F, float x, float y, float z, float& up, float& vp) {
  const double f = F / 2.0;
  float lx, ly, lz, ox, oy;
  int face;
  if (z > 0 && x / z <= 1 && x / z >= -1 && y / z <= 1 && y / z >= -1) { face = 0; lx = x; ly = y; lz = z; ox = (float)F; oy = (float)F; }
  else if (x > 0 && y / x <= 1 && y / x >= -1 && z / x <= 1 && z / x >= -1) { face = 2; lx = -z; ly = y; lz = x; ox = (float)(2 * F); oy = (float)F; }
  else if (x < 0 && y / (-x) <= 1 && y / (-x) >= -1 && z / (-x) <= 1 && z / (-x) >= -1) { face = 1; lx = z; ly = y; lz = -x; ox = 0.0f; oy = (float)F; }
  else if (y > 0 && x / y <= 1 && x / y >= -1 && z / y <= 1 && z / y >= -1) { face = 4; lx = x; ly = -z; lz = y; ox = (float)F; oy = (float)(2 * F); }
  else if (y < 0 && x / (-y) <= 1 && x / (-y) >= -1 && z / (-y) <= 1 && z / (-y) >= -1) { face = 3; lx = x; ly = z; lz = -y; ox = (float)F; oy = 0.0f; }
  else { up = -1.0f; vp = -1.0f; return -1; }
  up = (float)((double)lx * f / (double)lz + f);
  vp = (float)((double)ly * f / (double)lz + f);
  if (up < 0 || up >= F || vp < 0 || vp >= F) return -1;
  if (ox != 0.0f) up += ox;          // the reference adds nothing on the first column / row of faces
  if (oy != 0.0f) vp += oy;
  return face;
}

#endif
