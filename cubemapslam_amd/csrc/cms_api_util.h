// cms_api_util.h -- host-side helpers shared by the cms_api_*.hip files; included by cms_api_frames.hip behind cms_ctx, cms_fail and HIPCHK.
#pragma once
#include <cmath>
#include <functional>
#include <mutex>
#include <string>

static inline size_t cms_align(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }
// Offsets of the pieces of one scratch / staging block.  Every piece starts on a 256-byte boundary; `pad` bytes behind a piece belong to it
// (kernels read whole uint4 rows, offset lists have one entry more than items: a caller's padding is part of its layout).
struct CmsBlock {
  size_t size = 0;
  size_t take(size_t bytes, size_t pad = 0) { const size_t at = size; size += cms_align(bytes + pad); return at; }
};
// The HIP side of CmsStage (cms_stage.h): pinned blocks with hipHostMalloc's default flags (non-coherent: fast copies).
struct CmsHipMem {
  static int take(void** p, size_t bytes, bool pinned) { HIPCHK(pinned ? hipHostMalloc(p, bytes) : hipMalloc(p, bytes)); return CMS_OK; }
  static int give(void* p, bool pinned) { HIPCHK(pinned ? hipHostFree(p) : hipFree(p)); return CMS_OK; }
  static int wait(void* stream) { HIPCHK(hipStreamSynchronize((hipStream_t)stream)); return CMS_OK; }
  static int copy(void* dst, const void* src, size_t bytes, bool to_device, void* stream) {
    HIPCHK(hipMemcpyAsync(dst, src, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, (hipStream_t)stream));
    return CMS_OK;
  }
  static int range_error(const char* who) { return cms_fail(CMS_ERR_HIP, (std::string(who) + ": a staged copy reaches beyond its block").c_str()); }
};
// a `create` entry's device test; `what` is the entry's own message
static int cms_check_device(int device, const char* what) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device < 0 || device >= ndev) return cms_fail(CMS_ERR_NO_DEVICE, what);
  return CMS_OK;
}
// 16-entry per-level table of a kernel's argument struct: src[l] for the context's levels, `pad` behind them
static inline void cms_level_table(float* dst, const cms_ctx* c, const float* src, float pad) {
  for (int l = 0; l < 16; ++l) dst[l] = l < c->g.nlevels ? src[l] : pad;
}
static inline float cms_cos_fov(const cms_ctx* c) {      // CamModelGeneral::SetCosFovTh (CamModelGeneral.h:224-229), float
  const float fov = (float)c->cam.fov_deg;
  const float pif = 3.1415926535897932384626f;
  return std::cos(fov / 2 * (pif / 180));
}
static inline float cms_log_scale(const cms_ctx* c) {      // mfLogScaleFactor = log(mfScaleFactor), float (Frame.cpp:113)
  return std::log(c->g.nlevels > 1 ? c->scale[1] : 1.2f);
}
// a result array in pinned (device-visible) host memory: the last kernel of a call may store there itself
static inline bool cms_is_pinned(const void* ptr) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, ptr) == hipSuccess) return at.type == hipMemoryTypeHost;
  (void)hipGetLastError();                                         // (a pageable pointer: not an error, just the copy)
  return false;
}
static inline float cms_grid_inv(const cms_ctx* c) { return (float)(3 * CMS_AREA_G) / (float)c->g.W; }      // mfGridElementLengthInv (Frame.cpp:149)

// Raise a kernel's dynamic-LDS ceiling above the 64 KB default.  The attribute is per function AND per device: `done` is the kernel's own
// flag per device (a static of the caller); every launcher of the kernel calls this.
static int cms_lds_ceiling_once(const void* kernel, int bytes, int device, bool (&done)[64]) {
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  if (device >= 0 && device < 64 && !done[device]) { HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes)); done[device] = true; }
  return CMS_OK;
}

// Where the map points of a search entry come from when not from the caller's host arrays: the hook fills pos | normal | min_dist | max_dist | desc
// of the call's points on the device, in the order of stream s (cms_api_mappoints.hip: rows of a cms_mpstore named by id).  The launch chain behind
// it is the host-array entry's.
using CmsPointGather = std::function<int(hipStream_t s, float* pos, float* normal, float* min_dist, float* max_dist, uint8_t* desc)>;

// The window-query entries guess a candidate capacity (64 per window) and repeat ONCE with the exact size when the device counted more.
// attempt(cap, total) is one whole attempt: reserve (CmsStage::reserve may reallocate: block pointers are taken after that), stage the
// caller's arrays (in/out ones afresh), launch, synchronise, leave the device's candidate total in `total`, and deliver the results only if
// total <= cap (the list kernel never writes beyond cap, and the searches do nothing on lists that were cut).
template <class Attempt>
static int cms_retry_capacity(int cap, const char* entry, Attempt&& attempt) {
  for (int i = 0; i < 2; ++i) {
    int total = 0;
    const int rc = attempt(cap, total);
    if (rc || total <= cap) return rc;
    cap = total + 64;
  }
  return cms_fail(CMS_ERR_OVERFLOW, (std::string(entry) + ": candidate lists kept growing").c_str());
}
