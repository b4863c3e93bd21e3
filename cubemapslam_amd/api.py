"""ctypes binding of libcubemapslam_hip.so (the C-ABI in include/cubemapslam_hip.h).

Plumbing only: every call goes straight to the hand-written HIP library.  There is NO CPU fallback: if the shared
library is missing or no MI355X is visible the calls raise.
"""
import time
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CMS_HIP_LIB") or os.path.join(_HERE, "lib", "libcubemapslam_hip.so")   # override: developer A/B builds (tools/ab_build.sh)


class CmsError(RuntimeError):
    pass


class Camera(C.Structure):
    _fields_ = [("c", C.c_double), ("d", C.c_double), ("e", C.c_double), ("u0", C.c_double), ("v0", C.c_double),
                ("invpol", C.c_double * 12), ("pol", C.c_double * 5), ("Iw", C.c_int), ("Ih", C.c_int),
                ("face", C.c_int), ("fov_deg", C.c_double)]


class OrbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int), ("scale_factor", C.c_float), ("nlevels", C.c_int),
                ("ini_th_fast", C.c_int), ("min_th_fast", C.c_int)]


class Geometry(C.Structure):
    _fields_ = [("W", C.c_int), ("F", C.c_int), ("nlevels", C.c_int), ("kp_cap", C.c_int), ("max_batch", C.c_int),
                ("level_w", C.c_int * 12), ("level_h", C.c_int * 12), ("level_quota", C.c_int * 12),
                ("level_cells", C.c_int * 12), ("scale", C.c_float * 12), ("inv_scale", C.c_float * 12),
                ("sigma2", C.c_float * 12), ("inv_sigma2", C.c_float * 12), ("pyramid_bytes_per_frame", C.c_size_t),
                ("candidate_entries_per_frame", C.c_size_t), ("fisheye_stride", C.c_int)]


class BaStats(C.Structure):
    _fields_ = [("iterations_done", C.c_int * 2), ("chi2_initial", C.c_double * 2), ("chi2_final", C.c_double * 2),
                ("lambda_final", C.c_double * 2), ("n_outliers_mid", C.c_int), ("n_outliers_final", C.c_int)]


KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4")])

_lib = None


def lib():
    """Load the HIP library; raises if it has not been built (python -m cubemapslam_amd.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CmsError("libcubemapslam_hip.so is missing -- build it with `python -m cubemapslam_amd.build` "
                           "(there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        L.cms_last_error.restype = C.c_char_p
        for n in ("cms_ctx_stream", "cms_frames_input", "cms_ba_stream"):
            getattr(L, n).restype = C.c_void_p
            getattr(L, n).argtypes = [C.c_void_p]
        L.cms_ctx_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.cms_ctx_destroy.argtypes = [C.c_void_p]
        L.cms_ctx_destroy.restype = None
        L.cms_ctx_geometry.argtypes = [C.c_void_p, C.c_void_p]
        L.cms_remap.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.cms_set_mask.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.cms_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.cms_remap_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.cms_frames_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_int]
        L.cms_frames_upload_async.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_int]
        L.cms_frames_upload_wait.argtypes = [C.c_void_p]
        L.cms_frames_upload_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.cms_frames_process_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.cms_host_alloc.argtypes = [C.c_void_p, C.c_size_t]
        L.cms_host_free.argtypes = [C.c_void_p]
        L.cms_host_free.restype = None
        L.cms_ba_profile_kernel.argtypes = [C.c_void_p, C.c_int]
        L.cms_ba_profile_get.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.cms_ba_debug_compose.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cms_frames_process.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.cms_frames_sync.argtypes = [C.c_void_p]
        L.cms_frames_results.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cms_frames_fetch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.cms_debug_lut.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.cms_debug_cubemap.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.cms_debug_level.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.cms_debug_candidates.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.cms_debug_distributed.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.cms_profile_enable.argtypes = [C.c_void_p, C.c_int]
        L.cms_profile_get.argtypes = [C.c_void_p, C.c_void_p]
        L.cms_hamming_best2.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 9
        L.cms_hamming_best2_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 10
        L.cms_hamming_matrix.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.cms_ba_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double,
                                    C.c_double, C.c_double]
        L.cms_ba_reset.argtypes = [C.c_void_p]
        L.cms_ba_optimize.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.cms_ba_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cms_ba_destroy.argtypes = [C.c_void_p]
        L.cms_ba_destroy.restype = None
        L.cms_ba_run.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double,
                                 C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cms_ba_linearize.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double,
                                       C.c_double, C.c_int, C.c_double] + [C.c_void_p] * 7
        L.cms_area_set_keypoints.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.cms_area_grid.argtypes = [C.c_void_p, C.c_int]
        L.cms_features_in_area.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_int, C.c_void_p]
        L.cms_features_in_area_device.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 8 + [C.c_int, C.c_int, C.c_void_p]
        L.cms_features_in_area_batch_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 9 + [C.c_int, C.c_void_p]
        L.cms_area_set_descriptors.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.cms_search_local_points.argtypes = ([C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_float] * 3 + [C.c_int, C.c_int] +
                                              [C.c_void_p] * 9)
        L.cms_search_local_points_ids.argtypes = ([C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p] + [C.c_float] * 3 + [C.c_int, C.c_int] +
                                                  [C.c_void_p] * 9)
        L.cms_kfstore_fuse_search_sets_ids.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_float, C.c_void_p, C.c_void_p]
        L.cms_search_by_projection.argtypes = ([C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_float, C.c_int, C.c_int, C.c_int] +
                                               [C.c_void_p] * 3)
        L.cms_project_last_frame_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_float] + [C.c_void_p] * 5
        L.cms_rotation_filter_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int]
        L.cms_is_in_frustum_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_float, C.c_float] + [C.c_void_p] * 8
        L.cms_search_local_points_device.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_float, C.c_int] + [C.c_void_p] * 3
        L.cms_create_new_map_points.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
        L.cms_kfstore_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.cms_kfstore_destroy.argtypes = [C.c_void_p]
        L.cms_kfstore_destroy.restype = None
        L.cms_kfstore_put.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.cms_kfstore_update.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
        L.cms_kfstore_fuse_search.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8 + [C.c_float, C.c_void_p, C.c_void_p]
        L.cms_kfstore_fuse_search_sets.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 3 + [C.c_float, C.c_void_p, C.c_void_p]
        L.cms_kfstore_put_from_frame.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
        L.cms_kfstore_update_poses.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
        L.cms_kfstore_debug_fetch.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 12
        L.cms_ba_debug_fetch_plan.argtypes = [C.c_void_p] * 14
        L.cms_kfstore_create_new_map_points.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5
        L.cms_distinctive_descriptors.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cms_update_normal_and_depth.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8
        L.cms_fuse_search.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_float, C.c_void_p, C.c_void_p]
        L.cms_pose_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.cms_pose_destroy.argtypes = [C.c_void_p]
        L.cms_pose_destroy.restype = None
        L.cms_pose_stream.argtypes = [C.c_void_p]
        L.cms_pose_stream.restype = C.c_void_p
        _edge = [C.c_void_p] * 5 + [C.c_double] * 4
        L.cms_pose_upload.argtypes = [C.c_void_p, C.c_int] + _edge + [C.c_void_p]
        L.cms_pose_launch.argtypes = [C.c_void_p]
        L.cms_pose_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.cms_pose_optimize_batch.argtypes = [C.c_void_p, C.c_int] + _edge + [C.c_void_p] * 4
        L.cms_pose_optimize.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_double] * 4 + [C.c_void_p] * 4
        _lib = L
    return _lib


def _p(a):
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    return a.ctypes.data_as(C.c_void_p)


def _chk(rc, what):
    if rc < 0:
        raise CmsError("%s failed (%d): %s" % (what, rc, lib().cms_last_error().decode()))
    return rc


class _Handle:
    """Life cycle of a handle of the library: _create fills self.h through the class's create entry, close() hands it to the destroy entry once,
    and __del__ swallows whatever a close at interpreter exit raises"""
    _entries = None      # (create, destroy)

    def _create(self, *args, out_last=False):
        self.h = C.c_void_p()
        args = args + (C.byref(self.h),) if out_last else (C.byref(self.h),) + args
        _chk(getattr(lib(), self._entries[0])(*args), self._entries[0])

    def close(self):
        if getattr(self, "h", None):
            getattr(lib(), self._entries[1])(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def make_camera(d):
    cam = Camera()
    for k in ("c", "d", "e", "u0", "v0", "Iw", "Ih", "face", "fov_deg"):
        setattr(cam, k, d[k])
    for i in range(12):
        cam.invpol[i] = d["invpol"][i] if i < len(d["invpol"]) else 0.0
    for i in range(5):
        cam.pol[i] = d["pol"][i] if i < len(d["pol"]) else 0.0
    return cam


RT_DTYPE = np.dtype([(n, "<u2") for n in ("tx", "ty", "x0", "y0", "nd", "rows", "flags", "pad")])   # cms_remap_tile
RT_LDS_MAX = 32768      # CMS_RT_LDS_MAX: the LDS budget cms_ctx_create builds the table with


def remap_lut_host(cam):
    """cms_remap_lut_host: the packed remap LUT [3F][3F] u32, built on the host (no device)"""
    cam = make_camera(cam) if isinstance(cam, dict) else cam
    W = 3 * cam.face
    out = np.zeros((W, (W + 3) // 4 * 4), np.uint32)
    f = lib().cms_remap_lut_host
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    _chk(f(C.byref(cam), _p(out), out.shape[1]), "cms_remap_lut_host")
    return out[:, :W]


def remap_tiles_host(cam, lut, tile_w, tile_h, lds_budget=RT_LDS_MAX):
    """cms_remap_tiles_host: (tiles as RT_DTYPE records, n_live, lds_bytes) of the remap's tile table, built on the host"""
    cam = make_camera(cam) if isinstance(cam, dict) else cam
    lut = np.ascontiguousarray(lut, np.uint32)
    W = 3 * cam.face
    cap = ((W + tile_w - 1) // tile_w) * ((W + tile_h - 1) // tile_h)
    out = np.zeros(cap, RT_DTYPE)
    n_live, n_all, lds = C.c_int(), C.c_int(), C.c_int()
    f = lib().cms_remap_tiles_host
    f.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_int] + [C.c_void_p] * 3
    _chk(f(C.byref(cam), _p(lut), lut.strides[0] // 4, tile_w, tile_h, lds_budget, _p(out), cap, C.byref(n_live), C.byref(n_all), C.byref(lds)),
         "cms_remap_tiles_host")
    return out[:n_all.value].copy(), n_live.value, lds.value


def fast_cells_host(cam, which, nfeatures=2000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7):
    """cms_fast_cells_host: the FAST work list `which` (0 every cell, 1 without the zero corners, 2 the remapped batch's) as (level, row, column)
    int arrays in the kernel's order, built on the host (no device)"""
    cam = make_camera(cam) if isinstance(cam, dict) else cam
    orb = OrbParams(nfeatures, scale_factor, nlevels, ini_th, min_th)
    f = lib().cms_fast_cells_host
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    n = C.c_int()
    _chk(f(C.byref(cam), C.byref(orb), which, None, 0, C.byref(n)), "cms_fast_cells_host")
    out = np.zeros(max(n.value, 1), np.int32)
    _chk(f(C.byref(cam), C.byref(orb), which, _p(out), len(out), C.byref(n)), "cms_fast_cells_host")
    out = out[:n.value]
    return out & 15, (out >> 4) & 255, (out >> 12) & 255


class Context(_Handle):
    """cms_ctx: remap LUT + extractor tables + device buffers for up to max_batch frames."""
    _entries = ("cms_ctx_create", "cms_ctx_destroy")

    def __init__(self, cam, nfeatures=2000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7, max_batch=1, device=0):
        self.cam = make_camera(cam) if isinstance(cam, dict) else cam
        self.orb = OrbParams(nfeatures, scale_factor, nlevels, ini_th, min_th)
        self._create(device, C.byref(self.cam), C.byref(self.orb), max_batch)
        self.geom = Geometry()
        _chk(lib().cms_ctx_geometry(self.h, C.byref(self.geom)), "cms_ctx_geometry")
        self.W = self.geom.W
        self.max_batch = max_batch

    @property
    def stream(self):
        return lib().cms_ctx_stream(self.h)

    def set_mask(self, mask):
        mask = np.ascontiguousarray(mask, np.uint8)
        _chk(lib().cms_set_mask(self.h, _p(mask), mask.strides[0]), "cms_set_mask")

    def set_distance_bounds_mode(self, scaled):
        f = lib().cms_set_distance_bounds_mode
        f.argtypes = [C.c_void_p, C.c_int]
        _chk(f(self.h, int(scaled)), "cms_set_distance_bounds_mode")

    def set_gaussian_mode(self, column_mode):
        f = lib().cms_set_gaussian_mode
        f.argtypes = [C.c_void_p, C.c_int]
        _chk(f(self.h, int(column_mode)), "cms_set_gaussian_mode")

    def remap(self, fisheye, cubemap=None):
        fisheye = np.ascontiguousarray(fisheye, np.uint8)
        if cubemap is None:
            cubemap = np.zeros((self.W, self.W), np.uint8)
        _chk(lib().cms_remap(self.h, _p(fisheye), fisheye.strides[0], _p(cubemap), cubemap.strides[0]), "cms_remap")
        return cubemap

    def extract(self, cubemap, cap=None):
        cubemap = np.ascontiguousarray(cubemap, np.uint8)
        cap = cap or self.geom.kp_cap
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int()
        _chk(lib().cms_extract(self.h, _p(cubemap), cubemap.strides[0], _p(kps), _p(desc), cap, C.byref(n)), "cms_extract")
        return kps[:n.value].copy(), desc[:n.value].copy()

    def remap_extract(self, fisheye, cap=None):
        fisheye = np.ascontiguousarray(fisheye, np.uint8)
        cap = cap or self.geom.kp_cap
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int()
        _chk(lib().cms_remap_extract(self.h, _p(fisheye), fisheye.strides[0], _p(kps), _p(desc), cap, C.byref(n)), "cms_remap_extract")
        return kps[:n.value].copy(), desc[:n.value].copy()

    def remap_extract_rays(self, fisheye, cap=None):
        """cms_remap_extract_rays: key points, descriptors and Frame::mvKeyRays (n x 3 float) of one frame, one synchronisation"""
        fisheye = np.ascontiguousarray(fisheye, np.uint8)
        cap = cap or self.geom.kp_cap
        kps = np.zeros(cap, KP_DTYPE); desc = np.zeros((cap, 32), np.uint8); rays = np.zeros((cap, 3), np.float32)
        n = C.c_int()
        _chk(lib().cms_remap_extract_rays(self.h, _p(fisheye), fisheye.strides[0], _p(kps), _p(desc), _p(rays), cap, C.byref(n)), "cms_remap_extract_rays")
        return kps[:n.value].copy(), desc[:n.value].copy(), rays[:n.value].copy()

    def fetch_rays(self, b):
        """cms_frames_fetch_rays: mvKeyRays of frame b of the last process() call"""
        cap = self.geom.kp_cap
        rays = np.zeros((cap, 3), np.float32)
        n = C.c_int()
        _chk(lib().cms_frames_fetch_rays(self.h, b, _p(rays), cap, C.byref(n)), "cms_frames_fetch_rays")
        return rays[:n.value].copy()

    def rays_ptr(self):
        a = C.c_void_p()
        _chk(lib().cms_frames_rays(self.h, C.byref(a)), "cms_frames_rays")
        return a.value

    # ---- batched device path
    def upload(self, frames):
        frames = np.ascontiguousarray(frames, np.uint8)
        assert frames.ndim == 3
        _chk(lib().cms_frames_upload(self.h, _p(frames), frames.strides[1], frames.strides[0], frames.shape[0]), "cms_frames_upload")

    def upload_async(self, frames):
        """input streaming: `frames` must live in pinned memory (host_alloc); the copy runs on the context's copy stream and the next
        process() waits for it on the device"""
        assert frames.ndim == 3 and frames.dtype == np.uint8 and frames.flags.c_contiguous
        _chk(lib().cms_frames_upload_async(self.h, _p(frames), frames.strides[1], frames.strides[0], frames.shape[0]), "cms_frames_upload_async")

    def upload_device(self, d_ptr, B):
        """staging <- device buffer [B][Ih][fisheye_stride] (inputs resident in HBM), asynchronous on the ctx stream"""
        _chk(lib().cms_frames_upload_device(self.h, C.c_void_p(int(d_ptr)), B), "cms_frames_upload_device")

    def process_device(self, d_ptr, B):
        """process(B) on a device buffer [B][Ih][fisheye_stride] read in place (no staging copy); the caller keeps it untouched until sync()"""
        _chk(lib().cms_frames_process_device(self.h, C.c_void_p(int(d_ptr)), B), "cms_frames_process_device")

    def stream_wait_extracted(self, hip_stream):
        """the given HIP stream waits (on the device) for the extraction of this context's last process() call"""
        f = lib().cms_stream_wait_extracted
        f.argtypes = [C.c_void_p, C.c_void_p]
        _chk(f(self.h, C.c_void_p(int(hip_stream))), "cms_stream_wait_extracted")

    def upload_wait(self):
        _chk(lib().cms_frames_upload_wait(self.h), "cms_frames_upload_wait")

    def process(self, B, from_fisheye=True):
        _chk(lib().cms_frames_process(self.h, B, 1 if from_fisheye else 0), "cms_frames_process")

    def sync(self):
        _chk(lib().cms_frames_sync(self.h), "cms_frames_sync")

    def fetch(self, b):
        cap = self.geom.kp_cap
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int()
        _chk(lib().cms_frames_fetch(self.h, b, _p(kps), _p(desc), cap, C.byref(n)), "cms_frames_fetch")
        return kps[:n.value].copy(), desc[:n.value].copy()

    def results_ptrs(self):
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _chk(lib().cms_frames_results(self.h, C.byref(a), C.byref(b), C.byref(c)), "cms_frames_results")
        return a.value, b.value, c.value

    def input_ptr(self):
        return lib().cms_frames_input(self.h)

    def profile(self, on=True):
        lib().cms_profile_enable(self.h, 1 if on else 0)

    def profile_ms(self):
        ms = np.zeros(7, np.float32)
        _chk(lib().cms_profile_get(self.h, _p(ms)), "cms_profile_get")
        return dict(zip(("remap", "pyramid", "fast", "octree", "cull", "describe", "total"), ms.tolist()))

    # ---- debug read-back
    def debug_lut(self):
        W = self.W
        out = np.zeros((W, (W + 3) // 4 * 4), np.uint32)
        s = C.c_int()
        _chk(lib().cms_debug_lut(self.h, _p(out), C.byref(s)), "cms_debug_lut")
        return out[:, :W]

    def debug_level(self, b, l):
        w, h = self.geom.level_w[l], self.geom.level_h[l]
        out = np.zeros((h, w), np.uint8)
        _chk(lib().cms_debug_level(self.h, b, l, _p(out), w), "cms_debug_level")
        return out

    def debug_candidates(self, b, l):
        cap = self.geom.level_w[l] * self.geom.level_h[l] // 4 + 4096
        out = np.zeros((cap, 3), np.int32)
        n = C.c_int()
        _chk(lib().cms_debug_candidates(self.h, b, l, _p(out), cap, C.byref(n)), "cms_debug_candidates")
        return out[:n.value].copy()

    def debug_distributed(self, b, l):
        cap = self.geom.level_quota[l] + 8
        out = np.zeros((cap, 3), np.int32)
        n = C.c_int()
        _chk(lib().cms_debug_distributed(self.h, b, l, _p(out), cap, C.byref(n)), "cms_debug_distributed")
        return out[:n.value].copy()

    # ---- matching
    def hamming_best2(self, qdesc, tdesc, cand_off, cand_idx, tlevel=None, texcl=None):
        qdesc = np.ascontiguousarray(qdesc, np.uint8); tdesc = np.ascontiguousarray(tdesc, np.uint8)
        cand_off = np.ascontiguousarray(cand_off, np.int32); cand_idx = np.ascontiguousarray(cand_idx, np.int32)
        tl = np.ascontiguousarray(tlevel, np.int32) if tlevel is not None else None
        tx = np.ascontiguousarray(texcl, np.uint8) if texcl is not None else None
        nq = len(qdesc)
        outs = [np.zeros(max(nq, 1), np.int32) for _ in range(5)]
        _chk(lib().cms_hamming_best2(self.h, _p(qdesc), nq, _p(tdesc), len(tdesc), _p(cand_off), _p(cand_idx), _p(tl), _p(tx),
                                     *[_p(o) for o in outs]), "cms_hamming_best2")
        keys = ("best_idx", "best_dist", "best_level", "second_dist", "second_level")
        return {k: o[:nq] for k, o in zip(keys, outs)}

    def area_set_keypoints(self, b, kps):
        """put caller key points into frame slot b (tests / callers that extracted elsewhere)"""
        kps = np.ascontiguousarray(kps, KP_DTYPE)
        _chk(lib().cms_area_set_keypoints(self.h, b, len(kps), _p(kps)), "cms_area_set_keypoints")

    def area_grid(self, B):
        """Frame::AssignFeaturesToGrid for frames 0..B-1 (device-resident key points)"""
        _chk(lib().cms_area_grid(self.h, B), "cms_area_grid")

    def features_in_area(self, b, qx, qy, qr, qmin, qmax, cap=None):
        """Frame::GetFeaturesInArea for a batch of queries against frame b -> (off[nq+1], idx[total]) in the reference's order"""
        qx = np.ascontiguousarray(qx, np.float32); qy = np.ascontiguousarray(qy, np.float32); qr = np.ascontiguousarray(qr, np.float32)
        qmin = np.ascontiguousarray(qmin, np.int32); qmax = np.ascontiguousarray(qmax, np.int32)
        nq = len(qx)
        cap = cap or max(1, 64 * nq + 1024)
        off = np.zeros(nq + 1, np.int32); idx = np.zeros(cap, np.int32); tot = C.c_int(0)
        _chk(lib().cms_features_in_area(self.h, b, nq, _p(qx), _p(qy), _p(qr), _p(qmin), _p(qmax), _p(off), _p(idx), cap, C.byref(tot)),
             "cms_features_in_area")
        return off, idx[:tot.value]

    def features_in_area_device(self, b, nq, d_q5, d_cnt, d_off, d_idx, cap, idx_base, d_total):
        """device-pointer variant: d_q5 = (qx, qy, qr, qmin, qmax) device addresses"""
        _chk(lib().cms_features_in_area_device(self.h, b, nq, *[C.c_void_p(int(a)) for a in d_q5], C.c_void_p(int(d_cnt)), C.c_void_p(int(d_off)),
                                               C.c_void_p(int(d_idx)), cap, idx_base, C.c_void_p(int(d_total))), "cms_features_in_area_device")

    def features_in_area_batch_device(self, nq, d_qframe, d_q5, d_cnt, d_off, d_idx, cap, d_total):
        """all frames of the batch in one launch sequence; d_qframe[q] = frame searched by query q; indices are batch rows"""
        _chk(lib().cms_features_in_area_batch_device(self.h, nq, C.c_void_p(int(d_qframe)), *[C.c_void_p(int(a)) for a in d_q5], C.c_void_p(int(d_cnt)),
                                                     C.c_void_p(int(d_off)), C.c_void_p(int(d_idx)), cap, C.c_void_p(int(d_total))),
             "cms_features_in_area_batch_device")

    def area_set_descriptors(self, b, desc):
        desc = np.ascontiguousarray(desc, np.uint8)
        _chk(lib().cms_area_set_descriptors(self.h, b, len(desc), _p(desc)), "cms_area_set_descriptors")

    def search_local_points(self, b, pose15, pos, normal, min_dist, max_dist, mp_desc, kp_mp, viewing_cos_limit=0.5, th=1.0, nnratio=0.8,
                            th_high=100):
        """Frame::isInFrustum + ORBMatcher::SearchByProjection(F, vpMapPoints, th) for frame b (area_grid first).  kp_mp: int32 per key
        point (>= 0 = taken), updated in place.  Returns dict(in_view, proj_x, proj_y, level, view_cos, match, n_matches, rounds)."""
        pose15 = np.ascontiguousarray(pose15, np.float32).reshape(15)
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3); normal = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
        n = len(pos)
        min_dist = np.ascontiguousarray(min_dist, np.float32); max_dist = np.ascontiguousarray(max_dist, np.float32)
        mp_desc = np.ascontiguousarray(mp_desc, np.uint8).reshape(n, 32)
        assert kp_mp.dtype == np.int32 and kp_mp.flags.c_contiguous
        vis = np.zeros(n, np.uint8); px = np.zeros(n, np.float32); py = np.zeros(n, np.float32); lvl = np.zeros(n, np.int32)
        vc = np.zeros(n, np.float32); match = np.full(n, -1, np.int32)
        nm = C.c_int(0); rounds = C.c_int(0)
        _chk(lib().cms_search_local_points(self.h, b, _p(pose15), n, _p(pos), _p(normal), _p(min_dist), _p(max_dist), _p(mp_desc),
                                           viewing_cos_limit, th, nnratio, th_high, len(kp_mp), _p(kp_mp), _p(vis), _p(px), _p(py), _p(lvl),
                                           _p(vc), _p(match), C.addressof(nm), C.addressof(rounds)), "cms_search_local_points")
        return dict(in_view=vis, proj_x=px, proj_y=py, level=lvl, view_cos=vc, match=match, n_matches=nm.value, rounds=rounds.value)

    def search_local_points_ids(self, b, pose15, mpstore, ids, kp_mp, viewing_cos_limit=0.5, th=1.0, nnratio=0.8, th_high=100):
        """cms_search_local_points_ids: search_local_points with the map points named by id in a MapPointStore; same dict"""
        pose15 = np.ascontiguousarray(pose15, np.float32).reshape(15)
        ids = _ids32(ids)
        n = len(ids)
        assert kp_mp.dtype == np.int32 and kp_mp.flags.c_contiguous
        vis = np.zeros(n, np.uint8); px = np.zeros(n, np.float32); py = np.zeros(n, np.float32); lvl = np.zeros(n, np.int32)
        vc = np.zeros(n, np.float32); match = np.full(n, -1, np.int32)
        nm = C.c_int(0); rounds = C.c_int(0)
        _chk(lib().cms_search_local_points_ids(self.h, b, _p(pose15), mpstore.h, n, _p(ids) if n else None, viewing_cos_limit, th, nnratio, th_high, len(kp_mp), _p(kp_mp),
                                               _p(vis), _p(px), _p(py), _p(lvl), _p(vc), _p(match), C.addressof(nm), C.addressof(rounds)), "cms_search_local_points_ids")
        return dict(in_view=vis, proj_x=px, proj_y=py, level=lvl, view_cos=vc, match=match, n_matches=nm.value, rounds=rounds.value)

    def search_by_projection(self, b, pose12, valid, Xw, octave, angle, mp_desc, kp_mp, th=15.0, check_ori=True, th_high=100):
        """ORBMatcher::SearchByProjection(CurrentFrame, LastFrame, th, mono) against frame slot b -> (match, n_matches); kp_mp in/out"""
        a = [np.ascontiguousarray(pose12, np.float32), np.ascontiguousarray(valid, np.uint8), np.ascontiguousarray(Xw, np.float32),
             np.ascontiguousarray(octave, np.int32), np.ascontiguousarray(angle, np.float32), np.ascontiguousarray(mp_desc, np.uint8)]
        n = len(a[1])
        match = np.full(n, -1, np.int32); nm = C.c_int(0)
        assert kp_mp.dtype == np.int32
        _chk(lib().cms_search_by_projection(self.h, b, _p(a[0]), n, *[_p(v) for v in a[1:]], th, int(check_ori), th_high, len(kp_mp), _p(kp_mp), _p(match),
                                            C.addressof(nm)), "cms_search_by_projection")
        return match, nm.value

    def search_by_projection_keyframe(self, b, pose12, kf_angle, pos, min_dist, max_dist, mp_desc, kp_mp, th=10.0, orb_dist=100, check_ori=True):
        """ORBMatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) against frame slot b with a key frame that is not resident
        -> (match, n_matches).  One entry per listed map point (non-NULL, not bad, not in sAlreadyFound; key-frame order): kf_angle =
        pKF->mvKeys[i].angle, pos, min_dist, max_dist, mp_desc.  kp_mp int32 per frame key point (>= 0 = holds a map point), updated in place."""
        a = [np.ascontiguousarray(pose12, np.float32).reshape(12), np.ascontiguousarray(kf_angle, np.float32), np.ascontiguousarray(pos, np.float32).reshape(-1, 3),
             np.ascontiguousarray(min_dist, np.float32), np.ascontiguousarray(max_dist, np.float32), np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)]
        n = len(a[1])
        assert all(len(v) == n for v in a[2:])
        assert kp_mp.dtype == np.int32 and kp_mp.flags.c_contiguous
        match = np.full(max(n, 1), -1, np.int32); nm = C.c_int(0)
        L = lib()
        L.cms_search_by_projection_keyframe.argtypes = ([C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_float, C.c_int, C.c_int, C.c_int] +
                                                        [C.c_void_p] * 3)
        _chk(L.cms_search_by_projection_keyframe(self.h, b, _p(a[0]), n, *[_p(v) for v in a[1:]], float(th), int(orb_dist), int(check_ori), len(kp_mp), _p(kp_mp),
                                                 _p(match), C.addressof(nm)), "cms_search_by_projection_keyframe")
        return match[:n], nm.value

    def search_for_initialization(self, b2, k1, d1, prev_matched, window=100, nnratio=0.9, check_ori=True):
        """ORBMatcher::SearchForInitialization(F1, F2 = frame slot b2, vbPrevMatched, vnMatches12, windowSize) -> (matches12, nmatches); prev_matched
        (n1, 2) float32 is updated in place"""
        k1 = np.ascontiguousarray(k1, KP_DTYPE); d1 = np.ascontiguousarray(d1, np.uint8)
        assert prev_matched.dtype == np.float32 and prev_matched.flags.c_contiguous and prev_matched.shape == (len(k1), 2)
        m12 = np.full(max(len(k1), 1), -1, np.int32); nm = C.c_int(0)
        f = lib().cms_search_for_initialization
        f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
        _chk(f(self.h, b2, len(k1), _p(k1), _p(d1), _p(prev_matched), int(window), float(nnratio), int(check_ori), _p(m12), C.addressof(nm)),
             "cms_search_for_initialization")
        return m12[:len(k1)], nm.value

    def project_last_frame_device(self, n, d_qframe, d_pose12, d_valid, d_Xw, d_oct, th, d_q5):
        """d_q5 = (qx, qy, qr, qmin, qmax) raw device pointers"""
        v = lambda a: C.c_void_p(int(a)) if a else None
        _chk(lib().cms_project_last_frame_device(self.h, n, v(d_qframe), v(d_pose12), v(d_valid), v(d_Xw), v(d_oct), th, *[v(a) for a in d_q5]),
             "cms_project_last_frame_device")

    def rotation_filter_device(self, B, d_mp_off, d_last_angle, d_kp_mp, d_mp_match, d_n_matches, check_orientation=True):
        v = lambda a: C.c_void_p(int(a)) if a else None
        _chk(lib().cms_rotation_filter_device(self.h, B, v(d_mp_off), v(d_last_angle), v(d_kp_mp), v(d_mp_match), v(d_n_matches), int(check_orientation)),
             "cms_rotation_filter_device")

    def is_in_frustum_device(self, nmp, d_mp_frame, d_pose15, d_pos, d_normal, d_min, d_max, viewing_cos_limit, th, d_outs5, d_q3):
        """d_outs5 = (in_view u8, proj_x, proj_y, level, view_cos); d_q3 = (qr, qmin, qmax) or (0, 0, 0); raw device pointers"""
        v = lambda a: C.c_void_p(int(a)) if a else None
        _chk(lib().cms_is_in_frustum_device(self.h, nmp, v(d_mp_frame), v(d_pose15), v(d_pos), v(d_normal), v(d_min), v(d_max),
                                            viewing_cos_limit, th, *[v(a) for a in d_outs5], *[v(a) for a in d_q3]), "cms_is_in_frustum_device")

    def search_local_points_device(self, B, d_mp_off, d_mp_desc, d_cand_off, d_cand_idx, d_pair_dist, nnratio, th_high, d_kp_mp, d_mp_match,
                                   d_rounds=0):
        v = lambda a: C.c_void_p(int(a)) if a else None
        _chk(lib().cms_search_local_points_device(self.h, B, v(d_mp_off), v(d_mp_desc), v(d_cand_off), v(d_cand_idx), v(d_pair_dist), nnratio,
                                                  th_high, v(d_kp_mp), v(d_mp_match), v(d_rounds)), "cms_search_local_points_device")

    def hamming_best2_device(self, qdesc, q_row, nq, tdesc, cand_off, cand_idx, t_level, t_excl, outs):
        """all arguments are raw device pointers (ints); asynchronous on the ctx stream"""
        _chk(lib().cms_hamming_best2_device(self.h, _p(qdesc), _p(q_row), nq, _p(tdesc), _p(cand_off), _p(cand_idx), _p(t_level),
                                            _p(t_excl), *[_p(o) for o in outs]), "cms_hamming_best2_device")

    def hamming_matrix(self, a, b):
        a = np.ascontiguousarray(a, np.uint8); b = np.ascontiguousarray(b, np.uint8)
        out = np.zeros((len(a), len(b)), np.uint16)
        _chk(lib().cms_hamming_matrix(self.h, _p(a), len(a), _p(b), len(b), _p(out)), "cms_hamming_matrix")
        return out


    def compute_bow(self, vocab, rows, n, levelsup=4):
        """cms_frames_compute_bow: Frame::ComputeBoW for rows `rows` (n[i] key points each) of the last batch in one launch sequence; the results stay
        resident per row (fetch_bow, KeyframeStore.search_by_bow_frames)."""
        rows = np.ascontiguousarray(rows, np.int32); n = np.ascontiguousarray(n, np.int32)
        assert len(rows) == len(n)
        L = lib()
        L.cms_frames_compute_bow.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _chk(L.cms_frames_compute_bow(self.h, vocab.h, int(levelsup), len(rows), _p(rows), _p(n)), "cms_frames_compute_bow")

    def fetch_bow(self, b):
        """cms_frames_fetch_bow: dict(word_id, word_val, node_id, node_off, node_feat) of row b (mBowVec and mFeatVec as arrays)"""
        L = lib()
        L.cms_frames_fetch_bow.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        nw, nn = C.c_int(), C.c_int()
        cap = self.geom.kp_cap
        o = _bow_arrays(cap, cap, cap)
        _chk(L.cms_frames_fetch_bow(self.h, b, C.byref(nw), _p(o["word_id"]), _p(o["word_val"]), len(o["word_id"]), C.byref(nn), _p(o["node_id"]), _p(o["node_off"]),
                                    _p(o["node_feat"]), len(o["node_id"]), cap), "cms_frames_fetch_bow")
        return _bow_trim(o, nw.value, nn.value)


class PinnedArray:
    """uint8 numpy array over pinned host memory from cms_host_alloc (freed with the object)"""

    def __init__(self, shape):
        n = int(np.prod(shape))
        self.p = C.c_void_p()
        _chk(lib().cms_host_alloc(C.byref(self.p), n), "cms_host_alloc")
        self.array = np.ctypeslib.as_array((C.c_uint8 * n).from_address(self.p.value)).reshape(shape)

    def close(self):
        if self.p:
            self.array = None
            lib().cms_host_free(self.p)
            self.p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Keyframe(C.Structure):
    """cms_keyframe (include/cubemapslam_hip.h)"""
    _fields_ = [("n", C.c_int), ("kps", C.c_void_p), ("desc", C.c_void_p), ("rays", C.c_void_p), ("mp", C.c_void_p),
                ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3),
                ("nnodes", C.c_int), ("node_id", C.c_void_p), ("node_off", C.c_void_p), ("node_feat", C.c_void_p), ("median_depth", C.c_float)]


def make_keyframe(kf):
    """kf: dict with x, y, octave, angle, desc, rays, mp, R, t, Ow, node_id, node_off, node_feat, median_depth (synth.keyframe_set entries
    plus 'rays').  Returns (Keyframe, keep-alive list)."""
    n = len(kf["x"])
    kps = np.zeros(n, KP_DTYPE); kps["x"] = kf["x"]; kps["y"] = kf["y"]; kps["octave"] = kf["octave"]; kps["angle"] = kf["angle"]
    keep = [kps, np.ascontiguousarray(kf["desc"], np.uint8), np.ascontiguousarray(kf["rays"], np.float32), np.ascontiguousarray(kf["mp"], np.int32),
            np.ascontiguousarray(kf["node_id"], np.int32), np.ascontiguousarray(kf["node_off"], np.int32), np.ascontiguousarray(kf["node_feat"], np.int32)]
    K = Keyframe()
    K.n = n; K.kps = keep[0].ctypes.data; K.desc = keep[1].ctypes.data; K.rays = keep[2].ctypes.data; K.mp = keep[3].ctypes.data
    K.Rcw[:] = [float(v) for v in np.asarray(kf["R"], np.float32).reshape(9)]
    K.tcw[:] = [float(v) for v in kf["t"]]; K.Ow[:] = [float(v) for v in kf["Ow"]]
    K.nnodes = len(keep[4]); K.node_id = keep[4].ctypes.data; K.node_off = keep[5].ctypes.data; K.node_feat = keep[6].ctypes.data
    K.median_depth = float(kf["median_depth"])
    return K, keep


def search_for_triangulation(ctx, K1, K2, E12=None, check_orientation=False):
    """cms_search_for_triangulation: ORBMatcher::SearchForTriangulation(pKF1, pKF2, E12, ...) alone.  K1, K2: Keyframe structs; E12 (9 floats,
    row major) or None = ComputeE12 of the two poses.  Returns (matches12 int32[n1], nmatches)."""
    m = np.full(max(K1.n, 1), -1, np.int32)
    n = C.c_int()
    e = None if E12 is None else np.ascontiguousarray(E12, np.float32)
    lib().cms_search_for_triangulation.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    _chk(lib().cms_search_for_triangulation(ctx.h, C.byref(K1), C.byref(K2), _p(e) if e is not None else None, int(check_orientation), _p(m), C.byref(n)),
         "cms_search_for_triangulation")
    return m[:K1.n].copy(), n.value


def create_new_map_points(ctx, jobs, check_orientation=False, cap=None):
    """jobs: list of (current Keyframe, [neighbour Keyframes in covisibility order]).  Returns per job (neigh, idx1, idx2, x3d)."""
    nj = len(jobs)
    cur = (Keyframe * max(nj, 1))(*[j[0] for j in jobs])
    flat = [k for j in jobs for k in j[1]]
    neigh = (Keyframe * max(len(flat), 1))(*flat)
    off = np.concatenate([[0], np.cumsum([len(j[1]) for j in jobs])]).astype(np.int32)
    cap = cap if cap is not None else max([j[0].n for j in jobs] + [1])
    n_new = np.zeros(max(nj, 1), np.int32)
    on = np.zeros((max(nj, 1), cap), np.int32); o1 = np.zeros_like(on); o2 = np.zeros_like(on); ox = np.zeros((max(nj, 1), cap, 3), np.float32)
    _chk(lib().cms_create_new_map_points(ctx.h, nj, C.addressof(cur), _p(off), C.addressof(neigh), int(check_orientation), cap, _p(n_new), _p(on), _p(o1),
                                         _p(o2), _p(ox)), "cms_create_new_map_points")
    return [(on[j, :n_new[j]].copy(), o1[j, :n_new[j]].copy(), o2[j, :n_new[j]].copy(), ox[j, :n_new[j]].copy()) for j in range(nj)]


class BowJob(C.Structure):
    """cms_bow_job (include/cubemapslam_hip.h)"""
    _fields_ = [("slot", C.c_int), ("b", C.c_int), ("n", C.c_int), ("nnodes", C.c_int), ("node_id", C.c_void_p), ("node_off", C.c_void_p),
                ("node_feat", C.c_void_p), ("kf_skip", C.c_void_p)]


class BowKfJob(C.Structure):
    """cms_bow_kf_job (include/cubemapslam_hip.h)"""
    _fields_ = [("slot1", C.c_int), ("n1", C.c_int), ("slot2", C.c_int), ("n2", C.c_int), ("skip1", C.c_void_p), ("skip2", C.c_void_p)]


class Sim3SearchJob(C.Structure):
    """cms_sim3_search_job (include/cubemapslam_hip.h)"""
    _fields_ = [("slot1", C.c_int), ("n1", C.c_int), ("slot2", C.c_int), ("n2", C.c_int), ("s12", C.c_float), ("R12", C.c_float * 9), ("t12", C.c_float * 3),
                ("off1", C.c_int), ("off2", C.c_int)]


class Sim3ProjJob(C.Structure):
    """cms_sim3_proj_job (include/cubemapslam_hip.h)"""
    _fields_ = [("slot", C.c_int), ("n", C.c_int), ("Scw", C.c_float * 12), ("set", C.c_int)]


class KfProjJob(C.Structure):
    """cms_kfproj_job (include/cubemapslam_hip.h)"""
    _fields_ = [("slot", C.c_int), ("b", C.c_int), ("n", C.c_int), ("pose12", C.c_float * 12), ("nmp", C.c_int), ("kf_feat", C.c_void_p), ("pos", C.c_void_p),
                ("min_dist", C.c_void_p), ("max_dist", C.c_void_p), ("mp_desc", C.c_void_p), ("kp_mp", C.c_void_p), ("match", C.c_void_p)]


class KfdbJob(C.Structure):
    """cms_kfdb_job (include/cubemapslam_hip.h)"""
    _fields_ = [("mode", C.c_int), ("group", C.c_int), ("query", C.c_int), ("b", C.c_int), ("slot", C.c_int), ("nwords", C.c_int), ("word_id", C.c_void_p),
                ("word_val", C.c_void_p), ("min_score", C.c_float), ("n_connected", C.c_int), ("connected", C.c_void_p)]


KFDB_RELOC, KFDB_LOOP = 0, 1
KFDB_QUERY = {"row": 0, "slot": 1, "words": 2}


def kfdb_jobs(jobs):
    """cms_kfdb_job records from dicts: mode (KFDB_RELOC / KFDB_LOOP), group, query = ("row", b) | ("slot", s) | ("words", ids, vals), and for
    KFDB_LOOP min_score and connected (slots).  Returns (array, the numpy arrays the records point into: keep them until the call has returned)."""
    arr = (KfdbJob * max(len(jobs), 1))()
    keep = []
    for q, j in zip(arr, jobs):
        form = j["query"]
        q.mode = int(j["mode"]); q.group = int(j.get("group", 0)); q.query = KFDB_QUERY[form[0]]
        if form[0] == "row":
            q.b = int(form[1])
        elif form[0] == "slot":
            q.slot = int(form[1])
        else:
            ids = np.ascontiguousarray(form[1], np.int32); vals = np.ascontiguousarray(form[2], np.float64)
            assert len(ids) == len(vals)
            keep += [ids, vals]
            q.nwords = len(ids); q.word_id = ids.ctypes.data if len(ids) else None; q.word_val = vals.ctypes.data if len(ids) else None
        conn = np.ascontiguousarray(j.get("connected", ()), np.int32)
        keep.append(conn)
        q.min_score = float(j.get("min_score", 0.0)); q.n_connected = len(conn); q.connected = conn.ctypes.data if len(conn) else None
    return arr, keep


def kfdb_results(njobs, K, cap, cand, n_cand, common, score):
    """per job (candidate slots, common words int32[K], score bits uint32[K]) from the arrays of cms_kfdb_detect"""
    return [([int(c) for c in cand[j, :min(int(n_cand[j]), cap)]], common[j].copy(), score[j].view(np.uint32).copy()) for j in range(njobs)]


def _bow_fv(fv):
    """a FeatureVector as CSR int32 arrays: fv = dict(node_id, node_off, node_feat) or the tuple (node_id, node_off, node_feat)"""
    if isinstance(fv, dict):
        fv = (fv["node_id"], fv["node_off"], fv["node_feat"])
    nid, noff, nfeat = (np.ascontiguousarray(a, np.int32) for a in fv)
    if len(noff) == 0:
        noff = np.zeros(1, np.int32)
    return nid, noff, (nfeat if len(nfeat) else np.zeros(1, np.int32))


def search_by_bow(ctx, b, n, fv, K, skip=None, nnratio=0.7, check_orientation=True):
    """cms_search_by_bow: ORBMatcher::SearchByBoW(pKF, F, vpMapPointMatches) with the key frame K (a Keyframe struct, make_keyframe) from the host and
    the frame = row b of ctx's last batch (n key points) with FeatureVector fv (see _bow_fv).  skip: None or one byte per key-frame feature (!= 0:
    the map point is bad).  Returns (kf_idx int32[n]: key-frame feature whose map point frame key point i receives, or -1; n_matches)."""
    nid, noff, nfeat = _bow_fv(fv)
    sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
    kf_idx = np.full(max(n, 1), -1, np.int32)
    nm = C.c_int()
    L = lib()
    L.cms_search_by_bow.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int,
                                    C.c_void_p, C.c_void_p]
    _chk(L.cms_search_by_bow(ctx.h, b, n, len(nid), _p(nid), _p(noff), _p(nfeat), C.byref(K), _p(sk), float(nnratio), int(check_orientation), _p(kf_idx),
                             C.byref(nm)), "cms_search_by_bow")
    return kf_idx[:n].copy(), nm.value


def _bow_arrays(nw, nn, nf):
    return dict(word_id=np.zeros(nw, np.int32), word_val=np.zeros(nw, np.float64), node_id=np.zeros(nn, np.int32), node_off=np.zeros(nn + 1, np.int32),
                node_feat=np.zeros(max(nf, 1), np.int32))


def _bow_trim(o, nw, nn):
    noff = o["node_off"][:nn + 1].copy()
    return dict(word_id=o["word_id"][:nw].copy(), word_val=o["word_val"][:nw].copy(), node_id=o["node_id"][:nn].copy(), node_off=noff,
                node_feat=o["node_feat"][:int(noff[nn])].copy())


def load_vocabulary_text(path):
    """ORBvoc.txt's format (DBoW2 loadFromTextFile) -> dict(k, L, scoring, weighting, parent, is_leaf, desc, weight) with node 0 = the root.  Empty
    lines are skipped; the tree's shape is checked by Vocabulary / cms_vocab_create."""
    with open(path, "r") as f:
        lines = [ln for ln in f.read().split("\n")]
    if not lines or not lines[0].split():
        raise CmsError("vocabulary text: empty file")
    hdr = [int(v) for v in lines[0].split()]
    if len(hdr) < 4:
        raise CmsError("vocabulary text: not a correct text file (header)")
    rows = [ln.split() for ln in lines[1:] if ln.strip()]
    for i, r in enumerate(rows):
        if len(r) < 35:
            raise CmsError("vocabulary text: line %d ends early" % (i + 2))
    n = len(rows) + 1
    parent = np.zeros(n, np.int32); is_leaf = np.zeros(n, np.uint8); desc = np.zeros((n, 32), np.uint8); weight = np.zeros(n, np.float64)
    if rows:
        parent[1:] = [int(r[0]) for r in rows]; is_leaf[1:] = [1 if int(r[1]) > 0 else 0 for r in rows]
        desc[1:] = np.array([[int(v) & 255 for v in r[2:34]] for r in rows], np.uint8); weight[1:] = [float(r[34]) for r in rows]
    return dict(k=hdr[0], L=hdr[1], scoring=hdr[2], weighting=hdr[3], parent=parent, is_leaf=is_leaf, desc=desc, weight=weight)


class Vocabulary(_Handle):
    """cms_vocab: the DBoW2 vocabulary tree on one device (read-only, shared by any number of contexts and stores of that device).  Arrays as the text
    format holds them: node 0 is the root, parent[i] < i, is_leaf marks the words, desc n_nodes x 32 bytes, weight float64."""
    _entries = ("cms_vocab_create", "cms_vocab_destroy")

    def __init__(self, k, L, scoring, weighting, parent, is_leaf, desc, weight, device=0):
        parent = np.ascontiguousarray(parent, np.int32); is_leaf = np.ascontiguousarray(is_leaf, np.uint8)
        desc = np.ascontiguousarray(desc, np.uint8); weight = np.ascontiguousarray(weight, np.float64)
        assert len(is_leaf) == len(parent) and len(weight) == len(parent) and desc.size == 32 * len(parent)
        L_ = lib()
        L_.cms_vocab_create.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 4
        L_.cms_vocab_destroy.argtypes = [C.c_void_p]
        L_.cms_vocab_destroy.restype = None
        L_.cms_vocab_info.argtypes = [C.c_void_p, C.c_void_p]
        L_.cms_vocab_transform.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 7
        self._create(device, int(k), int(L), int(scoring), int(weighting), len(parent), _p(parent), _p(is_leaf), _p(desc), _p(weight))

    @classmethod
    def from_dict(cls, t, device=0):
        return cls(t["k"], t["L"], t["scoring"], t["weighting"], t["parent"], t["is_leaf"], t["desc"], t["weight"], device=device)

    @classmethod
    def from_text_file(cls, path, device=0):
        return cls.from_dict(load_vocabulary_text(path), device=device)

    def info(self):
        a = np.zeros(7, np.int32)
        _chk(lib().cms_vocab_info(self.h, _p(a)), "cms_vocab_info")
        return dict(zip(("k", "L", "scoring", "weighting", "nodes", "words", "device"), (int(v) for v in a)))

    def transform(self, ctx, desc, levelsup=4):
        """cms_vocab_transform: descriptors from the host (n x 32 uint8) -> dict(word_id, word_val, node_id, node_off, node_feat)"""
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(desc)
        o = _bow_arrays(max(n, 1), max(n, 1), n)
        nw, nn = C.c_int(), C.c_int()
        _chk(lib().cms_vocab_transform(self.h, ctx.h, n, _p(desc) if n else None, int(levelsup), C.byref(nw), _p(o["word_id"]), _p(o["word_val"]), C.byref(nn),
                                       _p(o["node_id"]), _p(o["node_off"]), _p(o["node_feat"])), "cms_vocab_transform")
        return _bow_trim(o, nw.value, nn.value)


class KeyframeStore(_Handle):
    """cms_kfstore: key frames resident on the device in slots"""
    _entries = ("cms_kfstore_create", "cms_kfstore_destroy")

    def __init__(self, ctx, max_keyframes, max_features=2048, max_nodes=2048):
        self.ctx = ctx
        self.max_keyframes = int(max_keyframes)
        self._create(ctx.h, max_keyframes, max_features, max_nodes)

    def put(self, slot, K):
        _chk(lib().cms_kfstore_put(self.h, slot, C.byref(K)), "cms_kfstore_put")

    def update(self, slot, R=None, t=None, Ow=None, median_depth=None, mp=None):
        f = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)
        a = [f(R, np.float32), f(t, np.float32), f(Ow, np.float32), None if median_depth is None else np.array([median_depth], np.float32), f(mp, np.int32)]
        _chk(lib().cms_kfstore_update(self.h, slot, *[_p(v) for v in a]), "cms_kfstore_update")

    def put_from_frame(self, slot, src_ctx, b, n, kf):
        """cms_kfstore_put_from_frame: frame b of src_ctx's last batch (key points, descriptors, rays, grid: device to device) becomes the key frame in
        `slot`; kf supplies what the host holds: R, t, Ow, median_depth, mp (or None), node_id / node_off / node_feat.  Asynchronous."""
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        i32 = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)
        R, t, Ow = f32(np.asarray(kf["R"]).reshape(9)), f32(kf["t"]), f32(kf["Ow"])
        mp, nid, noff, nfeat = i32(kf.get("mp")), i32(kf["node_id"]), i32(kf["node_off"]), i32(kf["node_feat"])
        L = lib()
        _chk(L.cms_kfstore_put_from_frame(self.h, slot, src_ctx.h, b, n, _p(R), _p(t), _p(Ow), float(kf["median_depth"]), _p(mp), len(nid), _p(nid), _p(noff), _p(nfeat)),
             "cms_kfstore_put_from_frame")

    def put_from_frames(self, src_ctx, items):
        """cms_kfstore_put_from_frames: several key frames of src_ctx's last batch in ONE call (one kernel); items = [(slot, b, n, kf), ...] with kf as in
        put_from_frame.  All items are checked before anything is touched: on an error the store is unchanged."""
        class KfFromFrame(C.Structure):      # cms_kf_from_frame (include/cubemapslam_hip.h)
            _fields_ = [("slot", C.c_int), ("b", C.c_int), ("n", C.c_int), ("Rcw", C.c_void_p), ("tcw", C.c_void_p), ("Ow", C.c_void_p), ("median_depth", C.c_float),
                        ("mp", C.c_void_p), ("nnodes", C.c_int), ("node_id", C.c_void_p), ("node_off", C.c_void_p), ("node_feat", C.c_void_p)]
        arr = (KfFromFrame * len(items))()
        keep = []
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        i32 = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)
        ptr = lambda a: None if a is None else a.ctypes.data
        for q, (slot, b, n, kf) in zip(arr, items):
            R, t, Ow = f32(np.asarray(kf["R"]).reshape(9)), f32(kf["t"]), f32(kf["Ow"])
            mp, nid, noff, nfeat = i32(kf.get("mp")), i32(kf["node_id"]), i32(kf["node_off"]), i32(kf["node_feat"])
            keep.append((R, t, Ow, mp, nid, noff, nfeat))
            q.slot = slot; q.b = b; q.n = n; q.Rcw = ptr(R); q.tcw = ptr(t); q.Ow = ptr(Ow); q.median_depth = float(kf["median_depth"]); q.mp = ptr(mp)
            q.nnodes = len(nid); q.node_id = ptr(nid); q.node_off = ptr(noff); q.node_feat = ptr(nfeat)
        L = lib()
        L.cms_kfstore_put_from_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _chk(L.cms_kfstore_put_from_frames(self.h, src_ctx.h, len(items), arr), "cms_kfstore_put_from_frames")

    def debug_fetch(self, slot, max_features=16384, max_nodes=16384):
        """cms_kfstore_debug_fetch: the slot's device contents as a dict"""
        hdr = np.zeros(21, np.uint32); misc = np.zeros(2, np.int32)
        L = lib()
        _chk(L.cms_kfstore_debug_fetch(self.h, slot, *([None] * 10), _p(hdr), _p(misc)), "cms_kfstore_debug_fetch")
        n, nn = int(hdr[1]), int(hdr[3])
        o = dict(kps=np.zeros(n, KP_DTYPE), desc=np.zeros((n, 32), np.uint8), rays=np.zeros((n, 3), np.float32), mp=np.zeros(n, np.int32), feat_node=np.zeros(n, np.int32),
                 sorted=np.zeros(n, np.uint16), node_id=np.zeros(nn, np.int32), node_off=np.zeros(nn + 1, np.int32), node_feat=np.zeros(max(n, 1), np.int32),
                 cell_start=np.zeros(5 * 50 * 50 + 1, np.int32))
        _chk(L.cms_kfstore_debug_fetch(self.h, slot, _p(o["kps"]), _p(o["desc"]), _p(o["rays"]), _p(o["mp"]), _p(o["feat_node"]), _p(o["sorted"]), _p(o["node_id"]),
                                       _p(o["node_off"]), _p(o["node_feat"]), _p(o["cell_start"]), _p(hdr), _p(misc)), "cms_kfstore_debug_fetch")
        o["node_feat"] = o["node_feat"][:int(o["node_off"][-1]) if nn else 0]
        o["header"] = hdr; o["nvalid"] = int(misc[0]); o["kp_cnt"] = int(misc[1])
        return o

    def update_map_points(self, slot, feat, mp):
        """cms_kfstore_update_map_points: (slot, feature, new id) triples into the slots' mp rows, one asynchronous call"""
        a = [np.ascontiguousarray(v, np.int32).reshape(-1) for v in (slot, feat, mp)]
        assert len(a[0]) == len(a[1]) == len(a[2])
        L = lib()
        L.cms_kfstore_update_map_points.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3
        pp = lambda v: _p(v) if len(v) else None
        _chk(L.cms_kfstore_update_map_points(self.h, len(a[0]), pp(a[0]), pp(a[1]), pp(a[2])), "cms_kfstore_update_map_points")

    def update_poses(self, slots, R, t, Ow):
        """cms_kfstore_update_poses: poses of resident key frames after a local BA, one asynchronous call"""
        slots = np.ascontiguousarray(slots, np.int32)
        a = [np.ascontiguousarray(R, np.float32).reshape(-1), np.ascontiguousarray(t, np.float32).reshape(-1), np.ascontiguousarray(Ow, np.float32).reshape(-1)]
        assert len(a[0]) == 9 * len(slots) and len(a[1]) == 3 * len(slots) and len(a[2]) == 3 * len(slots)
        _chk(lib().cms_kfstore_update_poses(self.h, len(slots), _p(slots), _p(a[0]), _p(a[1]), _p(a[2])), "cms_kfstore_update_poses")

    def scene_median_depth(self, mpstore, slots, q=2, store=False):
        """cms_kfstore_scene_median_depth: KeyFrame::ComputeSceneMedianDepth(q) of the slots from their current mp rows and the table's positions
        -> (depth[n], n_depths[n]); a slot without a depth reads (-1.0, 0).  store: the slots with a depth also keep it as their median_depth"""
        L = lib()
        L.cms_kfstore_scene_median_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        s = np.ascontiguousarray(slots, np.int32).reshape(-1)
        depth = np.zeros(max(len(s), 1), np.float32); nd = np.zeros(max(len(s), 1), np.int32)
        _chk(L.cms_kfstore_scene_median_depth(self.h, mpstore.h, len(s), _p(s) if len(s) else None, int(q), int(bool(store)), _p(depth), _p(nd)),
             "cms_kfstore_scene_median_depth")
        return depth[:len(s)], nd[:len(s)]

    def fuse_search(self, jobs, th=3.0):
        """jobs: list of (slot, dict(skip, pos, normal, min_dist, max_dist, desc)) -> per job (best_idx, best_dist)"""
        nj = len(jobs)
        slots = np.array([j[0] for j in jobs], np.int32)
        off = np.concatenate([[0], np.cumsum([len(j[1]["pos"]) for j in jobs])]).astype(np.int32)
        cat = lambda k, dt: np.ascontiguousarray(np.concatenate([np.asarray(j[1][k]) for j in jobs]), dt)
        a = [cat("skip", np.uint8), cat("pos", np.float32), cat("normal", np.float32), cat("min_dist", np.float32), cat("max_dist", np.float32), cat("desc", np.uint8)]
        n = int(off[-1])
        bi = np.zeros(n, np.int32); bd = np.zeros(n, np.int32)
        _chk(lib().cms_kfstore_fuse_search(self.h, nj, _p(slots), _p(off), *[_p(v) for v in a], th, _p(bi), _p(bd)), "cms_kfstore_fuse_search")
        return [(bi[off[j]:off[j + 1]].copy(), bd[off[j]:off[j + 1]].copy()) for j in range(nj)]

    def fuse_search_sets(self, sets, jobs, th=3.0):
        """cms_kfstore_fuse_search_sets.  sets: list of dict(pos, normal, min_dist, max_dist, desc); jobs: list of (slot, set index, skip array or None)
        -> per job (best_idx, best_dist)"""
        soff = np.concatenate([[0], np.cumsum([len(q["pos"]) for q in sets])]).astype(np.int32)
        cat = lambda k, dt: np.ascontiguousarray(np.concatenate([np.asarray(q[k]) for q in sets]), dt)
        a = [cat("pos", np.float32), cat("normal", np.float32), cat("min_dist", np.float32), cat("max_dist", np.float32), cat("desc", np.uint8)]
        slots = np.array([j[0] for j in jobs], np.int32); jset = np.array([j[1] for j in jobs], np.int32)
        sizes = [int(soff[j[1] + 1] - soff[j[1]]) for j in jobs]
        eoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        skip = np.ascontiguousarray(np.concatenate([np.zeros(sz, np.uint8) if j[2] is None else np.asarray(j[2], np.uint8) for j, sz in zip(jobs, sizes)]), np.uint8)
        bi = np.zeros(int(eoff[-1]), np.int32); bd = np.zeros(int(eoff[-1]), np.int32)
        _chk(lib().cms_kfstore_fuse_search_sets(self.h, len(sets), _p(soff), *[_p(v) for v in a], len(jobs), _p(slots), _p(jset), _p(skip), th, _p(bi), _p(bd)),
             "cms_kfstore_fuse_search_sets")
        return [(bi[eoff[j]:eoff[j + 1]].copy(), bd[eoff[j]:eoff[j + 1]].copy()) for j in range(len(jobs))]

    def fuse_search_sets_ids(self, mpstore, sets, jobs, th=3.0):
        """cms_kfstore_fuse_search_sets_ids.  sets: list of id lists (rows of a MapPointStore of this store); jobs as in fuse_search_sets
        -> per job (best_idx, best_dist)"""
        soff = np.concatenate([[0], np.cumsum([len(q) for q in sets])]).astype(np.int32)
        ids = _ids32(np.concatenate([np.asarray(q, np.int64).reshape(-1) for q in sets]) if len(sets) else [])
        slots = np.array([j[0] for j in jobs], np.int32); jset = np.array([j[1] for j in jobs], np.int32)
        sizes = [int(soff[j[1] + 1] - soff[j[1]]) for j in jobs]
        eoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        skip = np.ascontiguousarray(np.concatenate([np.zeros(sz, np.uint8) if j[2] is None else np.asarray(j[2], np.uint8) for j, sz in zip(jobs, sizes)]), np.uint8)
        bi = np.zeros(max(int(eoff[-1]), 1), np.int32); bd = np.zeros(max(int(eoff[-1]), 1), np.int32)
        _chk(lib().cms_kfstore_fuse_search_sets_ids(self.h, mpstore.h, len(sets), _p(soff), _p(ids) if len(ids) else None, len(jobs), _p(slots), _p(jset), _p(skip), th,
                                                    _p(bi), _p(bd)), "cms_kfstore_fuse_search_sets_ids")
        return [(bi[eoff[j]:eoff[j + 1]].copy(), bd[eoff[j]:eoff[j + 1]].copy()) for j in range(len(jobs))]

    def create_new_map_points(self, jobs, check_orientation=False, cap=2048, copy=True):
        """jobs: list of (current slot, [neighbour slots in covisibility order]) -> per job (neigh, idx1, idx2, x3d).
        The job arrays and the output buffers are kept between calls with the same job list (a mapping thread calls this once per key frame,
        next to threads that hold the interpreter lock: fresh 0.8 MB of zeroed arrays per call were ~2 ms of a 3 ms call whose library
        part takes 0.3 ms).  copy=False returns views into those buffers, valid until the next call."""
        nj = len(jobs)
        key = (cap, tuple((int(j[0]), tuple(int(s) for s in j[1])) for j in jobs))      # (the content, not the list's identity: a caller may edit its list in place)
        st = getattr(self, "_cnmp", None)
        if st is None or st[0] != key:
            cur = np.array([j[0] for j in jobs], np.int32)
            neigh = np.array([s for j in jobs for s in j[1]] + [0], np.int32)
            off = np.concatenate([[0], np.cumsum([len(j[1]) for j in jobs])]).astype(np.int32)
            n_new = np.zeros(max(nj, 1), np.int32)
            on = np.zeros((max(nj, 1), cap), np.int32); o1 = np.zeros_like(on); o2 = np.zeros_like(on); ox = np.zeros((max(nj, 1), cap, 3), np.float32)
            arrs = (cur, off, neigh, n_new, on, o1, o2, ox)
            st = self._cnmp = (key, arrs, [_p(a) for a in arrs])
        cur, off, neigh, n_new, on, o1, o2, ox = st[1]
        pc, po, pn, pnn, pon, po1, po2, pox = st[2]
        t0 = time.perf_counter()
        _chk(lib().cms_kfstore_create_new_map_points(self.h, nj, pc, po, pn, int(check_orientation), cap, pnn, pon, po1, po2, pox), "cms_kfstore_create_new_map_points")
        self.last_call_ms = 1e3 * (time.perf_counter() - t0)      # the library call alone (the wrapper's array handling is Python's)
        if not copy:
            return [(on[j, :n_new[j]], o1[j, :n_new[j]], o2[j, :n_new[j]], ox[j, :n_new[j]]) for j in range(nj)]
        return [(on[j, :n_new[j]].copy(), o1[j, :n_new[j]].copy(), o2[j, :n_new[j]].copy(), ox[j, :n_new[j]].copy()) for j in range(nj)]

    def search_by_bow(self, src_ctx, jobs, nnratio=0.7, check_orientation=True):
        """cms_kfstore_search_by_bow: ORBMatcher::SearchByBoW(pKF, F, ...) for many (resident key frame, frame) pairs in ONE launch on src_ctx's stream.
        jobs: list of (slot, b, n, fv, skip): frame b of src_ctx's last batch with n key points, fv its FeatureVector (see _bow_fv), skip None or one
        byte per feature of the slot's key frame (!= 0: the map point is bad).  Returns per job (kf_idx int32[n], n_matches)."""
        arr = (BowJob * max(len(jobs), 1))()
        keep = []
        for q, (slot, b, n, fv, skip) in zip(arr, jobs):
            nid, noff, nfeat = _bow_fv(fv)
            sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
            keep.append((nid, noff, nfeat, sk))
            q.slot = slot; q.b = b; q.n = n; q.nnodes = len(nid)
            q.node_id = nid.ctypes.data; q.node_off = noff.ctypes.data; q.node_feat = nfeat.ctypes.data; q.kf_skip = None if sk is None else sk.ctypes.data
        off = np.concatenate([[0], np.cumsum([int(j[2]) for j in jobs])]).astype(np.int64)
        kf_idx = np.full(max(int(off[-1]), 1), -1, np.int32); nm = np.zeros(max(len(jobs), 1), np.int32)
        L = lib()
        L.cms_kfstore_search_by_bow.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
        _chk(L.cms_kfstore_search_by_bow(self.h, src_ctx.h, len(jobs), arr, float(nnratio), int(check_orientation), _p(kf_idx), _p(nm)), "cms_kfstore_search_by_bow")
        return [(kf_idx[off[j]:off[j + 1]].copy(), int(nm[j])) for j in range(len(jobs))]

    def search_by_bow_keyframes(self, src_ctx, jobs, nnratio=0.75, check_orientation=True):
        """cms_kfstore_search_by_bow_keyframes: ORBMatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (LoopClosing::ComputeSim3) for many pairs of resident key
        frames in ONE launch on src_ctx's stream.  jobs: list of (slot1, n1, slot2, n2, skip1, skip2): the slots with their stored key-point counts,
        skip None or one byte per feature of the slot's key frame (!= 0: the map point is bad).  Returns per job (idx2 int32[n1]: the key-frame-2
        feature whose map point key point i of key frame 1 receives, or -1; n_matches)."""
        arr = (BowKfJob * max(len(jobs), 1))()
        keep = []
        for q, (slot1, n1, slot2, n2, skip1, skip2) in zip(arr, jobs):
            sk = [None if v is None else np.ascontiguousarray(v, np.uint8) for v in (skip1, skip2)]
            keep.append(sk)
            q.slot1 = slot1; q.n1 = n1; q.slot2 = slot2; q.n2 = n2
            q.skip1 = None if sk[0] is None else sk[0].ctypes.data; q.skip2 = None if sk[1] is None else sk[1].ctypes.data
        off = np.concatenate([[0], np.cumsum([max(int(j[1]), 0) for j in jobs])]).astype(np.int64)
        idx2 = np.full(max(int(off[-1]), 1), -1, np.int32); nm = np.zeros(max(len(jobs), 1), np.int32)
        L = lib()
        L.cms_kfstore_search_by_bow_keyframes.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
        _chk(L.cms_kfstore_search_by_bow_keyframes(self.h, src_ctx.h, len(jobs), arr, float(nnratio), int(check_orientation), _p(idx2), _p(nm)),
             "cms_kfstore_search_by_bow_keyframes")
        return [(idx2[off[j]:off[j + 1]].copy(), int(nm[j])) for j in range(len(jobs))]

    def search_by_sim3(self, src_ctx, jobs, th=7.5, z_as_written=True, out=None, n_mp=None):
        """cms_kfstore_search_by_sim3: ORBMatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (LoopClosing::ComputeSim3) for many pairs of
        resident key frames in ONE call on src_ctx's stream.  jobs: list of dict(slot1, slot2, s12, R12, t12, mp1, mp2); mp1 / mp2 = per key point of that
        key frame dict(skip, pos, min_dist, max_dist, desc), skip != 0 <=> no map point, already matched or bad (the other arrays are read only where
        skip == 0).  n1 / n2 are the lengths of the skip arrays unless the job gives them.  z_as_written: the depth of line :1507 as the reference
        has it.  out: (idx2, n_found) arrays to receive the results (pinned ones, say); off1 / off2 of a job and n_mp default to the concatenation
        this wrapper builds.  Returns per job (idx2 int32[n1]: the key point of key frame 2
        whose map point key point i of key frame 1 receives, or -1; n_found)."""
        nj = len(jobs)
        arr = (Sim3SearchJob * max(nj, 1))()
        parts = []
        at = 0
        for q, j in zip(arr, jobs):
            n1, n2 = len(j["mp1"]["skip"]), len(j["mp2"]["skip"])
            q.slot1 = j["slot1"]; q.slot2 = j["slot2"]; q.n1 = j.get("n1", n1); q.n2 = j.get("n2", n2); q.s12 = float(j["s12"])
            q.R12[:] = [float(v) for v in np.asarray(j["R12"], np.float32).reshape(9)]; q.t12[:] = [float(v) for v in np.asarray(j["t12"], np.float32).reshape(3)]
            q.off1 = j.get("off1", at); q.off2 = j.get("off2", at + n1)
            at += n1 + n2
            parts += [j["mp1"], j["mp2"]]

        def cat(k, dt, tail):
            if not parts:
                return np.zeros((0,) + tail, dt)
            return np.ascontiguousarray(np.concatenate([np.asarray(m[k], dt).reshape((-1,) + tail) for m in parts]), dt)
        a = [cat("skip", np.uint8, ()), cat("pos", np.float32, (3,)), cat("min_dist", np.float32, ()), cat("max_dist", np.float32, ()), cat("desc", np.uint8, (32,))]
        off = np.concatenate([[0], np.cumsum([max(int(q.n1), 0) for q in arr[:nj]])]).astype(np.int64)
        idx2, nf = out if out is not None else (np.full(max(int(off[-1]), 1), -1, np.int32), np.zeros(max(nj, 1), np.int32))
        L = lib()
        L.cms_kfstore_search_by_sim3.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_float, C.c_int, C.c_void_p, C.c_void_p]
        _chk(L.cms_kfstore_search_by_sim3(self.h, src_ctx.h, nj, arr, at if n_mp is None else n_mp, *[_p(v) for v in a], float(th), int(bool(z_as_written)), _p(idx2), _p(nf)),
             "cms_kfstore_search_by_sim3")
        return [(idx2[off[k]:off[k + 1]].copy(), int(nf[k])) for k in range(nj)]

    def _sim3_proj_args(self, sets, jobs):
        """the shared arguments of the two Sim3 projection entries.  sets: list of dict(pos, normal, min_dist, max_dist, desc); jobs: list of
        dict(slot, n, Scw (3 x 4 or 4 x 4), set, skip (None or per point of the set), taken (None or n bytes; SearchByProjection only))"""
        soff = np.concatenate([[0], np.cumsum([len(q["pos"]) for q in sets])]).astype(np.int32)

        def cat(k, dt, tail):
            if not sets:
                return np.zeros((0,) + tail, dt)
            return np.ascontiguousarray(np.concatenate([np.asarray(q[k], dt).reshape((-1,) + tail) for q in sets]), dt)
        a = [cat("pos", np.float32, (3,)), cat("normal", np.float32, (3,)), cat("min_dist", np.float32, ()), cat("max_dist", np.float32, ()), cat("desc", np.uint8, (32,))]
        nj = len(jobs)
        arr = (Sim3ProjJob * max(nj, 1))()
        sizes = []
        for q, j in zip(arr, jobs):
            q.slot = j["slot"]; q.n = j["n"]; q.set = j["set"]
            q.Scw[:] = [float(v) for v in np.asarray(j["Scw"], np.float32).reshape(-1)[:12]]
            sizes.append(int(soff[j["set"] + 1] - soff[j["set"]]) if 0 <= j["set"] < len(sets) else 0)
        eoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        skip = None
        if any(j.get("skip") is not None for j in jobs):
            skip = np.ascontiguousarray(np.concatenate([np.zeros(sz, np.uint8) if j.get("skip") is None else np.asarray(j["skip"], np.uint8) for j, sz in zip(jobs, sizes)]
                                                       + [np.zeros(1, np.uint8)]), np.uint8)
        return soff, a, arr, eoff, skip

    def search_by_projection_sim3(self, src_ctx, sets, jobs, th=10.0, out=None):
        """cms_kfstore_search_by_projection_sim3: ORBMatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (LoopClosing::ComputeSim3's last step)
        for many (resident key frame, Scw, set of map points) jobs in ONE call on src_ctx's stream.  sets / jobs: see _sim3_proj_args; a job's taken
        flags say vpMatched[idx] != NULL on entry and are not written.  out: (match_kp, n_matches) arrays to receive the results (pinned ones, say).
        Returns per job (match_kp int32[points of its set]: the key point the point takes or -1; n_matches)."""
        soff, a, arr, eoff, skip = self._sim3_proj_args(sets, jobs)
        nj = len(jobs)
        taken = np.ascontiguousarray(np.concatenate([np.zeros(max(int(j["n"]), 0), np.uint8) if j.get("taken") is None else np.asarray(j["taken"], np.uint8) for j in jobs]
                                                    + [np.zeros(1, np.uint8)]), np.uint8)
        mk, nm = out if out is not None else (np.full(max(int(eoff[-1]), 1), -1, np.int32), np.zeros(max(nj, 1), np.int32))
        L = lib()
        L.cms_kfstore_search_by_projection_sim3.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 3 + [C.c_float, C.c_void_p, C.c_void_p]
        _chk(L.cms_kfstore_search_by_projection_sim3(self.h, src_ctx.h, len(sets), _p(soff), *[_p(v) for v in a], nj, arr, None if skip is None else _p(skip), _p(taken), float(th),
                                                     _p(mk), _p(nm)), "cms_kfstore_search_by_projection_sim3")
        return [(mk[eoff[k]:eoff[k + 1]].copy(), int(nm[k])) for k in range(nj)]

    def fuse_search_sim3(self, src_ctx, sets, jobs, th=4.0, out=None):
        """cms_kfstore_fuse_search_sim3: the search half of ORBMatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (LoopClosing::SearchAndFuse) for many
        (resident key frame, Scw, set of map points) jobs in ONE call on src_ctx's stream.  sets / jobs: see _sim3_proj_args.  out: (best_idx, best_dist)
        arrays to receive the results.  Returns per job (best_idx int32[points of its set] or -1, best_dist (256 where -1))."""
        soff, a, arr, eoff, skip = self._sim3_proj_args(sets, jobs)
        nj = len(jobs)
        bi, bd = out if out is not None else (np.full(max(int(eoff[-1]), 1), -1, np.int32), np.full(max(int(eoff[-1]), 1), 256, np.int32))
        L = lib()
        L.cms_kfstore_fuse_search_sim3.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 2 + [C.c_float, C.c_void_p, C.c_void_p]
        _chk(L.cms_kfstore_fuse_search_sim3(self.h, src_ctx.h, len(sets), _p(soff), *[_p(v) for v in a], nj, arr, None if skip is None else _p(skip), float(th), _p(bi), _p(bd)),
             "cms_kfstore_fuse_search_sim3")
        return [(bi[eoff[k]:eoff[k + 1]].copy(), bd[eoff[k]:eoff[k + 1]].copy()) for k in range(nj)]

    def compute_bow(self, vocab, slots, levelsup=4):
        """cms_kfstore_compute_bow: KeyFrame::ComputeBoW on the resident descriptors of `slots`; the FeatureVector goes into the slots' layout, the
        BowVector stays per slot (fetch_bow).  CMS_ERR_OVERFLOW (CmsError) when a FeatureVector exceeds max_nodes: no slot is changed."""
        slots = np.ascontiguousarray(slots, np.int32)
        L = lib()
        L.cms_kfstore_compute_bow.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        _chk(L.cms_kfstore_compute_bow(self.h, vocab.h, int(levelsup), len(slots), _p(slots)), "cms_kfstore_compute_bow")

    def fetch_bow(self, slot, cap=16384, feature_vector=False):
        """cms_kfstore_fetch_bow: (word_id int32, word_val float64) of the slot's BowVector; feature_vector=True: the dict of Context.fetch_bow instead
        (mBowVec and mFeatVec as arrays)"""
        o = _bow_arrays(cap, cap, cap)
        nw, nn = C.c_int(), C.c_int()
        L = lib()
        L.cms_kfstore_fetch_bow.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        fv = feature_vector
        _chk(L.cms_kfstore_fetch_bow(self.h, slot, C.byref(nw), _p(o["word_id"]), _p(o["word_val"]), cap, C.byref(nn), _p(o["node_id"]) if fv else None,
                                     _p(o["node_off"]) if fv else None, _p(o["node_feat"]) if fv else None, cap, cap), "cms_kfstore_fetch_bow")
        if fv:
            return _bow_trim(o, nw.value, nn.value)
        return o["word_id"][:nw.value].copy(), o["word_val"][:nw.value].copy()

    def search_by_bow_frames(self, src_ctx, jobs, nnratio=0.7, check_orientation=True):
        """cms_kfstore_search_by_bow_frames: search_by_bow with the frame's FeatureVector taken from the row's resident result (Context.compute_bow).
        jobs: list of (slot, b, n, skip).  Returns per job (kf_idx int32[n], n_matches)."""
        arr = (BowJob * max(len(jobs), 1))()
        keep = []
        for q, (slot, b, n, skip) in zip(arr, jobs):
            sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
            keep.append(sk)
            q.slot = slot; q.b = b; q.n = n; q.nnodes = 0
            q.node_id = None; q.node_off = None; q.node_feat = None; q.kf_skip = None if sk is None else sk.ctypes.data
        off = np.concatenate([[0], np.cumsum([int(j[2]) for j in jobs])]).astype(np.int64)
        kf_idx = np.full(max(int(off[-1]), 1), -1, np.int32); nm = np.zeros(max(len(jobs), 1), np.int32)
        L = lib()
        L.cms_kfstore_search_by_bow_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
        _chk(L.cms_kfstore_search_by_bow_frames(self.h, src_ctx.h, len(jobs), arr, float(nnratio), int(check_orientation), _p(kf_idx), _p(nm)),
             "cms_kfstore_search_by_bow_frames")
        return [(kf_idx[off[j]:off[j + 1]].copy(), int(nm[j])) for j in range(len(jobs))]

    # ---- KeyFrameDatabase over the slots (cms_kfdb_*)
    def set_bow(self, slot, word_id, word_val):
        """cms_kfstore_set_bow: the BowVector the host computed for the key frame in `slot` (ids ascending)"""
        ids = np.ascontiguousarray(word_id, np.int32); vals = np.ascontiguousarray(word_val, np.float64)
        assert len(ids) == len(vals)
        L = lib()
        L.cms_kfstore_set_bow.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _chk(L.cms_kfstore_set_bow(self.h, int(slot), len(ids), _p(ids) if len(ids) else None, _p(vals) if len(ids) else None), "cms_kfstore_set_bow")

    def db_add(self, slots, groups=None):
        """cms_kfdb_add: KeyFrameDatabase::add for the key frames in `slots`; groups: one int >= 0 per slot (default 0)"""
        slots = np.ascontiguousarray(slots, np.int32)
        groups = np.zeros(len(slots), np.int32) if groups is None else np.ascontiguousarray(groups, np.int32)
        assert len(groups) == len(slots)
        L = lib()
        L.cms_kfdb_add.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _chk(L.cms_kfdb_add(self.h, len(slots), _p(slots), _p(groups)), "cms_kfdb_add")

    def db_erase(self, slots):
        """cms_kfdb_erase: KeyFrameDatabase::erase (a slot that is not in the database is left alone)"""
        slots = np.ascontiguousarray(slots, np.int32)
        L = lib()
        L.cms_kfdb_erase.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _chk(L.cms_kfdb_erase(self.h, len(slots), _p(slots)), "cms_kfdb_erase")

    def db_clear(self, group=-1):
        """cms_kfdb_clear: KeyFrameDatabase::clear of one group, or of all (-1)"""
        L = lib()
        L.cms_kfdb_clear.argtypes = [C.c_void_p, C.c_int]
        _chk(L.cms_kfdb_clear(self.h, int(group)), "cms_kfdb_clear")

    def db_set_covisibles(self, slots, neigh):
        """cms_kfdb_set_covisibles: GetBestCovisibilityKeyFrames(10) per slot as slots, neigh int32[n, 10], best first, -1 padded"""
        slots = np.ascontiguousarray(slots, np.int32); neigh = np.ascontiguousarray(neigh, np.int32).reshape(-1, 10)
        assert len(neigh) == len(slots)
        L = lib()
        L.cms_kfdb_set_covisibles.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _chk(L.cms_kfdb_set_covisibles(self.h, len(slots), _p(slots), _p(neigh)), "cms_kfdb_set_covisibles")

    def detect_candidates(self, src_ctx, jobs, cand_cap=None, diag=True):
        """cms_kfdb_detect: DetectRelocalizationCandidates / DetectLoopCandidates for many queries as ONE launch sequence on src_ctx's stream.  jobs: see
        kfdb_jobs.  Returns per job (candidate slots, common words int32[K] or None, score bits uint32[K] or None); self.last_n_cand holds the counts,
        also when the call raises CMS_ERR_OVERFLOW (CmsError)."""
        K = self.max_keyframes
        cap = K if cand_cap is None else int(cand_cap)
        nj = len(jobs)
        arr, keep = kfdb_jobs(jobs)
        cand = np.full((max(nj, 1), max(cap, 1)), -1, np.int32); n_cand = np.zeros(max(nj, 1), np.int32)
        common = np.zeros((max(nj, 1), K), np.int32) if diag else None
        score = np.zeros((max(nj, 1), K), np.float32) if diag else None
        L = lib()
        L.cms_kfdb_detect.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 4
        self.last_n_cand = n_cand
        if cap == 0:
            cand = np.full((max(nj, 1), 1), -1, np.int32)
        t0 = time.perf_counter()
        rc = L.cms_kfdb_detect(self.h, src_ctx.h, nj, arr, cap, _p(cand), _p(n_cand), _p(common), _p(score))
        self.last_call_ms = 1e3 * (time.perf_counter() - t0)
        _chk(rc, "cms_kfdb_detect")
        if not diag:
            return [([int(c) for c in cand[j, :int(n_cand[j])]], None, None) for j in range(nj)]
        return kfdb_results(nj, K, cap, cand, n_cand, common, score)

    def bow_score(self, slot_a, slot_b):
        """cms_kfstore_bow_score: ORBVocabulary::score of the BowVectors of pairs of slots (DetectLoop's score() loop), float64[npairs]"""
        a = np.ascontiguousarray(slot_a, np.int32); b = np.ascontiguousarray(slot_b, np.int32)
        assert len(a) == len(b)
        out = np.zeros(max(len(a), 1), np.float64)
        L = lib()
        L.cms_kfstore_bow_score.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _chk(L.cms_kfstore_bow_score(self.h, len(a), _p(a), _p(b), _p(out)), "cms_kfstore_bow_score")
        return out[:len(a)]

    def search_by_projection(self, src_ctx, jobs, th=10.0, orb_dist=100, check_orientation=True):
        """cms_kfstore_search_by_projection: ORBMatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) for many (resident key frame,
        frame) pairs as ONE launch sequence on src_ctx's stream.  jobs: list of dict(slot, b, pose12, kf_feat, pos, min_dist, max_dist, desc, kp_mp):
        frame b of src_ctx's last batch (len(kp_mp) key points; kp_mp int32, >= 0 = holds a map point, updated in place) and the listed map points of
        the slot's key frame (kf_feat ascending; non-NULL, not bad, not in sAlreadyFound).  Returns per job (match int32[nmp], n_matches)."""
        arr = (KfProjJob * max(len(jobs), 1))()
        keep = []
        for q, j in zip(arr, jobs):
            kp_mp = j["kp_mp"]
            assert kp_mp.dtype == np.int32 and kp_mp.flags.c_contiguous
            a = [np.ascontiguousarray(j["kf_feat"], np.int32), np.ascontiguousarray(j["pos"], np.float32).reshape(-1, 3), np.ascontiguousarray(j["min_dist"], np.float32),
                 np.ascontiguousarray(j["max_dist"], np.float32), np.ascontiguousarray(j["desc"], np.uint8).reshape(-1, 32)]
            n = len(a[0])
            assert all(len(v) == n for v in a[1:])
            match = np.full(max(n, 1), -1, np.int32)
            keep.append((a, match, n))
            q.slot = j["slot"]; q.b = j["b"]; q.n = len(kp_mp); q.nmp = n
            q.pose12[:] = [float(v) for v in np.asarray(j["pose12"], np.float32).reshape(12)]
            q.kf_feat, q.pos, q.min_dist, q.max_dist, q.mp_desc = (v.ctypes.data for v in a)
            q.kp_mp = kp_mp.ctypes.data; q.match = match.ctypes.data
        nm = np.zeros(max(len(jobs), 1), np.int32)
        L = lib()
        L.cms_kfstore_search_by_projection.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p]
        _chk(L.cms_kfstore_search_by_projection(self.h, src_ctx.h, len(jobs), arr, float(th), int(orb_dist), int(check_orientation), _p(nm)),
             "cms_kfstore_search_by_projection")
        return [(k[1][:k[2]], int(nm[i])) for i, k in enumerate(keep)]


def _csr(lists):
    """offsets and the concatenation of a list of int lists (one spare entry: an empty array has no pointer worth passing)"""
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in lists])
    flat = np.zeros(int(off[-1]) + 1, np.int32)
    if int(off[-1]):
        wide = np.concatenate([np.asarray(x, np.int64).reshape(-1) for x in lists if len(x)])
        if wide.min() < -(1 << 31) or wide.max() >= (1 << 31):
            raise CmsError("an id or index outside the range of a 32-bit int: %d .. %d" % (int(wide.min()), int(wide.max())))
        flat[:-1] = wide
    return off, flat


class Covisibility(_Handle):
    """cms_covis: the observation index over member slots of a KeyframeStore (UpdateConnections, KeyFrameCulling, the local-map votes and points).
    Members are named by their position in the list build() was given.  Calls on one object are serialised inside the library."""
    _entries = ("cms_covis_create", "cms_covis_destroy")

    def __init__(self, store, max_members):
        L = lib()
        L.cms_covis_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.cms_covis_destroy.argtypes = [C.c_void_p]; L.cms_covis_destroy.restype = None
        L.cms_covis_build.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.cms_covis_votes.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 3
        L.cms_covis_connections.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 3
        L.cms_covis_culling.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3
        L.cms_covis_local_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        self.store = store
        self.n_members = 0
        self._create(store.h, int(max_members))

    def build(self, member_slots):
        """cms_covis_build: snapshot the members' rows as the store holds them now"""
        s = np.ascontiguousarray(member_slots, np.int32).reshape(-1)
        _chk(lib().cms_covis_build(self.h, len(s), _p(s) if len(s) else None), "cms_covis_build")
        self.n_members = len(s)

    def votes(self, src_ctx, id_lists):
        """cms_covis_votes: per frame the ids of its map points -> votes[njobs, n_members]"""
        off, ids = _csr(id_lists)
        out = np.zeros((len(id_lists), self.n_members), np.int32)
        _chk(lib().cms_covis_votes(self.h, src_ctx.h, len(id_lists), _p(off), _p(ids), _p(out) if out.size else None), "cms_covis_votes")
        return out

    def connections(self, members, th=15):
        """cms_covis_connections -> (weights[njobs, M], order[njobs, M] padded with -1, n_connected[njobs])"""
        m = np.ascontiguousarray(members, np.int32).reshape(-1)
        shape = (len(m), max(self.n_members, 1))
        w = np.zeros(shape, np.int32); order = np.full(shape, -1, np.int32); nc = np.zeros(max(len(m), 1), np.int32)
        _chk(lib().cms_covis_connections(self.h, len(m), _p(m) if len(m) else None, int(th), _p(w), _p(order), _p(nc)), "cms_covis_connections")
        return w[:, :self.n_members], order[:, :self.n_members], nc[:len(m)]

    def culling(self, chains, erasable, th_obs=3):
        """cms_covis_culling: chains of candidates (members), erasable flags of the same shape -> (n_mps, n_redundant, redundant) over all jobs"""
        off, jobs = _csr(chains)
        er = np.zeros(len(jobs), np.uint8)
        er[:int(off[-1])] = [int(bool(v)) for x in erasable for v in x]
        assert sum(len(x) for x in erasable) == int(off[-1])
        n = max(int(off[-1]), 1)
        nm = np.zeros(n, np.int32); nr = np.zeros(n, np.int32); red = np.zeros(n, np.uint8)
        _chk(lib().cms_covis_culling(self.h, len(chains), _p(off), _p(jobs), _p(er), int(th_obs), _p(nm), _p(nr), _p(red)), "cms_covis_culling")
        return nm[:int(off[-1])], nr[:int(off[-1])], red[:int(off[-1])]

    def local_points(self, src_ctx, member_lists, cap):
        """cms_covis_local_points -> (code, n_out[njobs], [ids written per job]); the code is 0 or CMS_ERR_OVERFLOW (-4), anything else raises"""
        off, kfs = _csr(member_lists)
        nj = len(member_lists)
        ids = np.full((max(nj, 1), max(int(cap), 1)), -1, np.int32); n_out = np.zeros(max(nj, 1), np.int32)
        rc = lib().cms_covis_local_points(self.h, src_ctx.h, nj, _p(off), _p(kfs), int(cap), _p(ids), _p(n_out))
        if rc != -4:
            _chk(rc, "cms_covis_local_points")
        return rc, n_out[:nj], [[int(v) for v in ids[j, :min(int(n_out[j]), int(cap))]] for j in range(nj)]

    def tracked_map_points(self, src_ctx, members, min_obs):
        """cms_covis_tracked_map_points: KeyFrame::TrackedMapPoints(min_obs[j]) of member members[j] on the index's snapshot -> count[njobs]"""
        L = lib()
        L.cms_covis_tracked_map_points.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 3
        m = np.ascontiguousarray(members, np.int32).reshape(-1)
        mo = np.ascontiguousarray(np.broadcast_to(np.asarray(min_obs, np.int32), m.shape))
        count = np.zeros(max(len(m), 1), np.int32)
        pp = lambda v: _p(v) if len(v) else None
        _chk(L.cms_covis_tracked_map_points(self.h, src_ctx.h, len(m), pp(m), pp(mo), _p(count)), "cms_covis_tracked_map_points")
        return count[:len(m)]

    def local_ba_windows(self, mps, jobs, cap_kf, cap_points, cap_edges, pinned=False, out=None):
        """cms_covis_local_ba_windows: the local BA windows of `jobs` ((local members in the reference's order, first_member or -1) each) from this
        index, its store and the MapPointStore mps.  -> one dict per job in synth.ba_problem's layout (poses, fixed, points, e_pose, e_point, e_obs,
        e_invsig2, e_face, fx, fy, cx, cy: what BundleAdjuster and ba_run take) plus kf_member, point_id, e_feat and counts.  pinned: the arrays lie
        in pinned memory the kernels store into, and the dicts carry _pinned (ba_window_array sets CMS_BA_INPUTS_PINNED).  out: arrays of
        ba_window_arrays() to fill instead of fresh ones (a refused call must leave them as they are).  CMS_ERR_OVERFLOW raises CmsOverflow with the
        counts of every job in .counts."""
        L = lib()
        L.cms_covis_local_ba_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 3 + [C.c_void_p] * 12
        nj = len(jobs)
        arr = (BaWindowJob * max(nj, 1))()
        keep = []
        for q, (members, first) in zip(arr, jobs):
            m = np.ascontiguousarray(members, np.int32).reshape(-1)
            keep.append(m)
            q.n_local = len(m); q.local_members = m.ctypes.data if len(m) else None; q.first_member = int(first)
        o = out if out is not None else ba_window_arrays(nj, cap_kf, cap_points, cap_edges, pinned)
        rc = L.cms_covis_local_ba_windows(self.h, mps.h, nj, arr, int(cap_kf), int(cap_points), int(cap_edges),
                                          *[_p(o[k]) for k in ("counts",) + BA_WINDOW_ARRAYS])
        if rc == -4:
            e = CmsOverflow(lib().cms_last_error().decode())
            e.counts = o["counts"][:nj].copy()
            raise e
        _chk(rc, "cms_covis_local_ba_windows")
        f = self.store.ctx.geom.F / 2.0
        res = []
        for j in range(nj):
            K, _, P, E = (int(v) for v in o["counts"][j])
            w = dict(poses=o["poses"][j, :K], fixed=o["fixed"][j, :K], points=o["points"][j, :P], e_pose=o["e_pose"][j, :E], e_point=o["e_point"][j, :E],
                     e_obs=o["e_obs"][j, :E], e_invsig2=o["e_invsig2"][j, :E], e_face=o["e_face"][j, :E], fx=f, fy=f, cx=f, cy=f,
                     kf_member=o["kf_member"][j, :K], point_id=o["point_id"][j, :P], e_feat=o["e_feat"][j, :E], counts=o["counts"][j].copy())
            if pinned:
                w["_pinned"] = o["_pinned"]
            res.append(w)
        return res


class BaWindowJob(C.Structure):      # cms_ba_window_job (include/cubemapslam_hip.h)
    _fields_ = [("n_local", C.c_int), ("local_members", C.c_void_p), ("first_member", C.c_int)]


class CmsOverflow(Exception):
    """CMS_ERR_OVERFLOW of an entry that still delivers its counts"""


BA_WINDOW_ARRAYS = ("kf_member", "point_id", "poses", "fixed", "points", "e_pose", "e_point", "e_obs", "e_invsig2", "e_face", "e_feat")


def ba_window_arrays(njobs, cap_kf, cap_points, cap_edges, pinned=False, fill=0):
    """the output arrays of cms_covis_local_ba_windows for njobs jobs, every byte `fill`; pinned: views of PinnedArray blocks kept under _pinned"""
    nj, ck, cp, ce = max(int(njobs), 1), int(cap_kf), int(cap_points), int(cap_edges)
    spec = dict(counts=((nj, 4), np.int32), kf_member=((nj, ck), np.int32), point_id=((nj, cp), np.int32), poses=((nj, ck, 7), np.float64), fixed=((nj, ck), np.uint8),
                points=((nj, cp, 3), np.float64), e_pose=((nj, ce), np.int32), e_point=((nj, ce), np.int32), e_obs=((nj, ce, 2), np.float64),
                e_invsig2=((nj, ce), np.float64), e_face=((nj, ce), np.int8), e_feat=((nj, ce), np.int32))
    o = dict(_pinned=[])
    for k, (shape, dt) in spec.items():
        nbytes = int(np.prod(shape)) * np.dtype(dt).itemsize
        if pinned and k != "counts":
            pa = PinnedArray((max(nbytes, 16),))
            o["_pinned"].append(pa)
            raw = pa.array[:nbytes]
        else:
            raw = np.empty(nbytes, np.uint8)
        raw[...] = fill
        o[k] = raw.view(dt).reshape(shape)
    return o


MP_DESCRIPTOR, MP_NORMAL_DEPTH = 1, 2
MP_VISIBLE, MP_FOUND = 1, 2      # the columns of MapPointStore.count


def _ids32(ids):
    """ids as a contiguous int32 array; one that does not fit is refused here, before it could wrap"""
    wide = np.asarray(ids, np.int64).reshape(-1)
    if len(wide) and (wide.min() < -(1 << 31) or wide.max() >= (1 << 31)):
        raise CmsError("an id outside the range of a 32-bit int: %d .. %d" % (int(wide.min()), int(wide.max())))
    return np.ascontiguousarray(wide, np.int32)


class MapPointStore(_Handle):
    """cms_mpstore: the map-point table next to a KeyframeStore, rows indexed by id (position, normal, distance bounds, descriptor, reference slot).
    Calls on one object are serialised inside the library."""
    _entries = ("cms_mpstore_create", "cms_mpstore_destroy")

    def __init__(self, store, max_points):
        L = lib()
        L.cms_mpstore_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.cms_mpstore_destroy.argtypes = [C.c_void_p]; L.cms_mpstore_destroy.restype = None
        L.cms_mpstore_set.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3
        L.cms_mpstore_erase.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.cms_mpstore_refresh.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.cms_mpstore_fetch.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8
        self.store = store
        self.max_points = int(max_points)
        self._create(store.h, int(max_points))

    def set(self, ids, pos=None, ref_slot=None):
        """cms_mpstore_set: world positions (n x 3 or None) and reference slots (n or None) of the rows `ids`; asynchronous"""
        ids = _ids32(ids)
        pos = None if pos is None else np.ascontiguousarray(pos, np.float32).reshape(-1)
        ref = None if ref_slot is None else np.ascontiguousarray(ref_slot, np.int32).reshape(-1)
        assert (pos is None or len(pos) == 3 * len(ids)) and (ref is None or len(ref) == len(ids))
        pp = lambda v: _p(v) if v is not None and len(v) else None
        _chk(lib().cms_mpstore_set(self.h, len(ids), pp(ids), pp(pos), pp(ref)), "cms_mpstore_set")

    def erase(self, ids):
        """cms_mpstore_erase: the rows are empty again; asynchronous"""
        ids = _ids32(ids)
        _chk(lib().cms_mpstore_erase(self.h, len(ids), _p(ids) if len(ids) else None), "cms_mpstore_erase")

    def refresh(self, covis, ids, what=MP_DESCRIPTOR | MP_NORMAL_DEPTH):
        """cms_mpstore_refresh: descriptor and / or normal and depth of the rows `ids` from the index -> status per id (0 done, 1 no observation,
        2 the reference slot does not observe the id)"""
        ids = _ids32(ids)
        status = np.zeros(max(len(ids), 1), np.uint8)
        _chk(lib().cms_mpstore_refresh(self.h, covis.h, len(ids), _p(ids) if len(ids) else None, int(what), _p(status)), "cms_mpstore_refresh")
        return status[:len(ids)]

    def fetch(self, ids):
        """cms_mpstore_fetch -> dict(pos, normal, min_dist, max_dist, desc, best_member, best_feature) of the rows `ids`"""
        ids = _ids32(ids)
        n = len(ids)
        o = dict(pos=np.zeros((n, 3), np.float32), normal=np.zeros((n, 3), np.float32), min_dist=np.zeros(n, np.float32), max_dist=np.zeros(n, np.float32),
                 desc=np.zeros((n, 32), np.uint8), best_member=np.zeros(n, np.int32), best_feature=np.zeros(n, np.int32))
        if n:
            _chk(lib().cms_mpstore_fetch(self.h, n, _p(ids), _p(o["pos"]), _p(o["normal"]), _p(o["min_dist"]), _p(o["max_dist"]), _p(o["desc"]), _p(o["best_member"]),
                                         _p(o["best_feature"])), "cms_mpstore_fetch")
        return o

    # ---- the statistics columns (mnVisible, mnFound, mnFirstKFid) and LocalMapping::MapPointCulling
    @staticmethod
    def _stats_lib():
        L = lib()
        L.cms_mpstore_set_stats.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
        L.cms_mpstore_add_stats.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3
        L.cms_mpstore_fetch_stats.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
        L.cms_mpstore_count.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_int]
        L.cms_mpstore_culling.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p]
        return L

    @staticmethod
    def _column(v, n):
        if v is None:
            return None
        v = np.ascontiguousarray(v, np.int32).reshape(-1)
        assert len(v) == n
        return v

    def set_stats(self, ids, first_kf=None, visible=None, found=None):
        """cms_mpstore_set_stats: absolute mnFirstKFid / mnVisible / mnFound of set rows (None = unchanged); asynchronous"""
        ids = _ids32(ids)
        a = [self._column(v, len(ids)) for v in (first_kf, visible, found)]
        pp = lambda v: _p(v) if v is not None and len(v) else None
        _chk(self._stats_lib().cms_mpstore_set_stats(self.h, len(ids), pp(ids), *[pp(v) for v in a]), "cms_mpstore_set_stats")

    def add_stats(self, ids, d_visible=None, d_found=None):
        """cms_mpstore_add_stats: IncreaseVisible(n) / IncreaseFound(n) of set rows (None = 0); asynchronous"""
        ids = _ids32(ids)
        a = [self._column(v, len(ids)) for v in (d_visible, d_found)]
        pp = lambda v: _p(v) if v is not None and len(v) else None
        _chk(self._stats_lib().cms_mpstore_add_stats(self.h, len(ids), pp(ids), *[pp(v) for v in a]), "cms_mpstore_add_stats")

    def fetch_stats(self, ids):
        """cms_mpstore_fetch_stats -> (visible, found, first_kf) of the rows `ids`; an empty row reads (1, 1, -1)"""
        ids = _ids32(ids)
        n = len(ids)
        o = [np.zeros(n, np.int32) for _ in range(3)]
        if n:
            _chk(self._stats_lib().cms_mpstore_fetch_stats(self.h, n, _p(ids), _p(o[0]), _p(o[1]), _p(o[2])), "cms_mpstore_fetch_stats")
        return tuple(o)

    def count(self, src_ctx, which, id_lists, flags=None, count_if=1):
        """cms_mpstore_count: per frame a list of ids (-1 = no point) and, or None for all frames, a list of flags of the same length; an entry adds 1
        to column `which` (MP_VISIBLE / MP_FOUND) iff its id is >= 0 and (flags is None or (flag != 0) == (count_if != 0)).  Asynchronous on
        src_ctx's stream"""
        off, ids = _csr(id_lists)
        fl = None
        if flags is not None:
            assert [len(f) for f in flags] == [len(x) for x in id_lists]
            fl = np.zeros(len(ids), np.uint8)
            if int(off[-1]):
                fl[:-1] = np.concatenate([np.asarray(f, np.uint8).reshape(-1) for f in flags if len(f)])
        _chk(self._stats_lib().cms_mpstore_count(self.h, src_ctx.h, int(which), len(id_lists), _p(off), _p(ids), _p(fl), int(count_if)), "cms_mpstore_count")

    def culling(self, covis, id_lists, current_kf, th_obs=2, apply=False):
        """cms_mpstore_culling: per MapPointCulling call the recent ids and the current key frame's mnId -> one array of verdicts per job (0 stays,
        1 bad by found ratio, 2 bad by too few observations, 3 leaves the list, 4 empty row).  apply: SetBadFlag of verdicts 1 and 2 on the store's
        mp rows and the table"""
        off, ids = _csr(id_lists)
        cur = np.zeros(len(id_lists) + 1, np.int32)
        cur[:-1] = np.asarray(current_kf, np.int32).reshape(-1)
        verdict = np.zeros(len(ids), np.uint8)
        _chk(self._stats_lib().cms_mpstore_culling(self.h, covis.h, len(id_lists), _p(off), _p(ids), _p(cur), int(th_obs), int(bool(apply)), _p(verdict)),
             "cms_mpstore_culling")
        return [verdict[off[j]:off[j + 1]].copy() for j in range(len(id_lists))]


def distinctive_descriptors(ctx, obs_off, desc):
    obs_off = np.ascontiguousarray(obs_off, np.int32); desc = np.ascontiguousarray(desc, np.uint8)
    out = np.zeros(len(obs_off) - 1, np.int32)
    _chk(lib().cms_distinctive_descriptors(ctx.h, len(out), _p(obs_off), _p(desc), _p(out)), "cms_distinctive_descriptors")
    return out


def update_normal_and_depth(ctx, obs_off, pos, obs_Ow, ref_Ow, ref_level, normal, min_dist, max_dist):
    """normal / min_dist / max_dist: float32 arrays updated in place"""
    a = [np.ascontiguousarray(obs_off, np.int32), np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(obs_Ow, np.float32),
         np.ascontiguousarray(ref_Ow, np.float32), np.ascontiguousarray(ref_level, np.int32)]
    _chk(lib().cms_update_normal_and_depth(ctx.h, len(a[0]) - 1, *[_p(v) for v in a], _p(normal), _p(min_dist), _p(max_dist)), "cms_update_normal_and_depth")


def fuse_search(ctx, b, pose15, skip, pos, normal, min_dist, max_dist, desc, th):
    """search half of ORBMatcher::Fuse against key-frame slot b -> (best_idx, best_dist)"""
    n = len(pos)
    a = [np.ascontiguousarray(pose15, np.float32), np.ascontiguousarray(skip, np.uint8), np.ascontiguousarray(pos, np.float32),
         np.ascontiguousarray(normal, np.float32), np.ascontiguousarray(min_dist, np.float32), np.ascontiguousarray(max_dist, np.float32),
         np.ascontiguousarray(desc, np.uint8)]
    bi = np.zeros(n, np.int32); bd = np.zeros(n, np.int32)
    _chk(lib().cms_fuse_search(ctx.h, b, _p(a[0]), n, *[_p(v) for v in a[1:]], th, _p(bi), _p(bd)), "cms_fuse_search")
    return bi, bd


class BundleAdjuster(_Handle):
    """cms_ba: one local-BA window resident on the device."""
    _entries = ("cms_ba_create", "cms_ba_destroy")

    def __init__(self, prob, device=0):
        self.prob = prob
        self.K, self.P, self.E = len(prob["poses"]), len(prob["points"]), len(prob["e_pose"])
        poses = np.ascontiguousarray(prob["poses"], np.float64); pts = np.ascontiguousarray(prob["points"], np.float64)
        self._create(device, self.K, _p(poses), _p(prob["fixed"]), self.P, _p(pts), self.E, _p(prob["e_pose"]), _p(prob["e_point"]),
                     _p(np.ascontiguousarray(prob["e_obs"], np.float64)), _p(prob["e_invsig2"]), _p(prob["e_face"]), prob["fx"], prob["fy"], prob["cx"], prob["cy"])

    @classmethod
    def from_handle(cls, prob, handle):
        self = cls.__new__(cls)
        self.prob = prob
        self.K, self.P, self.E = len(prob["poses"]), len(prob["points"]), len(prob["e_pose"])
        self.h = C.c_void_p(handle)
        return self

    def reset(self):
        _chk(lib().cms_ba_reset(self.h), "cms_ba_reset")

    def optimize(self, its=(5, 10), stop=None):
        st = BaStats()
        stop_arr = np.array([1 if stop else 0], np.uint8)
        rc = _chk(lib().cms_ba_optimize(self.h, its[0], its[1], _p(stop_arr), C.byref(st)), "cms_ba_optimize")
        return rc, st

    def read(self):
        poses = np.zeros((self.K, 7)); pts = np.zeros((self.P, 3)); flags = np.zeros(self.E, np.uint8)
        _chk(lib().cms_ba_read(self.h, _p(poses), _p(pts), _p(flags)), "cms_ba_read")
        return poses, pts, flags

    def fetch_plan(self):
        """cms_ba_debug_fetch_plan: the plan arrays as the device holds them (whichever planner made the window)"""
        P, E = self.P, self.E
        out = dict(pinv=np.zeros(P, np.int32), perm=np.zeros(E, np.int32), info=np.zeros(E, np.uint32), pt_off=np.zeros(P + 1, np.int32),
                   e_pose=np.zeros(E, np.int32), e_point=np.zeros(E, np.int32), e_face=np.zeros(E, np.int8), chunk_e0=np.zeros(P + 2, np.int32),
                   rm_chunk=np.zeros((P, 4), np.int32), rm_cost=np.zeros(P + 2, np.uint32), run_mf=np.zeros((P, 64), np.uint32), run_fl=np.zeros((P, 64, 12), np.uint32))
        cnt = np.zeros(8, np.int32)
        L = lib()
        _chk(L.cms_ba_debug_fetch_plan(self.h, _p(out["pinv"]), _p(out["perm"]), _p(out["info"]), _p(out["pt_off"]), _p(out["e_pose"]), _p(out["e_point"]),
                                       _p(out["e_face"]), _p(out["chunk_e0"]), _p(out["rm_chunk"]), _p(out["rm_cost"]), _p(out["run_mf"]), _p(out["run_fl"]), _p(cnt)),
             "cms_ba_debug_fetch_plan")
        nch, n_rm, nr = int(cnt[0]), int(cnt[1]), int(cnt[2])
        out.update(n_chunks=nch, n_rm=n_rm, n_runs=nr, np=int(cnt[3]), rm_points=int(cnt[4]), R_rm=int(cnt[5]), R=int(cnt[6]), device_planned=bool(cnt[7]), plan_kernel=int(cnt[7]) == 2)
        out["chunk_e0"] = out["chunk_e0"][:nch + 1].copy(); out["rm_chunk"] = out["rm_chunk"][:n_rm].copy(); out["rm_cost"] = out["rm_cost"][:nch + 1].copy()
        out["run_mf"] = out["run_mf"][:nr].copy(); out["run_fl"] = out["run_fl"][:nr].copy()
        return out

    @property
    def stream(self):
        return lib().cms_ba_stream(self.h)

    def set_stream(self, hip_stream):
        f = lib().cms_ba_set_stream
        f.argtypes = [C.c_void_p, C.c_void_p]
        _chk(f(self.h, C.c_void_p(int(hip_stream))), "cms_ba_set_stream")

    def profile_kernel(self, kernel_id):
        """HIP events around one kernel of the grouped driver's rounds (group owned by this handle); 3 = kb_ba_schur_points"""
        _chk(lib().cms_ba_profile_kernel(self.h, kernel_id), "cms_ba_profile_kernel")

    def profile_get(self):
        ms = C.c_double(0); n = C.c_long(0)
        _chk(lib().cms_ba_profile_get(self.h, C.byref(ms), C.byref(n)), "cms_ba_profile_get")
        return ms.value, n.value


def ba_compose_chunks(fixed, n_points, e_pose, e_point, lookahead=48):
    """Host-only: the chunk composition of the edge-major Schur kernel (cms_ba_debug_compose).  Returns (pinv, chunk_pt0, rank)."""
    fixed = np.ascontiguousarray(fixed, np.uint8); e_pose = np.ascontiguousarray(e_pose, np.int32); e_point = np.ascontiguousarray(e_point, np.int32)
    P, E = int(n_points), len(e_pose)
    pinv = np.zeros(P, np.int32); pt0 = np.zeros(P + 1, np.int32); rank = np.zeros(E, np.uint8)
    n = C.c_int(0)
    _chk(lib().cms_ba_debug_compose(len(fixed), _p(fixed), P, E, _p(e_pose), _p(e_point), int(lookahead), _p(pinv), _p(pt0), C.byref(n), _p(rank)),
         "cms_ba_debug_compose")
    return pinv, pt0[:n.value + 1].copy(), rank


def ba_plan(fixed, n_points, e_pose, e_point, tables=False):
    """Host-only: the plan cms_ba_create makes (cms_ba_debug_plan): internal order, chunks, signature runs and the run-major kernel's tables."""
    fixed = np.ascontiguousarray(fixed, np.uint8); e_pose = np.ascontiguousarray(e_pose, np.int32); e_point = np.ascontiguousarray(e_point, np.int32)
    P, E = int(n_points), len(e_pose)
    pinv = np.zeros(P, np.int32); perm = np.zeros(E, np.int32); info = np.zeros(E, np.uint32); pt0 = np.zeros(P + 2, np.int32)
    rmc = np.zeros((P, 4), np.int32); rl = np.zeros((P, 64, 2), np.uint32); cnt = np.zeros(8, np.int32)
    mf = np.zeros((P, 64), np.uint32) if tables else None; fl = np.zeros((P, 64, 12), np.uint32) if tables else None
    _chk(lib().cms_ba_debug_plan(len(fixed), _p(fixed), P, E, _p(e_pose), _p(e_point), _p(pinv), _p(perm), _p(info), _p(pt0), _p(rmc), _p(rl), _p(cnt),
                                 _p(mf), _p(fl)), "cms_ba_debug_plan")
    nch, n_rm, nruns = int(cnt[0]), int(cnt[1]), int(cnt[2])
    return dict(pinv=pinv, perm=perm, info=info, chunk_pt0=pt0[:nch + 1].copy(), rm_chunk=rmc[:n_rm].copy(), run_lane=rl[:nruns].copy(), n_chunks=nch,
                run_mf=None if mf is None else mf[:nruns].copy(), run_fl=None if fl is None else fl[:nruns].copy(),
                n_rm=n_rm, n_runs=nruns, np=int(cnt[3]), rm_points=int(cnt[4]), R_rm=int(cnt[5]), R=int(cnt[6]), usable=bool(cnt[7]))


def ba_plan_fast(fixed, n_points, e_pose, e_point):
    """Host-only: the device-side planner's result for a window (cms_ba_debug_plan_fast); `usable` False when it does not take the window."""
    fixed = np.ascontiguousarray(fixed, np.uint8); e_pose = np.ascontiguousarray(e_pose, np.int32); e_point = np.ascontiguousarray(e_point, np.int32)
    P, E = int(n_points), len(e_pose)
    pinv = np.zeros(P, np.int32); perm = np.zeros(E, np.int32); info = np.zeros(E, np.uint32); pt0 = np.zeros(P + 2, np.int32)
    rmc = np.zeros((P, 4), np.int32); cnt = np.zeros(8, np.int32); mf = np.zeros((P, 64), np.uint32); fl = np.zeros((P, 64, 12), np.uint32)
    _chk(lib().cms_ba_debug_plan_fast(len(fixed), _p(fixed), P, E, _p(e_pose), _p(e_point), _p(pinv), _p(perm), _p(info), _p(pt0), _p(rmc), _p(cnt), _p(mf), _p(fl)),
         "cms_ba_debug_plan_fast")
    nch, n_rm, nruns = int(cnt[0]), int(cnt[1]), int(cnt[2])
    return dict(pinv=pinv, perm=perm, info=info, chunk_pt0=pt0[:nch + 1].copy(), rm_chunk=rmc[:n_rm].copy(), n_chunks=nch, run_mf=mf[:nruns].copy(), run_fl=fl[:nruns].copy(),
                n_rm=n_rm, n_runs=nruns, np=int(cnt[3]), rm_points=int(cnt[4]), R_rm=int(cnt[5]), R=int(cnt[6]), usable=bool(cnt[7]))


def ba_run_fg(fixed, n_points, e_pose, e_point, fast=False):
    """Host-only: the tables of the opt-in one-wavefront run workgroups (cms_ba_debug_run_fg); None when the planner does not take the window."""
    fixed = np.ascontiguousarray(fixed, np.uint8); e_pose = np.ascontiguousarray(e_pose, np.int32); e_point = np.ascontiguousarray(e_point, np.int32)
    P, E = int(n_points), len(e_pose)
    fg = np.zeros((P, 64, 24), np.uint32); cut = np.zeros((2, 1025), np.int32); cnt = np.zeros(4, np.int32)
    _chk(lib().cms_ba_debug_run_fg(len(fixed), _p(fixed), P, E, _p(e_pose), _p(e_point), 1 if fast else 0, _p(fg), _p(cut), _p(cnt)), "cms_ba_debug_run_fg")
    if cnt[0] < 0:
        return None
    return dict(run_fg=fg[:int(cnt[0])].copy(), rm_cut=cut, n_runs=int(cnt[0]), n_rm=int(cnt[1]), n_rmA=int(cnt[2]), np=int(cnt[3]))


class BaWindow(C.Structure):      # cms_ba_window (include/cubemapslam_hip.h)
    _fields_ = [("K", C.c_int), ("poses", C.c_void_p), ("fixed", C.c_void_p), ("P", C.c_int), ("points", C.c_void_p), ("E", C.c_int), ("e_pose", C.c_void_p),
                ("e_point", C.c_void_p), ("e_obs", C.c_void_p), ("e_invsig2", C.c_void_p), ("e_face", C.c_void_p), ("fx", C.c_double), ("fy", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double), ("flags", C.c_int)]


def pin_problem(prob):
    """a copy of a BA problem whose observation-sized arrays lie in pinned host memory (cms_host_alloc), for cms_ba_window.flags = CMS_BA_INPUTS_PINNED;
    the PinnedArray objects travel with the dict and keep the memory alive"""
    q = dict(prob); keep = []
    for key, dt in (("points", np.float64), ("e_pose", np.int32), ("e_point", np.int32), ("e_obs", np.float64), ("e_invsig2", np.float64), ("e_face", np.int8)):
        a = np.ascontiguousarray(prob[key], dt)
        pa = PinnedArray((max(a.nbytes, 16),))
        v = pa.array[:a.nbytes].view(dt).reshape(a.shape); v[...] = a
        q[key] = v; keep.append(pa)
    q["_pinned"] = keep
    return q


def ba_window_array(probs):
    """(array of cms_ba_window, the numpy arrays it points into) for cms_ba_create_many; the problems' arrays must stay alive while the call runs"""
    arr = (BaWindow * len(probs))()
    keep = []
    for q, p in zip(arr, probs):
        a = [np.ascontiguousarray(p["poses"], np.float64), np.ascontiguousarray(p["fixed"], np.uint8), np.ascontiguousarray(p["points"], np.float64),
             np.ascontiguousarray(p["e_pose"], np.int32), np.ascontiguousarray(p["e_point"], np.int32), np.ascontiguousarray(p["e_obs"], np.float64),
             np.ascontiguousarray(p["e_invsig2"], np.float64), np.ascontiguousarray(p["e_face"], np.int8)]
        keep.append(a)
        q.K = len(a[0]); q.poses = a[0].ctypes.data; q.fixed = a[1].ctypes.data; q.P = len(a[2]); q.points = a[2].ctypes.data; q.E = len(a[3])
        q.e_pose = a[3].ctypes.data; q.e_point = a[4].ctypes.data; q.e_obs = a[5].ctypes.data; q.e_invsig2 = a[6].ctypes.data; q.e_face = a[7].ctypes.data
        q.fx = p["fx"]; q.fy = p["fy"]; q.cx = p["cx"]; q.cy = p["cy"]
        q.flags = (1 if p.get("_pinned") else 0) | (2 if p.get("_plan_on_device") else 0)      # CMS_BA_INPUTS_PINNED: pin_problem() made the arrays; CMS_BA_PLAN_ON_DEVICE
    return arr, keep


def ba_create_many(probs, device=0, threads=4, windows=None):
    """cms_ba_create_many: the windows of a group in one call (host parts on `threads` threads, one set-up launch per eight device-planned windows).
    windows: a prepared ba_window_array(probs) (bench.py builds it once per problem set)."""
    n = len(probs)
    arr, keep = windows if windows is not None else ba_window_array(probs)
    handles = (C.c_void_p * n)()
    L = lib()
    L.cms_ba_create_many.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    _chk(L.cms_ba_create_many(handles, n, device, arr, threads), "cms_ba_create_many")
    return [BundleAdjuster.from_handle(p, handles[i]) for i, p in enumerate(probs)]


def ba_read_many(bas):
    """cms_ba_read_many: [(poses, points, outlier flags)] of optimised windows, one gather launch per sixteen device-planned windows"""
    n = len(bas)
    outs = [(np.zeros((b.K, 7)), np.zeros((b.P, 3)), np.zeros(b.E, np.uint8)) for b in bas]
    handles = (C.c_void_p * n)(*[b.h for b in bas])
    pp = (C.c_void_p * n)(*[o[0].ctypes.data for o in outs]); pq = (C.c_void_p * n)(*[o[1].ctypes.data for o in outs]); pf = (C.c_void_p * n)(*[o[2].ctypes.data for o in outs])
    L = lib()
    L.cms_ba_read_many.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    _chk(L.cms_ba_read_many(handles, n, pp, pq, pf), "cms_ba_read_many")
    return outs


def ba_pool_trim(device=0):
    """cms_ba_pool_trim: hand the device slabs and pinned blocks that closed windows left in the pool back to the runtime -> bytes released"""
    n = C.c_size_t(0)
    L = lib()
    L.cms_ba_pool_trim.argtypes = [C.c_int, C.c_void_p]
    _chk(L.cms_ba_pool_trim(int(device), C.byref(n)), "cms_ba_pool_trim")
    return int(n.value)


def ba_set_deterministic(on):
    """cms_ba_set_deterministic: windows created afterwards run the fixed-order (bit-repeatable) kernels, like the reference's single-threaded g2o."""
    _chk(lib().cms_ba_set_deterministic(int(on) if not isinstance(on, bool) else (1 if on else 0)), "cms_ba_set_deterministic")      # (an integer >= 2: workgroups per window)


def ba_get_deterministic():
    return bool(lib().cms_ba_get_deterministic())


def ba_optimize_many(bas, its=(5, 10), stop=None, stop_array=None):
    """cms_ba_optimize_many: advance several BundleAdjuster windows in lock-step from one host thread.  stop_array: a uint8[1] array
    another thread may set while the call runs (Optimizer::LocalBundleAdjustment's pbStopFlag); None = no flag."""
    n = len(bas)
    handles = (C.c_void_p * n)(*[b.h for b in bas])
    stats = (BaStats * n)()
    stop_arr = stop_array if stop_array is not None else (np.array([1], np.uint8) if stop else None)
    lib().cms_ba_optimize_many.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    rc = _chk(lib().cms_ba_optimize_many(handles, n, its[0], its[1], _p(stop_arr), stats), "cms_ba_optimize_many")
    return rc, list(stats)


def ba_run(prob, its=(5, 10), stop=None, device=0):
    poses = np.array(prob["poses"], np.float64, copy=True); pts = np.array(prob["points"], np.float64, copy=True)
    E = len(prob["e_pose"])
    flags = np.zeros(E, np.uint8)
    st = BaStats()
    stop_arr = np.array([1 if stop else 0], np.uint8)
    rc = _chk(lib().cms_ba_run(device, len(poses), _p(poses), _p(prob["fixed"]), len(pts), _p(pts), E, _p(prob["e_pose"]),
                               _p(prob["e_point"]), _p(np.ascontiguousarray(prob["e_obs"], np.float64)), _p(prob["e_invsig2"]),
                               _p(prob["e_face"]), prob["fx"], prob["fy"], prob["cx"], prob["cy"], its[0], its[1], _p(stop_arr),
                               _p(flags), C.byref(st)), "cms_ba_run")
    return dict(rc=rc, poses=poses, points=pts, outliers=flags, stats=st)


def ba_optimize_global(bas, iterations, robust, stop=None, stop_array=None):
    """cms_ba_optimize_global_many: Optimizer::BundleAdjustment's one optimize(iterations) (Optimizer.cpp:570-572) over windows that have not
    been optimised since they were created or reset; Huber(sqrt(5.99)) on every edge if robust, no classification.  bas: one BundleAdjuster or
    a list.  -> (rc, [BaStats]) in the caller's order (slot [0] used)."""
    if isinstance(bas, BundleAdjuster):
        bas = [bas]
    n = len(bas)
    handles = (C.c_void_p * n)(*[b.h for b in bas])
    stats = (BaStats * n)()
    stop_arr = stop_array if stop_array is not None else (np.array([1], np.uint8) if stop else None)
    L = lib()
    L.cms_ba_optimize_global_many.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    rc = _chk(L.cms_ba_optimize_global_many(handles, n, int(iterations), 1 if robust else 0, _p(stop_arr), stats), "cms_ba_optimize_global_many")
    return rc, list(stats)


def ba_run_global(prob, iterations=10, robust=False, stop=None, device=0):
    """create, cms_ba_optimize_global, read, destroy -- ba_run's return shape (the outlier flags stay zero: global BA classifies nothing)"""
    ba = BundleAdjuster(prob, device)
    try:
        rc, st = ba_optimize_global([ba], iterations, robust, stop)
        poses, pts, flags = ba.read()
    finally:
        ba.close()
    return dict(rc=rc, poses=poses, points=pts, outliers=flags, stats=st[0])


def ba_solve_tiled(A, b, device=0):
    """cms_ba_debug_solve_tiled: the tiled LDL^T solve of a dense symmetric system on its own (the lower triangle of A is read) -> (x, status)"""
    A = np.ascontiguousarray(A, np.float64); b = np.ascontiguousarray(b, np.float64)
    n = int(b.shape[0])
    if A.shape != (n, n):
        raise ValueError("ba_solve_tiled: A must be n x n")
    x = np.zeros(n); status = np.zeros(1, np.int32)
    L = lib()
    L.cms_ba_debug_solve_tiled.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _chk(L.cms_ba_debug_solve_tiled(int(device), n, _p(A), _p(b), _p(x), _p(status)), "cms_ba_debug_solve_tiled")
    return x, int(status[0])


def ba_solve_timed(A, b, which=0, reps=3, device=0):
    """cms_ba_debug_solve_timed: (x, status, mean milliseconds per solve by HIP events); which: 0 the tiled solve, 1 k_ba_solve (n <= 1024)"""
    A = np.ascontiguousarray(A, np.float64); b = np.ascontiguousarray(b, np.float64)
    n = int(b.shape[0])
    x = np.zeros(n); status = np.zeros(1, np.int32); ms = np.zeros(1)
    L = lib()
    L.cms_ba_debug_solve_timed.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    _chk(L.cms_ba_debug_solve_timed(int(device), int(which), n, _p(A), _p(b), _p(x), _p(status), int(reps), _p(ms)), "cms_ba_debug_solve_timed")
    return x, int(status[0]), float(ms[0])


def ba_linearize(prob, robust=True, delta=float(np.sqrt(5.991)), device=0):
    K, P, E = len(prob["poses"]), len(prob["points"]), len(prob["e_pose"])
    poses = np.ascontiguousarray(prob["poses"], np.float64); pts = np.ascontiguousarray(prob["points"], np.float64)
    o = dict(err=np.zeros((E, 2)), Hpp=np.zeros((K, 6, 6)), bp=np.zeros((K, 6)), Hll=np.zeros((P, 3, 3)), bl=np.zeros((P, 3)),
             Hpl=np.zeros((E, 6, 3)), chi=np.zeros(1))
    _chk(lib().cms_ba_linearize(device, K, _p(poses), _p(prob["fixed"]), P, _p(pts), E, _p(prob["e_pose"]), _p(prob["e_point"]),
                                _p(np.ascontiguousarray(prob["e_obs"], np.float64)), _p(prob["e_invsig2"]), _p(prob["e_face"]),
                                prob["fx"], prob["fy"], prob["cx"], prob["cy"], 1 if robust else 0, float(delta), _p(o["err"]),
                                _p(o["Hpp"]), _p(o["bp"]), _p(o["Hll"]), _p(o["bl"]), _p(o["Hpl"]), _p(o["chi"])), "cms_ba_linearize")
    return o


class PoseStats(C.Structure):
    _fields_ = [("rounds", C.c_int), ("n_bad", C.c_int), ("iterations_done", C.c_int * 4)]


class PoseOptimizer(_Handle):
    """Optimizer::PoseOptimization for a batch of frames (cms_pose_*): problems are dicts like synth.pose_problem()."""
    _entries = ("cms_pose_create", "cms_pose_destroy")

    def __init__(self, max_frames, max_edges, device=0):
        self._create(device, max_frames, max_edges)
        self.nf = 0

    def stream(self):
        return lib().cms_pose_stream(self.h)

    def upload(self, probs):
        self.nf = len(probs)
        cnt = [len(p["Xw"]) for p in probs]
        self.off = np.zeros(self.nf + 1, np.int32); self.off[1:] = np.cumsum(cnt)
        cat = lambda k, dt, w: (np.ascontiguousarray(np.concatenate([np.asarray(p[k], dt).reshape(-1, w) for p in probs]), dt)
                                if self.off[-1] else np.zeros((0, w), dt))
        Xw, obs, inv, face = cat("Xw", np.float64, 3), cat("obs", np.float64, 2), cat("invsig2", np.float64, 1), cat("face", np.int8, 1)
        poses = np.ascontiguousarray(np.stack([p["pose0"] for p in probs]), np.float64)
        p0 = probs[0]
        _chk(lib().cms_pose_upload(self.h, self.nf, _p(self.off), _p(Xw), _p(obs), _p(inv), _p(face), p0["fx"], p0["fy"], p0["cx"],
                                   p0["cy"], _p(poses)), "cms_pose_upload")

    def launch(self):
        _chk(lib().cms_pose_launch(self.h), "cms_pose_launch")

    def fetch(self):
        poses = np.zeros((self.nf, 7)); out = np.zeros(max(int(self.off[-1]), 1), np.uint8)
        ninl = np.zeros(self.nf, np.int32); st = (PoseStats * self.nf)()
        _chk(lib().cms_pose_fetch(self.h, _p(poses), _p(out), _p(ninl), C.byref(st)), "cms_pose_fetch")
        outs = [out[self.off[f]:self.off[f + 1]].copy() for f in range(self.nf)]
        return ninl, poses, outs, list(st)

    def optimize(self, probs):
        self.upload(probs); self.launch()
        return self.fetch()

    def optimize_batch(self, probs):
        """cms_pose_optimize_batch on this handle (a few frames: the direct path through the handle's pinned block); the resident batch of
        upload / launch is left alone.  Returns (n_inliers, poses, outlier flags per frame, stats)."""
        nf = len(probs)
        cnt = [len(q["Xw"]) for q in probs]
        off = np.zeros(nf + 1, np.int32); off[1:] = np.cumsum(cnt)
        cat = lambda k, dt, w: (np.ascontiguousarray(np.concatenate([np.asarray(q[k], dt).reshape(-1, w) for q in probs]), dt)
                                if off[-1] else np.zeros((0, w), dt))
        Xw, obs, inv, face = cat("Xw", np.float64, 3), cat("obs", np.float64, 2), cat("invsig2", np.float64, 1), cat("face", np.int8, 1)
        poses = np.ascontiguousarray(np.stack([q["pose0"] for q in probs]), np.float64)
        out = np.zeros(max(int(off[-1]), 1), np.uint8); ninl = np.zeros(nf, np.int32); st = (PoseStats * nf)()
        p0 = probs[0]
        _chk(lib().cms_pose_optimize_batch(self.h, nf, _p(off), _p(Xw), _p(obs), _p(inv), _p(face), C.c_double(p0["fx"]), C.c_double(p0["fy"]),
                                           C.c_double(p0["cx"]), C.c_double(p0["cy"]), _p(poses), _p(out), _p(ninl), C.byref(st)), "cms_pose_optimize_batch")
        return ninl, poses, [out[off[f]:off[f + 1]].copy() for f in range(nf)], list(st)


def pose_optimize(prob, n=None, device=0):
    """One frame through the one-shot entry point cms_pose_optimize; returns (n_inliers, pose7, outlier flags, stats)."""
    n = len(prob["Xw"]) if n is None else n
    pose = np.array(prob["pose0"], np.float64, copy=True)
    out = np.zeros(max(n, 1), np.uint8); ninl = np.zeros(1, np.int32); st = PoseStats()
    Xw = np.ascontiguousarray(prob["Xw"][:n], np.float64); obs = np.ascontiguousarray(prob["obs"][:n], np.float64)
    inv = np.ascontiguousarray(prob["invsig2"][:n], np.float64); face = np.ascontiguousarray(prob["face"][:n], np.int8)
    _chk(lib().cms_pose_optimize(device, n, _p(Xw), _p(obs), _p(inv), _p(face), prob["fx"], prob["fy"], prob["cx"], prob["cy"],
                                 _p(pose), _p(out), _p(ninl), C.byref(st)), "cms_pose_optimize")
    return int(ninl[0]), pose, out[:n], st


class PnpJob(C.Structure):
    """cms_pnp_job (include/cubemapslam_hip.h)"""
    _fields_ = [("N", C.c_int), ("p3d", C.c_void_p), ("p2d", C.c_void_p), ("bearing", C.c_void_p), ("sigma2", C.c_void_p), ("kp_idx", C.c_void_p),
                ("b", C.c_int), ("n", C.c_int), ("th2", C.c_float), ("min_inliers", C.c_int), ("max_its", C.c_int), ("min_set", C.c_int),
                ("n_iterations", C.c_int), ("n_draws", C.c_int), ("draws", C.c_void_p), ("iterations", C.c_int), ("best_inliers", C.c_int),
                ("best_Tcw", C.c_float * 12), ("best_mask", C.c_void_p), ("status", C.c_int), ("no_more", C.c_int), ("n_inliers", C.c_int),
                ("iterations_run", C.c_int), ("Tcw", C.c_float * 12), ("inliers", C.c_void_p)]


def ransac_parameters(N, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4):
    """cms_pnp_ransac_parameters: PnPsolver::SetRansacParameters without the per-point part -> (min_inliers, max_its, epsilon)"""
    mi, it, ep = C.c_int(), C.c_int(), C.c_float()
    L = lib()
    L.cms_pnp_ransac_parameters.argtypes = [C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    _chk(L.cms_pnp_ransac_parameters(int(N), float(probability), int(min_inliers), int(max_iterations), int(min_set), float(epsilon), C.byref(mi), C.byref(it),
                                     C.byref(ep)), "cms_pnp_ransac_parameters")
    return mi.value, it.value, ep.value


def pnp_job_state(prob, n_iterations, draws, th2=5.991, min_set=4):
    """The arrays of one PnPsolver as a dict a PnpJob points into: prob has p3d (N x 3), p2d (N x 2), bearing (N x 3), sigma2 (N), min_inliers,
    max_its, and optionally the state carried from an earlier call (iterations, best_inliers, best_Tcw, best_mask).  draws: 4 ints per iteration."""
    N = len(prob["p3d"])
    f32 = lambda a, shape: np.ascontiguousarray(np.asarray(a, np.float32).reshape(shape))
    s = dict(N=N, p3d=f32(prob["p3d"], (N, 3)), p2d=f32(prob["p2d"], (N, 2)), bearing=f32(prob["bearing"], (N, 3)), sigma2=f32(prob["sigma2"], (N,)),
             draws=np.ascontiguousarray(np.asarray(draws, np.int32).ravel()), th2=float(th2), min_inliers=int(prob["min_inliers"]), max_its=int(prob["max_its"]),
             min_set=int(min_set), n_iterations=int(n_iterations), iterations=int(prob.get("iterations", 0)), best_inliers=int(prob.get("best_inliers", 0)),
             best_Tcw=np.array(prob.get("best_Tcw", np.zeros(12)), np.float32).ravel().copy(),
             best_mask=np.array(prob.get("best_mask", np.zeros(N)), np.uint8).ravel().copy(), inliers=np.zeros(max(N, 1), np.uint8))
    if len(s["best_mask"]) == 0:
        s["best_mask"] = np.zeros(1, np.uint8)
    return s


def pnp_jobs(states):
    """(PnpJob * n) over pnp_job_state() dicts; the dicts own the memory"""
    arr = (PnpJob * len(states))()
    for q, s in zip(arr, states):
        q.N = s["N"]; q.p3d = _p(s["p3d"]); q.p2d = _p(s["p2d"]); q.bearing = _p(s["bearing"]); q.sigma2 = _p(s["sigma2"])
        q.kp_idx = _p(s["kp_idx"]) if s.get("kp_idx") is not None else None; q.b = int(s.get("b", 0)); q.n = int(s.get("n", 0))
        q.th2 = s["th2"]; q.min_inliers = s["min_inliers"]; q.max_its = s["max_its"]; q.min_set = s["min_set"]; q.n_iterations = s["n_iterations"]
        q.n_draws = len(s["draws"]); q.draws = _p(s["draws"]) if len(s["draws"]) else None
        q.iterations = s["iterations"]; q.best_inliers = s["best_inliers"]; q.best_Tcw[:] = [float(v) for v in s["best_Tcw"]]; q.best_mask = _p(s["best_mask"])
        q.inliers = _p(s["inliers"])
    return arr


def pnp_results(arr, states):
    """What a call left in the job records, one dict per job (arrays copied)"""
    out = []
    for q, s in zip(arr, states):
        N = s["N"]
        out.append(dict(status=q.status, no_more=q.no_more, n_inliers=q.n_inliers, iterations=q.iterations, iterations_run=q.iterations_run,
                        best_inliers=q.best_inliers, Tcw=np.array(q.Tcw[:], np.float32), best_Tcw=np.array(q.best_Tcw[:], np.float32),
                        inliers=s["inliers"][:N].copy(), best_mask=s["best_mask"][:N].copy()))
    return out


def pnp_first_difference(want, got):
    """Two lists of result dicts compared bit for bit (arrays by their bytes, so NaN equals NaN): None, or (job, key, wanted, got) of the first difference"""
    for j, (w, g) in enumerate(zip(want, got)):
        for k in w:
            a, b = w[k], g[k]
            if isinstance(a, np.ndarray):
                a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
                if a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes():
                    return j, k, a, b
            elif a != b:
                return j, k, a, b
    return None


class PnPSolver(_Handle):
    """PnPsolver::iterate for many solvers in one launch sequence (cms_pnp_*).  jobs: a (PnpJob * n) array, e.g. from pnp_jobs()."""
    _entries = ("cms_pnp_create", "cms_pnp_destroy")

    def __init__(self, max_jobs, max_corr_total, max_hyp_total, device=0):
        L = lib()
        L.cms_pnp_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.cms_pnp_destroy.argtypes = [C.c_void_p]
        L.cms_pnp_iterate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        self._create(device, max_jobs, max_corr_total, max_hyp_total)

    def iterate(self, ctx, jobs):
        _chk(lib().cms_pnp_iterate(self.h, ctx.h, len(jobs), jobs), "cms_pnp_iterate")
        return jobs

    def iterate_frames(self, ctx, jobs):
        """cms_pnp_iterate_frames: p2d / bearing / sigma2 gathered on the device from row b of ctx's last batch through kp_idx"""
        lib().cms_pnp_iterate_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _chk(lib().cms_pnp_iterate_frames(self.h, ctx.h, len(jobs), jobs), "cms_pnp_iterate_frames")
        return jobs

    def run(self, ctx, states, frames=False):
        """One call over pnp_job_state() dicts -> one result dict per job (the states' in/out arrays are updated in place)"""
        arr = pnp_jobs(states)
        (self.iterate_frames if frames else self.iterate)(ctx, arr)
        return pnp_results(arr, states)


class Sim3Job(C.Structure):
    """cms_sim3_job (include/cubemapslam_hip.h)"""
    _fields_ = [("N", C.c_int), ("x3dc1", C.c_void_p), ("x3dc2", C.c_void_p), ("max_err1", C.c_void_p), ("max_err2", C.c_void_p), ("fix_scale", C.c_int),
                ("min_inliers", C.c_int), ("max_its", C.c_int), ("n_iterations", C.c_int), ("n_draws", C.c_int), ("draws", C.c_void_p), ("iterations", C.c_int),
                ("best_inliers", C.c_int), ("best_R", C.c_float * 9), ("best_t", C.c_float * 3), ("best_s", C.c_float), ("best_T12", C.c_float * 12),
                ("best_mask", C.c_void_p), ("status", C.c_int), ("no_more", C.c_int), ("n_inliers", C.c_int), ("iterations_run", C.c_int), ("T12", C.c_float * 12),
                ("inliers", C.c_void_p)]


def sim3_ransac_parameters(N, probability=0.99, min_inliers=6, max_iterations=300):
    """cms_sim3_ransac_parameters: Sim3Solver::SetRansacParameters -> max_its"""
    it = C.c_int()
    L = lib()
    L.cms_sim3_ransac_parameters.argtypes = [C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p]
    _chk(L.cms_sim3_ransac_parameters(int(N), float(probability), int(min_inliers), int(max_iterations), C.byref(it)), "cms_sim3_ransac_parameters")
    return it.value


_SIM3_BEST = (("best_R", 9), ("best_t", 3), ("best_T12", 12))


def sim3_job_state(prob, n_iterations, draws):
    """The arrays of one Sim3Solver as a dict a Sim3Job points into: prob has x3dc1, x3dc2 (N x 3), max_err1, max_err2 (N), min_inliers, max_its,
    optionally fix_scale and the state carried from an earlier call (iterations, best_inliers, best_R, best_t, best_s, best_T12, best_mask).
    draws: 3 ints per iteration."""
    N = len(prob["x3dc1"])
    f32 = lambda a, shape: np.ascontiguousarray(np.asarray(a, np.float32).reshape(shape))
    s = dict(N=N, x3dc1=f32(prob["x3dc1"], (N, 3)), x3dc2=f32(prob["x3dc2"], (N, 3)), max_err1=f32(prob["max_err1"], (N,)), max_err2=f32(prob["max_err2"], (N,)),
             draws=np.ascontiguousarray(np.asarray(draws, np.int32).ravel()), fix_scale=int(prob.get("fix_scale", 0)), min_inliers=int(prob["min_inliers"]),
             max_its=int(prob["max_its"]), n_iterations=int(n_iterations), iterations=int(prob.get("iterations", 0)), best_inliers=int(prob.get("best_inliers", 0)),
             best_s=np.array([prob.get("best_s", 0.0)], np.float32),
             best_mask=np.array(prob.get("best_mask", np.zeros(N)), np.uint8).ravel().copy(), inliers=np.zeros(max(N, 1), np.uint8))
    for k, n in _SIM3_BEST:
        s[k] = np.array(prob.get(k, np.zeros(n)), np.float32).ravel().copy()
    if len(s["best_mask"]) == 0:
        s["best_mask"] = np.zeros(1, np.uint8)
    return s


def sim3_jobs(states):
    """(Sim3Job * n) over sim3_job_state() dicts; the dicts own the memory"""
    arr = (Sim3Job * len(states))()
    for q, s in zip(arr, states):
        q.N = s["N"]; q.x3dc1 = _p(s["x3dc1"]); q.x3dc2 = _p(s["x3dc2"]); q.max_err1 = _p(s["max_err1"]); q.max_err2 = _p(s["max_err2"])
        q.fix_scale = s["fix_scale"]; q.min_inliers = s["min_inliers"]; q.max_its = s["max_its"]; q.n_iterations = s["n_iterations"]
        q.n_draws = len(s["draws"]); q.draws = _p(s["draws"]) if len(s["draws"]) else None
        q.iterations = s["iterations"]; q.best_inliers = s["best_inliers"]; q.best_mask = _p(s["best_mask"]); q.inliers = _p(s["inliers"])
        for k, n in _SIM3_BEST:      # by bytes: a carried NaN keeps its bits
            C.memmove(getattr(q, k), _p(s[k]), 4 * n)
        C.memmove(C.byref(q, Sim3Job.best_s.offset), _p(s["best_s"]), 4)
    return arr


def sim3_results(arr, states):
    """What a call left in the job records, one dict per job (arrays copied)"""
    out = []
    for q, s in zip(arr, states):
        N = s["N"]
        r = dict(status=q.status, no_more=q.no_more, n_inliers=q.n_inliers, iterations=q.iterations, iterations_run=q.iterations_run,
                 best_inliers=q.best_inliers, T12=np.frombuffer(bytes(q.T12), np.float32).copy(),
                 best_s=np.frombuffer(C.string_at(C.addressof(q) + Sim3Job.best_s.offset, 4), np.float32).copy(),
                 inliers=s["inliers"][:N].copy(), best_mask=s["best_mask"][:N].copy())
        for k, _ in _SIM3_BEST:
            r[k] = np.frombuffer(bytes(getattr(q, k)), np.float32).copy()
        out.append(r)
    return out


sim3_first_difference = pnp_first_difference      # result dicts compared bit for bit: None, or (job, key, wanted, got)


class Sim3Solver(_Handle):
    """Sim3Solver::iterate for many solvers in one launch sequence (cms_sim3_*).  jobs: a (Sim3Job * n) array, e.g. from sim3_jobs()."""
    _entries = ("cms_sim3_create", "cms_sim3_destroy")

    def __init__(self, max_jobs, max_corr_total, max_hyp_total, device=0):
        L = lib()
        L.cms_sim3_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.cms_sim3_destroy.argtypes = [C.c_void_p]
        L.cms_sim3_iterate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        self._create(device, max_jobs, max_corr_total, max_hyp_total)

    def iterate(self, ctx, jobs):
        _chk(lib().cms_sim3_iterate(self.h, ctx.h, len(jobs), jobs), "cms_sim3_iterate")
        return jobs

    def run(self, ctx, states):
        """One call over sim3_job_state() dicts -> one result dict per job (the states' in/out arrays are updated in place)"""
        arr = sim3_jobs(states)
        self.iterate(ctx, arr)
        return sim3_results(arr, states)


SIM3_OPT_AS_WRITTEN, SIM3_OPT_ANALYTIC = 0, 1


class Sim3OptJob(C.Structure):
    """cms_sim3_opt_job (include/cubemapslam_hip.h)"""
    _fields_ = [("N", C.c_int), ("x3dc1", C.c_void_p), ("x3dc2", C.c_void_p), ("kp1", C.c_void_p), ("kp2", C.c_void_p), ("inv_sigma2_1", C.c_void_p),
                ("inv_sigma2_2", C.c_void_p), ("R12", C.c_double * 9), ("t12", C.c_double * 3), ("s12", C.c_double), ("th2", C.c_float), ("fix_scale", C.c_int),
                ("jacobian", C.c_int), ("n_inliers", C.c_int), ("keep", C.c_void_p), ("q12", C.c_double * 4), ("t12_out", C.c_double * 3), ("s12_out", C.c_double),
                ("n_correspondences", C.c_int), ("n_bad", C.c_int), ("iterations", C.c_int * 2)]


def sim3_opt_job_state(prob, th2=10.0, fix_scale=None, jacobian=SIM3_OPT_AS_WRITTEN):
    """The arrays of one OptimizeSim3 call as a dict a Sim3OptJob points into: prob has x3dc1, x3dc2 (N x 3), kp1, kp2 (N x 2), inv_sigma2_1,
    inv_sigma2_2 (N), R12 (3 x 3), t12, s12 and optionally fix_scale.  keep starts from a pattern, so that an untouched record shows."""
    N = len(prob["x3dc1"])
    f32 = lambda a, shape: np.ascontiguousarray(np.array(a, np.float32).reshape(shape))      # copies: a caller may edit a state
    return dict(N=N, x3dc1=f32(prob["x3dc1"], (N, 3)), x3dc2=f32(prob["x3dc2"], (N, 3)), kp1=f32(prob["kp1"], (N, 2)), kp2=f32(prob["kp2"], (N, 2)),
                inv_sigma2_1=f32(prob["inv_sigma2_1"], (N,)), inv_sigma2_2=f32(prob["inv_sigma2_2"], (N,)),
                R12=np.array(prob["R12"], np.float64).reshape(9).copy(), t12=np.array(prob["t12"], np.float64).reshape(3).copy(), s12=float(prob["s12"]),
                th2=float(th2), fix_scale=int(prob.get("fix_scale", 0) if fix_scale is None else fix_scale), jacobian=int(jacobian),
                keep=np.full(max(N, 1), 7, np.uint8))


def sim3_opt_jobs(states):
    """(Sim3OptJob * n) over sim3_opt_job_state() dicts; the dicts own the memory.  The scalar outputs start from -7."""
    arr = (Sim3OptJob * max(len(states), 1))()
    for q, s in zip(arr, states):
        q.N = s["N"]
        for k in ("x3dc1", "x3dc2", "kp1", "kp2", "inv_sigma2_1", "inv_sigma2_2", "keep"):
            setattr(q, k, _p(s[k]) if s[k] is not None else None)
        C.memmove(q.R12, _p(s["R12"]), 72); C.memmove(q.t12, _p(s["t12"]), 24)
        q.s12 = s["s12"]; q.th2 = s["th2"]; q.fix_scale = s["fix_scale"]; q.jacobian = s["jacobian"]
        q.n_inliers = -7; q.n_correspondences = -7; q.n_bad = -7; q.iterations[0] = -7; q.iterations[1] = -7
    return arr


def sim3_opt_results(arr, states):
    """What a call left in the job records, one dict per job (arrays copied)"""
    out = []
    for q, s in zip(arr, states):
        out.append(dict(n_inliers=q.n_inliers, n_correspondences=q.n_correspondences, n_bad=q.n_bad, iterations=np.array(q.iterations[:], np.int32),
                        keep=s["keep"][:s["N"]].copy(), q12=np.frombuffer(bytes(q.q12), np.float64).copy(), t12=np.frombuffer(bytes(q.t12_out), np.float64).copy(),
                        s12=np.frombuffer(C.string_at(C.addressof(q) + Sim3OptJob.s12_out.offset, 8), np.float64).copy()))
    return out


sim3_opt_first_difference = pnp_first_difference      # result dicts compared bit for bit: None, or (job, key, wanted, got)


class Sim3Optimizer(_Handle):
    """Optimizer::OptimizeSim3 for many hypotheses in one launch (cms_sim3_opt_*).  jobs: a (Sim3OptJob * n) array, e.g. from sim3_opt_jobs()."""
    _entries = ("cms_sim3_opt_create", "cms_sim3_opt_destroy")

    def __init__(self, max_jobs, max_corr_total, device=0):
        L = lib()
        L.cms_sim3_opt_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.cms_sim3_opt_destroy.argtypes = [C.c_void_p]
        L.cms_sim3_optimize.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        self._create(device, max_jobs, max_corr_total)

    def optimize(self, ctx, jobs, njobs=None):
        _chk(lib().cms_sim3_optimize(self.h, ctx.h, len(jobs) if njobs is None else njobs, jobs), "cms_sim3_optimize")
        return jobs

    def run(self, ctx, states):
        """One call over sim3_opt_job_state() dicts -> one result dict per job"""
        arr = sim3_opt_jobs(states)
        self.optimize(ctx, arr, len(states))
        return sim3_opt_results(arr, states)


class InitJob(C.Structure):
    """cms_init_job (include/cubemapslam_hip.h)"""
    _fields_ = [("n1", C.c_int), ("n2", C.c_int), ("keys1", C.c_void_p), ("rays1", C.c_void_p), ("keys2", C.c_void_p), ("rays2", C.c_void_p),
                ("matches12", C.c_void_p), ("b", C.c_int), ("sigma", C.c_float), ("iterations", C.c_int), ("n_draws", C.c_int), ("draws", C.c_void_p),
                ("status", C.c_int), ("R21", C.c_float * 9), ("t21", C.c_float * 3), ("p3d", C.c_void_p), ("triangulated", C.c_void_p),
                ("best_iteration", C.c_int), ("score", C.c_float), ("n_inliers", C.c_int), ("nGood", C.c_int * 4), ("parallax", C.c_float * 4),
                ("winner", C.c_int)]


def init_job_state(prob, draws, sigma=1.0, iterations=None, b=0):
    """The arrays of one Initializer attempt as a dict an InitJob points into: prob has keys1 (n1 x 2), rays1 (n1 x 3), keys2 (n2 x 2), rays2 (n2 x 3)
    and matches12 (n1, -1 = none).  draws: 8 ints per iteration.  The output arrays start from a pattern, so that an untouched record shows."""
    f32 = lambda a, w: np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, w))
    k1, r1, k2, r2 = f32(prob["keys1"], 2), f32(prob["rays1"], 3), f32(prob["keys2"], 2), f32(prob["rays2"], 3)
    n1 = len(k1)
    d = np.ascontiguousarray(np.asarray(draws, np.int32).ravel())
    return dict(n1=n1, n2=int(prob.get("n2", len(k2))), keys1=k1, rays1=r1, keys2=k2, rays2=r2, matches12=np.ascontiguousarray(prob["matches12"], np.int32),
                b=int(b), sigma=float(sigma), iterations=int(len(d) // 8 if iterations is None else iterations), draws=d,
                p3d=np.full((max(n1, 1), 3), 7.0, np.float32), triangulated=np.full(max(n1, 1), 9, np.uint8))


def init_jobs(states):
    """(InitJob * n) over init_job_state() dicts; the dicts own the memory.  The scalar outputs start from -7."""
    arr = (InitJob * len(states))()
    for q, s in zip(arr, states):
        q.n1 = s["n1"]; q.n2 = s["n2"]; q.keys1 = _p(s["keys1"]); q.rays1 = _p(s["rays1"]); q.keys2 = _p(s["keys2"]); q.rays2 = _p(s["rays2"])
        q.matches12 = _p(s["matches12"]); q.b = s["b"]; q.sigma = s["sigma"]; q.iterations = s["iterations"]
        q.n_draws = len(s["draws"]); q.draws = _p(s["draws"]) if len(s["draws"]) else None
        q.p3d = _p(s["p3d"]); q.triangulated = _p(s["triangulated"])
        q.status = -7; q.best_iteration = -7; q.winner = -7; q.n_inliers = -7
    return arr


def init_results(arr, states):
    """What a call left in the job records, one dict per job (arrays copied)"""
    out = []
    for q, s in zip(arr, states):
        n1 = s["n1"]
        out.append(dict(status=q.status, best_iteration=q.best_iteration, n_inliers=q.n_inliers, winner=q.winner, score=np.array([q.score], np.float32),
                        nGood=np.array(q.nGood[:], np.int32), parallax=np.array(q.parallax[:], np.float32), R21=np.array(q.R21[:], np.float32),
                        t21=np.array(q.t21[:], np.float32), p3d=s["p3d"][:n1].copy(), triangulated=s["triangulated"][:n1].copy()))
    return out


init_first_difference = pnp_first_difference      # result dicts compared bit for bit: None, or (job, key, wanted, got)


class TwoViewInitializer(_Handle):
    """Initializer::InitializeWithRays for many streams in one launch sequence (cms_init_*).  jobs: an (InitJob * n) array, e.g. from init_jobs()."""
    _entries = ("cms_init_create", "cms_init_destroy")

    def __init__(self, max_jobs, max_matches_total, max_keys1_total, max_hyp_total, device=0):
        L = lib()
        L.cms_init_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.cms_init_destroy.argtypes = [C.c_void_p]
        L.cms_init_two_view.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.cms_init_two_view_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        self._create(device, max_jobs, max_matches_total, max_keys1_total, max_hyp_total, out_last=True)

    def two_view(self, ctx, jobs, frames=False):
        L = lib()
        _chk((L.cms_init_two_view_frames if frames else L.cms_init_two_view)(self.h, ctx.h, len(jobs), jobs), "cms_init_two_view")
        return jobs

    def run(self, ctx, states):
        """One call over init_job_state() dicts -> one result dict per job"""
        arr = init_jobs(states)
        self.two_view(ctx, arr)
        return init_results(arr, states)

    def run_frames(self, ctx, states):
        """cms_init_two_view_frames: key points and key rays of frame 2 taken on the device from row b of ctx's last batch (n2 = its count)"""
        arr = init_jobs(states)
        self.two_view(ctx, arr, frames=True)
        return init_results(arr, states)


class EssGraphJob(C.Structure):
    """cms_ess_graph_job (include/cubemapslam_hip.h)"""
    _fields_ = [("N", C.c_int), ("Scw", C.c_void_p), ("Snc", C.c_void_p), ("fixed", C.c_int), ("E", C.c_int), ("edges", C.c_void_p), ("fix_scale", C.c_int),
                ("iterations", C.c_int), ("lambda_init", C.c_double), ("S_out", C.c_void_p), ("Tiw_out", C.c_void_p), ("chi2_initial", C.c_double),
                ("chi2_final", C.c_double), ("lambda_final", C.c_double), ("iterations_run", C.c_int), ("trials_run", C.c_int), ("flags", C.c_int)]


def ess_graph_job_state(graph, fix_scale=None, iterations=20, lambda_init=1e-16):
    """The arrays of one OptimizeEssentialGraph call as a dict an EssGraphJob points into: graph has Scw, Snc (N x 8: q(x y z w) | t | s), fixed, edges
    (E x 3: v0, v1, kind) and optionally fix_scale.  The output arrays start from a pattern, so that an untouched record shows."""
    Scw = np.ascontiguousarray(np.array(graph["Scw"], np.float64).reshape(-1, 8))
    N = len(Scw)
    edges = np.ascontiguousarray(np.array(graph["edges"], np.int32).reshape(-1, 3))
    return dict(N=N, Scw=Scw, Snc=np.ascontiguousarray(np.array(graph["Snc"], np.float64).reshape(N, 8)), fixed=int(graph["fixed"]), E=len(edges), edges=edges,
                fix_scale=int(graph.get("fix_scale", 0) if fix_scale is None else fix_scale), iterations=int(iterations), lambda_init=float(lambda_init),
                S_out=np.full((N, 8), 7.0, np.float64), Tiw_out=np.full((N, 12), 7.0, np.float32))


def ess_graph_jobs(states):
    """(EssGraphJob * n) over ess_graph_job_state() dicts; the dicts own the memory.  The scalar outputs start from -7."""
    arr = (EssGraphJob * max(len(states), 1))()
    for q, s in zip(arr, states):
        q.N = s["N"]; q.fixed = s["fixed"]; q.E = s["E"]; q.fix_scale = s["fix_scale"]; q.iterations = s["iterations"]; q.lambda_init = s["lambda_init"]
        for k in ("Scw", "Snc", "edges", "S_out", "Tiw_out"):
            setattr(q, k, _p(s[k]) if s[k] is not None and (k != "edges" or s["E"] > 0) else None)
        q.chi2_initial = -7.0; q.chi2_final = -7.0; q.lambda_final = -7.0; q.iterations_run = -7; q.trials_run = -7; q.flags = -7
    return arr


def ess_graph_results(arr, states):
    """What a call left in the job records, one dict per job (arrays copied)"""
    out = []
    for q, s in zip(arr, states):
        out.append(dict(S=s["S_out"].copy(), Tiw=s["Tiw_out"].copy(), chi2_initial=np.array([q.chi2_initial]), chi2_final=np.array([q.chi2_final]),
                        lambda_final=np.array([q.lambda_final]), iterations_run=q.iterations_run, trials_run=q.trials_run, flags=q.flags))
    return out


ess_graph_first_difference = pnp_first_difference      # result dicts compared bit for bit: None, or (job, key, wanted, got)


class EssentialGraphOptimizer(_Handle):
    """Optimizer::OptimizeEssentialGraph for many graphs in one launch (cms_ess_graph_*).  jobs: an (EssGraphJob * n) array, e.g. from ess_graph_jobs()."""
    _entries = ("cms_ess_graph_create", "cms_ess_graph_destroy")

    def __init__(self, max_jobs, max_vertices_total, max_edges_total, max_envelope_blocks_total, device=0):
        L = lib()
        L.cms_ess_graph_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.cms_ess_graph_destroy.argtypes = [C.c_void_p]
        L.cms_essential_graph_optimize.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        self._create(device, max_jobs, max_vertices_total, max_edges_total, max_envelope_blocks_total)

    def optimize(self, ctx, jobs, njobs=None):
        _chk(lib().cms_essential_graph_optimize(self.h, ctx.h, len(jobs) if njobs is None else njobs, jobs), "cms_essential_graph_optimize")
        return jobs

    def run(self, ctx, states):
        """One call over ess_graph_job_state() dicts -> one result dict per job"""
        arr = ess_graph_jobs(states)
        self.optimize(ctx, arr, len(states))
        return ess_graph_results(arr, states)


def sim3_correct_points(ctx, pos, ref, S_old, S_new):
    """cms_sim3_correct_points: pos (n x 3 float32), ref (n, < 0 = copied), S_old / S_new (K x 8) -> corrected positions (n x 3 float32)"""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    ref = np.ascontiguousarray(ref, np.int32)
    S_old = np.ascontiguousarray(S_old, np.float64).reshape(-1, 8); S_new = np.ascontiguousarray(S_new, np.float64).reshape(-1, 8)
    out = np.full((max(len(pos), 1), 3), 7.0, np.float32)
    f = lib().cms_sim3_correct_points
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    _chk(f(ctx.h, len(pos), _p(pos), _p(ref), len(S_old), _p(S_old), _p(S_new), _p(out)), "cms_sim3_correct_points")
    return out[:len(pos)]
