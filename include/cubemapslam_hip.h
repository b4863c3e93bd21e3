/*
 * cubemapslam_hip.h -- C-ABI of libcubemapslam_hip.so: the MI355X (gfx950) implementation of CubemapSLAM's
 * per-frame data-parallel hot path.  Plain C, caller-owned buffers, int status returns (0 = ok, <0 = error, see
 * cms_last_error()); nothing throws across this boundary and no torch / OpenCV / Eigen type appears in it.
 *
 * The reference has no FFI layer: its "boundary" is four C++ interfaces inside libCubemapSLAM.so.
 * Each entry point below names the reference interface it stands under; cubemapslam_amd/host/ holds C++ classes with
 * the reference's own signatures (ORBextractor::operator(), ORBMatcher, Optimizer::LocalBundleAdjustment,
 * System::CvtFisheyeToCubeMap_reverseQuery_withInterpolation) implemented on top of these calls, and INTEGRATION.md
 * shows the binding a maintainer of the reference would add.
 *
 * Threading contract (reference: Tracking thread extracts/matches, LocalMapping thread runs local BA concurrently,
 * System.cpp:108-127): a cms_ctx owns one HIP stream for the frame path; every cms_ba handle owns its own stream.
 * Frame-path calls on one ctx must come from one thread at a time; BA calls on one handle likewise; the two may
 * overlap freely.  The window-query, projection-search, mapping (cms_create_new_map_points, cms_kfstore_*, cms_fuse_search) and
 * map-point entries use the stream and the scratch arena of the ctx they are given: a mapping thread that runs next to a tracking
 * thread creates a context of its own (bench.py does).
 */
#ifndef CUBEMAPSLAM_HIP_H
#define CUBEMAPSLAM_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CMS_OK 0
#define CMS_ERR_ARG (-1)
#define CMS_ERR_HIP (-2)
#define CMS_ERR_UNSUPPORTED (-3)
#define CMS_ERR_OVERFLOW (-4)
#define CMS_ERR_NO_DEVICE (-5)

/* Face ids, include/CamModelGeneral.h:55-62 */
enum { CMS_FACE_UNKNOWN = -1, CMS_FACE_FRONT = 0, CMS_FACE_LEFT = 1, CMS_FACE_RIGHT = 2, CMS_FACE_UPPER = 3, CMS_FACE_LOWER = 4 };

/* What System::System reads from the YAML and hands to CamModelGeneral::SetCamParams (System.cpp:63-89). */
typedef struct {
  double c, d, e, u0, v0;  /* Camera.c/d/e/u0/v0 */
  double invpol[12];       /* Camera.pol0..11, zero padded (System.cpp:70-72) */
  double pol[5];           /* Camera.a0..4 */
  int Iw, Ih;              /* Camera.Iw / Ih */
  int face;                /* CubeFace.w == CubeFace.h; fx = fy = cx = cy = face/2 (System.cpp:83-84) */
  double fov_deg;          /* Camera.fov */
} cms_camera;

/* ORBextractor ctor arguments (include/ORBExtractor.h:55-56, Tracking.cpp:88-96) */
typedef struct { int nfeatures; float scale_factor; int nlevels; int ini_th_fast; int min_th_fast; } cms_orb_params;

/* The cv::KeyPoint fields the extractor fills (ORBExtractor.cpp:811-821, 918-919) */
typedef struct { float x, y, size, angle, response; int octave; } cms_keypoint;

typedef struct {
  int W, F, nlevels, kp_cap, max_batch;
  int level_w[12], level_h[12], level_quota[12], level_cells[12];
  float scale[12], inv_scale[12], sigma2[12], inv_sigma2[12];  /* ORBextractor::GetScaleFactors() etc. (ORBExtractor.h:67-87) */
  size_t pyramid_bytes_per_frame, candidate_entries_per_frame;
  int fisheye_stride;      /* row stride (bytes) of the device fisheye staging buffer */
} cms_geometry;

typedef struct cms_ctx cms_ctx;

const char* cms_last_error(void);
int cms_device_count(void);

/* ---- context: builds the remap LUT (System::CreateUndistortRectifyMap, System.cpp:301-324) and the extractor
 *      tables (ORBextractor::ORBextractor, ORBExtractor.cpp:381-442) once, allocates device buffers for max_batch frames. */
int cms_ctx_create(cms_ctx** out, int device, const cms_camera* cam, const cms_orb_params* orb, int max_batch);
void cms_ctx_destroy(cms_ctx* ctx);
int cms_ctx_geometry(const cms_ctx* ctx, cms_geometry* out);
void* cms_ctx_stream(cms_ctx* ctx);  /* hipStream_t of the frame path (for event timing / interop) */

/* ---- single-frame, host-buffer calls (the literal drop-in boundary)
 * cms_remap        : System::CvtFisheyeToCubeMap_reverseQuery_withInterpolation (include/System.h:106-107, System.cpp:327-355).
 *                    Writes the five face rectangles of the caller's 3F x 3F canvas; corner blocks are left untouched.
 * cms_set_mask     : the `mask` argument of ORBextractor::operator() (ORBExtractor.cpp:846-848), kept on the device.
 * cms_extract      : ORBextractor::operator()(image, mask, keypoints, descriptors) (include/ORBExtractor.h:63-65,
 *                    ORBExtractor.cpp:838-926).  *n receives the key-point count; returns CMS_ERR_OVERFLOW if cap is too small. */
int cms_remap(cms_ctx* ctx, const uint8_t* fisheye, int fstride, uint8_t* cubemap, int cstride);
int cms_set_mask(cms_ctx* ctx, const uint8_t* mask, int mstride);
/* cv::GaussianBlur(7x7, sigma 2) in front of the descriptors (ORBExtractor.cpp:907-908): column_mode 0 (default) = the integer column pass
 * (sum + 32768) >> 16 of OpenCV <= 3.2's generic path, 1 = the float column pass of its SSE2 functor (x86 builds: ties round to even for
 * the columns x < width & ~3).  OpenCV is not vendored with the reference, so both definitions are offered. */
int cms_set_gaussian_mode(cms_ctx* ctx, int column_mode);
int cms_extract(cms_ctx* ctx, const uint8_t* cubemap, int cstride, cms_keypoint* kps, uint8_t* desc, int cap, int* n);
int cms_remap_extract(cms_ctx* ctx, const uint8_t* fisheye, int fstride, cms_keypoint* kps, uint8_t* desc, int cap, int* n);
/* ... and with Frame::mvKeyRays: Frame::ComputeKeyPointRays -> CamModelGeneral::TransformCubemapToRays of every key point (src/Frame.cpp:746-760,
 * include/CamModelGeneral.h:494-513), rays[3 i .. 3 i + 2] = unit bearing vector of key point i in rig axes.  The extraction computes them anyway
 * (every consumer behind it -- PoseOptimization's and LocalBundleAdjustment's edge filter ray.z < cosFovTh, Optimizer.cpp:97 / 323-325, cms_keyframe.rays
 * -- wants them); cms_frames_rays: device pointer [max_batch][kp_cap][3] float of the batched path; cms_frames_fetch_rays: frame b's to the host. */
int cms_remap_extract_rays(cms_ctx* ctx, const uint8_t* fisheye, int fstride, cms_keypoint* kps, uint8_t* desc, float* rays, int cap, int* n);
int cms_frames_rays(cms_ctx* ctx, void** d_rays);
int cms_frames_fetch_rays(cms_ctx* ctx, int b, float* rays, int cap, int* n);

/* ---- batched, device-resident frame path (many frames / streams per launch; inputs already in HBM)
 * cms_frames_input()   : device pointer of the fisheye staging buffer, [max_batch][Ih][fisheye_stride] bytes.
 * cms_frames_upload()  : convenience host->device copy of B fisheye frames into that buffer.
 * cms_frames_process() : enqueue remap + pyramid + FAST + octree + cull + orientation + rBRIEF for frames [0,B) on the
 *                        ctx stream (asynchronous).  from_fisheye = 0 skips the remap (level 0 was uploaded by cms_extract).
 * cms_frames_results() : device pointers of the outputs: kps [max_batch][kp_cap] cms_keypoint, desc [max_batch][kp_cap][32],
 *                        counts [max_batch] int.
 * cms_frames_upload_async() : input streaming (the per-frame imread -> remap -> track loop of cubemap_lafida.cpp:128-154, batched): copies
 *                        B fisheye frames from PINNED host memory (cms_host_alloc / hipHostMalloc / hipHostRegister) on the
 *                        context's copy stream.  The staging buffer is only read by the first kernel of a batch (the remap), so the
 *                        copy of batch s + 1 overlaps the rest of batch s; the next cms_frames_process waits for it on the device.
 *                        The source must stay untouched until cms_frames_upload_wait() returns (or that process call was synced).
 */
void* cms_frames_input(cms_ctx* ctx);
int cms_frames_upload(cms_ctx* ctx, const uint8_t* fisheye, int fstride, size_t frame_pitch, int B);
int cms_frames_upload_async(cms_ctx* ctx, const uint8_t* fisheye, int fstride, size_t frame_pitch, int B);
int cms_frames_upload_wait(cms_ctx* ctx);
/* scheduling aid: `hip_stream` (cms_ctx_stream of a mapping-side context, cms_ba_stream of a window group) waits on the device for the
 * extraction of ctx's last cms_frames_process; the first call only arms the event (takes effect from the next process call on) */
int cms_stream_wait_extracted(cms_ctx* ctx, void* hip_stream);
int cms_frames_upload_device(cms_ctx* ctx, const void* d_src, int B);   /* device -> staging copy, [B][Ih][fisheye_stride], async on the ctx stream */
/* device -> device copy on the ctx stream, asynchronous: e.g. resetting the per-key-point map-point slots of a resident batch before a tracking pass
 * (Frame::Frame leaves mvpMapPoints all NULL, src/Frame.cpp:99-102) without leaving the frame path's queue */
int cms_stream_copy_device(cms_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);
int cms_host_alloc(void** out, size_t bytes);   /* pinned host memory for cms_frames_upload_async */
void cms_host_free(void* p);
int cms_frames_process(cms_ctx* ctx, int B, int from_fisheye);
/* cms_frames_process(B, 1) on a batch that is already resident on the device, read IN PLACE: d_src has the staging layout [B][Ih][fisheye_stride]
 * (4-byte aligned; an allocation of exactly B * Ih * fisheye_stride bytes is enough, nothing behind it is read) and the remap is its only
 * reader.  Asynchronous on the ctx stream: the caller must not overwrite d_src until that launch has finished (cms_frames_sync, or an event
 * behind it).  The staging buffer of cms_frames_input / cms_frames_upload* is neither read nor written. */
int cms_frames_process_device(cms_ctx* ctx, const void* d_src, int B);
int cms_frames_sync(cms_ctx* ctx);
int cms_frames_results(cms_ctx* ctx, void** d_kps, void** d_desc, void** d_counts);
int cms_frames_fetch(cms_ctx* ctx, int b, cms_keypoint* kps, uint8_t* desc, int cap, int* n);

/* ---- the remap's 2-D tile table, host code only (no device is touched; cms_ctx_create builds the same table once per context).
 * cms_remap_lut_host  : the packed LUT, one u32 per canvas pixel, X[0:11) | Y[11:22) | ax[22:27) | ay[27:32); lut_stride (in entries) >= 3 face.
 *                       Cells the reference never writes (System.cpp:316-317) keep 0 == source pixel (0, 0) with weight 1.
 * cms_remap_tiles_host: one entry per tile_w x tile_h tile of the canvas (32 x 32, 64 x 16 or 128 x 8), live tiles first (*n_live), then the
 *                       tiles that lie wholly in the corner blocks (flag 2); *n_all entries in all, CMS_ERR_OVERFLOW if cap is too small.
 *                       (x0, y0) + (4 nd) x rows bytes = the source rectangle that covers the taps X .. X + 1, Y .. Y + 1 of every written
 *                       entry of the tile's cross pixels (nd = rows = 0: none); flag 1 = it exceeds lds_budget bytes for four frames and the
 *                       tile gathers from global memory.  *lds_bytes = the largest staged tile. */
typedef struct { uint16_t tx, ty, x0, y0, nd, rows, flags, pad; } cms_remap_tile;
int cms_remap_lut_host(const cms_camera* cam, uint32_t* lut, int lut_stride);
int cms_remap_tiles_host(const cms_camera* cam, const uint32_t* lut, int lut_stride, int tile_w, int tile_h, int lds_budget,
                         cms_remap_tile* out, int cap, int* n_live, int* n_all, int* lds_bytes);

/* ---- the FAST work lists, host code only (no device is touched; cms_ctx_create builds the same lists once per context).
 * which = 0: every cell the reference loop visits (ORBExtractor.cpp:764-781): the list of a caller-supplied canvas (cms_extract);
 *         1: without the cells that lie wholly in the zero corner blocks of a remapped cross;
 *         2: also without the cells whose whole ROI holds one value in every remapped frame -- corner blocks, or face pixels the reference never
 *            writes (LUT entry 0: the frame's pixel (0, 0)), followed down the pyramid through the resize tables: the list of a remapped batch.
 * Entries are level | row << 4 | column << 12 in the order k_fast_cells walks them.  *n = the list's length; cap = 0 only asks for it,
 * CMS_ERR_OVERFLOW if 0 < cap < *n. */
int cms_fast_cells_host(const cms_camera* cam, const cms_orb_params* orb, int which, int* out, int cap, int* n);

/* ---- stage-by-stage read-back for the parity tests */
int cms_debug_lut(cms_ctx* ctx, uint32_t* out, int* stride);
int cms_debug_cubemap(cms_ctx* ctx, int b, uint8_t* dst, int dstride);
int cms_debug_level(cms_ctx* ctx, int b, int level, uint8_t* dst, int dstride);
int cms_debug_candidates(cms_ctx* ctx, int b, int level, int* xys, int cap, int* n);   /* (x, y, score) rel. to minBorder, unordered */
int cms_debug_distributed(cms_ctx* ctx, int b, int level, int* xys, int cap, int* n);  /* octree output, list order, level coords */

/* ---- in-library stage timing with HIP events on the ctx stream (ms of the last cms_frames_process call)
 *      stages: 0 remap, 1 pyramid, 2 fast, 3 octree, 4 cull, 5 describe, 6 total */
int cms_profile_enable(cms_ctx* ctx, int on);
int cms_profile_get(cms_ctx* ctx, float* ms7);

/* ---- matching: ORBMatcher::DescriptorDistance (ORBMatcher.cpp:951-967) evaluated over the candidate list of every query
 *      (the inner loops of ORBMatcher::SearchByProjection, ORBMatcher.cpp:84-113 / 186-205).  Candidates are a CSR:
 *      query q scans cand_idx[cand_off[q] .. cand_off[q+1]).  t_excluded (optional) marks target key points that already
 *      hold a map point (ORBMatcher.cpp:91-95).  Outputs follow the sequential scan exactly (first minimum wins).
 *      The *_device variant takes device pointers and is asynchronous on the ctx stream; q_row (optional int[nq])
 *      gathers query q from row q_row[q] of qdesc, so one launch can match many frame pairs straight out of the
 *      extractor's descriptor buffer. */
int cms_hamming_best2(cms_ctx* ctx, const uint8_t* qdesc, int nq, const uint8_t* tdesc, int nt, const int* cand_off,
                      const int* cand_idx, const int* t_level, const uint8_t* t_excluded, int* best_idx, int* best_dist,
                      int* best_level, int* second_dist, int* second_level);
int cms_hamming_best2_device(cms_ctx* ctx, const void* qdesc, const void* q_row, int nq, const void* tdesc, const void* cand_off,
                             const void* cand_idx, const void* t_level, const void* t_excluded, void* best_idx,
                             void* best_dist, void* best_level, void* second_dist, void* second_level);
int cms_hamming_matrix(cms_ctx* ctx, const uint8_t* a, int na, const uint8_t* b, int nb, uint16_t* out);

/* ---- local bundle adjustment: numeric core of Optimizer::LocalBundleAdjustment (include/Optimizer.h:50,
 *      src/Optimizer.cpp:192-451) with EdgeSE3ProjectXYZMultiPinhole (include/g2o_cubemap_vertices_edges.h:90-134).
 *      The caller (the Optimizer mirror in cubemapslam_amd/host/) assembles the window exactly like Optimizer.cpp:194-357:
 *      poses K x 7 (tx,ty,tz,qx,qy,qz,qw; world->camera), fixed[K], points P x 3, and per observation: pose index,
 *      point index, measurement in the face, invSigma2 of the octave, face id.
 *      cms_ba_optimize runs optimize(its_robust) with Huber(sqrt(5.991)) -> chi2/depth classification ->
 *      optimize(its_final) on the inliers without kernel -> final classification (outlier_flags[e] = 1 to erase);
 *      *stop is polled between iterations like g2o's forceStopFlag (Optimizer.cpp:256-257): before anything is launched, then
 *      before every Levenberg trial the host enqueues.  With a stop pointer the grouped driver (optimize_many) queues a trial only
 *      after the previous one has finished, so a request raised mid-way takes effect at the next trial boundary -- where g2o's
 *      terminate() polls -- and the estimate left behind is the last accepted one, as with g2o. */
typedef struct cms_ba cms_ba;
typedef struct {
  int iterations_done[2];
  double chi2_initial[2], chi2_final[2], lambda_final[2];
  int n_outliers_mid, n_outliers_final;
} cms_ba_stats;
int cms_ba_create(cms_ba** out, int device, int K, const double* poses, const uint8_t* fixed, int P, const double* points,
                  int E, const int* e_pose, const int* e_point, const double* e_obs, const double* e_invsig2,
                  const int8_t* e_face, double fx, double fy, double cx, double cy);
/* The set-up of a window GROUP in one call (round 6): n windows as an array of descriptions (cms_ba_create's arguments).  The host parts run on up to
 * `threads` threads of the call (0: four), the set-up kernels of all device-planned windows are one launch per eight windows instead of one each --
 * a process that tracks many camera streams per GPU creates a group's sixteen windows per step (what Optimizer::LocalBundleAdjustment assembles once
 * per key frame, Optimizer.cpp:246-357).  On any error every window of the call is destroyed and out[] is all NULL.  The windows are independent
 * afterwards (cms_ba_set_stream, cms_ba_optimize_many, cms_ba_read / cms_ba_read_many, cms_ba_destroy each). */
typedef struct cms_ba_window {
  int K; const double* poses; const uint8_t* fixed; int P; const double* points; int E; const int* e_pose; const int* e_point;
  const double* e_obs; const double* e_invsig2; const int8_t* e_face; double fx, fy, cx, cy;
  int flags;      /* CMS_BA_INPUTS_PINNED | CMS_BA_PLAN_ON_DEVICE, or 0 */
} cms_ba_window;
/* flags: the window's observation-sized arrays (points, e_pose, e_point, e_obs, e_invsig2, e_face) lie in pinned host memory (cms_host_alloc, or registered with
 * the HIP runtime) and stay unchanged and alive until the window's first cms_ba_optimize* / cms_ba_read has returned or the window is destroyed: they are then
 * copied to the device from where they lie, asynchronously, instead of through the window's staging block -- a host that assembles a window's observations
 * (Optimizer.cpp:246-357) straight into pinned buffers saves one 3 MB memcpy per 80 k-observation window, as much host time as the window's whole plan. */
#define CMS_BA_INPUTS_PINNED 1
/* flags: the window's whole plan (signature groups, runs, internal point order, chunks, the left-over observations' diagonal copies) is made by a kernel
 * (k_ba_plan_many, one workgroup per window, launched per eight windows in front of their expansion) instead of by the calling threads; the call then waits
 * for those kernels (40 bytes of counts per window come back).  Same device arrays, byte for byte.  Worth it for a host short of cores -- the plan is
 * ~0.4 ms of a host thread per 80 k-observation window, half of what a two-core rank spends per step of bench.py; with cores to spare the host plan overlaps
 * the GPU better (bench.py sets the flag when its rank has at most two cores).  Windows the kernel does not take (a point seen twice by a key frame, no
 * signature runs, more than 64 key frames, CMS_BA_DET_POINTS windows) fall back to the host planners inside the call; an index out of range fails the call as ever. */
#define CMS_BA_PLAN_ON_DEVICE 2
int cms_ba_create_many(cms_ba** out, int n, int device, const cms_ba_window* windows, int threads);
/* ... and the read-back of n optimised windows (Optimizer.cpp:419-450): poses[i] / points[i] / outlier_flags[i] as cms_ba_read's (the arrays of
 * pointers, or single entries, may be NULL); one gather kernel per sixteen device-planned windows, one wait. */
int cms_ba_read_many(cms_ba** bas, int n, double** poses, double** points, uint8_t** outlier_flags);
int cms_ba_reset(cms_ba* ba);  /* restore the initial estimate on the device (benchmark loops) */
int cms_ba_optimize(cms_ba* ba, int its_robust, int its_final, const volatile uint8_t* stop, cms_ba_stats* stats);
/* n independent windows (e.g. the LocalMapping threads of n camera streams) advanced in lock-step by ONE host thread, each on
 * its own stream: same results as n cms_ba_optimize calls, without n host threads competing for the HIP runtime. stats[n]. */
int cms_ba_optimize_many(cms_ba** bas, int n, int its_robust, int its_final, const volatile uint8_t* stop, cms_ba_stats* stats);
/* ---- global bundle adjustment: numeric core of Optimizer::GlobalBundleAdjustemnt / Optimizer::BundleAdjustment (include/Optimizer.h,
 *      src/Optimizer.cpp:453-621) over the same window handle (the caller assembles the whole map as Optimizer.cpp:480-568 does).
 *      ONE SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg, exactly as one stage of the local BA runs it
 *      (lambda0 = 1e-5 max diag, the accept / reject rules, qmax == 10, rho == 0, nBad >= 3; *stop polled at the same places).
 *      robust != 0: Huber(sqrt(5.99)) on every edge -- BundleAdjustment's own text (:497); LocalBundleAdjustment writes 5.991 (:300) and
 *      cms_ba_optimize follows that.  robust == 0: no kernel.  No classification: no level is set, no outlier flag written; stats uses
 *      slot [0], everything else is zero.  *stop set on entry: nothing is enqueued, returns 1.  Defined for a window that has not been
 *      optimised since cms_ba_create / cms_ba_create_many / cms_ba_reset; any other window is CMS_ERR_ARG.  The _many form treats its
 *      windows as independent problems (grouped as cms_ba_optimize_many groups them), stats[n] in the caller's order.
 *      Windows whose reduced camera system (order 6 x free key frames) does not fit the LDS solves factor it with a tiled LDL^T over many
 *      workgroups (cms_ba_solve_tiled.hip) -- a dense factorisation in natural order where the reference runs Eigen's SimplicialLDLT under a
 *      fill-reducing ordering: the same factorisation in exact arithmetic, another rounding.  Up to order 16 384 (2 730 free key frames);
 *      beyond that CMS_ERR_UNSUPPORTED.  cms_ba_read / cms_ba_read_many return the estimate as ever. */
int cms_ba_optimize_global(cms_ba* ba, int iterations, int robust, const volatile uint8_t* stop, cms_ba_stats* stats);
int cms_ba_optimize_global_many(cms_ba** bas, int n, int iterations, int robust, const volatile uint8_t* stop, cms_ba_stats* stats);
/* developer entry: the tiled solve on its own.  A (n x n, row-major, host; only the lower triangle is read), b -> x, *status 1, or 0 with x = 0 after a
 * zero or non-finite pivot (no error code for that). */
int cms_ba_debug_solve_tiled(int device, int n, const double* A, const double* b, double* x, int* status);
/* ... and timed with HIP events over `reps` repetitions (*ms: mean milliseconds per solve; the matrix is restored on the device before each).
 * which: 0 the tiled solve, 1 k_ba_solve (the one-workgroup kernel of cms_ba_optimize's large windows; n <= 1024, beyond that CMS_ERR_UNSUPPORTED). */
int cms_ba_debug_solve_timed(int device, int which, int n, const double* A, const double* b, double* x, int* status, int reps, double* ms);
int cms_ba_read(cms_ba* ba, double* poses, double* points, uint8_t* outlier_flags);
void* cms_ba_stream(cms_ba* ba);
/* run this window on a stream the caller owns (shared by the windows of a group, or the mapping context's own stream): keeps the
 * number of streams of a process below the number of hardware queues */
int cms_ba_set_stream(cms_ba* ba, void* hip_stream);
/* developer aid: 100 MHz wall-clock stamps of the last single-window solve kernel (start, assembled, factorised, solved, end) */
int cms_ba_debug_clocks(cms_ba* ba, long long* out16);
/* measurement aid (bench.py's roofline of the dominant BA kernel): HIP events on the group's stream around ONE kernel of every round the
 * grouped driver enqueues for the group owned by `ba` (the first handle passed to cms_ba_optimize_many).  kernel_id: 0 off, 1 kb_ba_lin,
 * 2 kb_ba_maxdiag, 3 the Schur kernel of the path in use (kb_ba_lin_schur_edges by default: linearisation + Schur complement), 4 its range
 * reduction, 5 kb_ba_trial_solve3, 6 kb_ba_trial_edges, 7 kb_ba_reduce2.
 * cms_ba_profile_get returns the summed duration and the number of launches since cms_ba_profile_kernel was called. */
int cms_ba_profile_kernel(cms_ba* ba, int kernel_id);
int cms_ba_profile_get(cms_ba* ba, double* total_ms, long* launches);
/* developer / test aid, host only (no device needed): the chunk composition cms_ba_create builds for the edge-major Schur kernel -- which
 * points share a wavefront (<= 64 observations), in which order, and which copy of its key frame's diagonal block every observation adds
 * to -- chosen so that the lanes of one LDS addition fall on different banks.  lookahead <= 1: the caller's order.
 * pinv: P entries (internal point -> caller's point); chunk_pt0: room for P + 1, *n_chunks + 1 are written (first internal point of every
 * chunk, P last); rank (may be NULL): E entries, the caller's points in order, observations of a point by ascending key frame.
 * The graph itself is what Optimizer::LocalBundleAdjustment hands to g2o (Optimizer.cpp:192-363); the composition has no counterpart there. */
int cms_ba_debug_compose(int K, const uint8_t* fixed, int P, int E, const int* e_pose, const int* e_point, int lookahead,
                         int* pinv, int* chunk_pt0, int* n_chunks, uint8_t* rank);
/* developer / test aid, host only: the whole plan cms_ba_create makes for a window.  Points seen by the same set of key frames (one observation
 * signature) are grouped; a signature with enough points becomes a RUN whose chunks the run-major Schur kernel sums in registers
 * (cubemapslam_amd/csrc/cms_ba_schur_runs.hip), the rest are the composed chunks of cms_ba_debug_compose.  Outputs (upper-bound sizes): pinv P
 * (internal point -> caller's point), perm E (sorted edge -> caller's edge), info E (per-edge word of the kernels), chunk_pt0 P + 2, rm_chunk
 * 4 ints per run chunk (<= P), run_lane 128 u32 per run (<= P runs), run_mf 64 / run_fl 768 u32 per run (the MFMA variant's tables; may be
 * NULL), counts[8] = chunks, run chunks, runs, free key frames, points inside runs,
 * workgroups of a lone window for the run chunks / the left-over chunks, 1 if the window can use these kernels at all.  No counterpart in the
 * reference: the graph is what Optimizer::LocalBundleAdjustment hands to g2o (Optimizer.cpp:192-363). */
int cms_ba_debug_plan(int K, const uint8_t* fixed, int P, int E, const int* e_pose, const int* e_point, int* pinv, int* perm, uint32_t* info,
                      int* chunk_pt0, int* rm_chunk, uint32_t* run_lane, int* counts, uint32_t* run_mf, uint32_t* run_fl);
/* developer / test aid: the plan arrays as the DEVICE holds them for this window (after its set-up ran), whichever planner made them.  Since round 5
 * cms_ba_create plans most windows with one sequential pass over the observations on the host and per-point work only; the observation-sized
 * arrays (edge permutation, sorted edge arrays, per-edge words, diagonal copies, the runs' tables) are written by kernels
 * (cubemapslam_amd/csrc/cms_api_ba_plan.hip).  For the windows both planners take they give the same arrays: this entry is how the tests
 * compare them with cms_ba_debug_plan.  Sizes: pinv P, perm E, info E, pt_off P + 1, e_pose / e_point / e_face E, chunk_e0 chunks + 1, rm_chunk
 * 4 ints per run chunk, rm_cost chunks + 1, run_mf 64 / run_fl 768 words per run (any may be NULL); counts[8] as cms_ba_debug_plan's, with
 * counts[7] = 1 if the device-side planner made the window.  CMS_BA_HOST_PLAN=1 selects the host planner for every window (A/B). */
int cms_ba_debug_fetch_plan(cms_ba* ba, int* pinv, int* perm, uint32_t* info, int* pt_off, int* e_pose, int* e_point, int8_t* e_face, int* chunk_e0,
                            int* rm_chunk, uint32_t* rm_cost, uint32_t* run_mf, uint32_t* run_fl, int* counts);
/* ... and the same planner run entirely on the host (no device needed; the expansion kernels' bodies over host arrays): outputs as cms_ba_debug_plan's
 * (run_lane excepted); counts[7] = 0 when the window is not one the device-side planner takes (cms_ba_create then uses the host planner). */
int cms_ba_debug_plan_fast(int K, const uint8_t* fixed, int P, int E, const int* e_pose, const int* e_point, int* pinv, int* perm, uint32_t* info,
                           int* chunk_pt0, int* rm_chunk, int* counts, uint32_t* run_mf, uint32_t* run_fl);
/* developer / test aid, host only: the tables of the opt-in one-wavefront run workgroups (CMS_BA_RUN_WG=1, cubemapslam_amd/csrc/cms_ba_schur_runwg.hip:
 * round 6's re-decomposition of the Schur kernel, block_solver.hpp:367-437) as either planner makes them (fast != 0: the device-side planner's host
 * part).  run_fg: 64 x 24 words per run (per lane and MFMA accumulator its offset into the window's global copy of the reduced system, 0xFFFFFFFF: none),
 * rm_cut: 2 x 1025 cut points (per class of signature), counts[4] = runs (-1: the planner does not take the window), run chunks, class-0 run chunks,
 * free key frames. */
int cms_ba_debug_run_fg(int K, const uint8_t* fixed, int P, int E, const int* e_pose, const int* e_point, int fast, uint32_t* run_fg, int* rm_cut, int* counts);
/* developer / test entry, host only: the matching lanes -> copies of one group of 16 left-over observations (which = 0: the host planners' search, 1: the plan
 * kernel's register-only form of it -- the two must agree, tests/test_ba_plan_kernel_cpu.py); slots[n] = the lanes' free-pose slots, n <= 16 */
int cms_ba_debug_match(int which, int n, const int* slots, int np, int* choice_out);
void cms_ba_destroy(cms_ba* ba);
/* Device slabs and pinned blocks of destroyed windows wait in a per-device pool for the next window (CMS_BA_POOL_MB bounds the device part, default
 * 16384; the pool is also emptied and the allocation retried when hipMalloc fails).  cms_ba_pool_trim hands everything cached for `device` back
 * to the runtime -- for callers that share the device with other allocators; *released (may be NULL) receives the bytes. */
int cms_ba_pool_trim(int device, size_t* released);
/* Determinism as a product mode.  The reference optimises with a single-threaded g2o (ThirdParty/g2o/config.h:4: no OpenMP), so two runs on
 * the same window give the same bits.  The default device path adds with FP64 atomics (order varies from run to run: last bits differ, see
 * DESIGN.md section 2); cms_ba_set_deterministic(1) makes every window created AFTERWARDS add in a fixed order: the same kernels as the default
 * path with the Schur kernel's LDS additions performed in an order that follows from the window's plan alone (kb_ba_lin_schur_runs_det /
 * kb_ba_lin_schur_edges_det), the workgroups' sums kept as slices that the solve kernel adds in slice order instead of one global copy, and a cut
 * into workgroups that does not depend on the other windows of the call.  Same input, same bits: run after run, alone or in any group of a
 * cms_ba_optimize_many call, created by cms_ba_create or cms_ba_create_many (plan kernel included); bench.py's step runs at 0.84-0.87 of the default with
 * it (config.deterministic).  Windows the fused chain cannot take (more than 25 free key frames, a point seen twice by a key frame) run rounds 3-5's
 * pair-owner kernel (kb_ba_schur_points, CMS_BA_DET_POINTS=1 selects it for all) -- deterministic as well.  The choice is taken at cms_ba_create and
 * travels with the window; windows of both kinds may be passed to one cms_ba_optimize_many call (they run as separate groups).  Process-wide; the
 * environment variable CMS_BA_DETERMINISTIC=1 gives the initial value.  cms_ba_get_deterministic returns the current setting.
 * on >= 2 also says into how many workgroups such a window is cut (1: the default, 16 -- a group of sixteen windows fills the chip once; at most 128: a larger value is
 * clamped to 128 without an error, and cms_ba_get_deterministic then returns 128).  The count is
 * fixed when the window is created, because the bits depend on it.  A host that optimises ONE window per call (the reference's LocalMapping thread) should pass 64:
 * 2.4 instead of 3.5 ms per 80 k-observation window (default path 1.7 ms); sixteen windows in lock-step then take 6.1 instead of 4.8 ms. */
int cms_ba_set_deterministic(int on);
int cms_ba_get_deterministic(void);
/* one-shot convenience: create + optimize + read + destroy */
int cms_ba_run(int device, int K, double* poses, const uint8_t* fixed, int P, double* points, int E, const int* e_pose,
               const int* e_point, const double* e_obs, const double* e_invsig2, const int8_t* e_face, double fx, double fy,
               double cx, double cy, int its_robust, int its_final, const volatile uint8_t* stop, uint8_t* outlier_flags,
               cms_ba_stats* stats);
/* one linearisation at the given estimate (parity of the J^T J / J^T r build): Hpp K x 36, bp K x 6, Hll P x 9, bl P x 3,
 * Hpl E x 18 (caller's edge order), err E x 2, robust chi2 sum */
int cms_ba_linearize(int device, int K, const double* poses, const uint8_t* fixed, int P, const double* points, int E,
                     const int* e_pose, const int* e_point, const double* e_obs, const double* e_invsig2,
                     const int8_t* e_face, double fx, double fy, double cx, double cy, int robust, double huber_delta,
                     double* err, double* Hpp, double* bp, double* Hll, double* bl, double* Hpl, double* robust_chi2_sum);

/* ---- frame grid + window query: Frame::AssignFeaturesToGrid / PosInGrid (src/Frame.cpp:158-176, 728-744) and
 * Frame::GetFeaturesInArea with AddCells (src/Frame.cpp:36-72, 251-716), the step in front of every Hamming scan of
 * ORBMatcher::SearchByProjection / SearchForInitialization.  The reference's 41 window-unfolding cases (90 AddCells calls) are
 * reproduced literally (cubemapslam_amd/csrc/cms_area_table.h), so the candidate ORDER -- which decides Hamming ties -- is the
 * reference's.  cms_area_grid builds the 5 x 50 x 50 cell lists of frames 0..B-1 from the key points the last
 * cms_frames_process left on the device (or cms_area_set_keypoints put there); a query is (x, y, r, minLevel, maxLevel) in canvas
 * pixels; the result is a CSR list cand_off[nq+1] / cand_idx[] of key-point indices of frame b.  The _device variant takes and
 * returns device pointers (cnt_scratch: nq ints) and adds idx_base to every index, so the lists feed cms_hamming_best2_device
 * without touching the host. */
int cms_area_set_keypoints(cms_ctx* ctx, int b, int n, const cms_keypoint* kps);
int cms_area_grid(cms_ctx* ctx, int B);
int cms_features_in_area(cms_ctx* ctx, int b, int nq, const float* qx, const float* qy, const float* qr, const int* min_level,
                         const int* max_level, int* cand_off, int* cand_idx, int cap, int* total);
int cms_features_in_area_device(cms_ctx* ctx, int b, int nq, const void* d_qx, const void* d_qy, const void* d_qr, const void* d_min_level,
                                const void* d_max_level, void* d_cnt_scratch, void* d_cand_off, void* d_cand_idx, int cap, int idx_base,
                                void* d_total);
/* one launch sequence for a whole batch: d_qframe[q] names the frame (0 .. B-1 of cms_area_grid) query q searches; indices are batch rows */
int cms_features_in_area_batch_device(cms_ctx* ctx, int nq, const void* d_qframe, const void* d_qx, const void* d_qy, const void* d_qr,
                                      const void* d_min_level, const void* d_max_level, void* d_cnt_scratch, void* d_cand_off,
                                      void* d_cand_idx, int cap, void* d_total);

/* ---- track local map: Frame::isInFrustum (src/Frame.cpp:197-249, with MapPoint::PredictScale, src/MapPoint.cpp:404-419, and
 * Get{Min,Max}DistanceInvariance :375-385) for every local map point, then ORBMatcher::SearchByProjection(Frame&, const
 * vector<MapPoint*>&, th) (src/ORBMatcher.cpp:50-128, RadiusByViewingCos :380-386) -- the pair Tracking::SearchLocalPoints
 * (src/Tracking.cpp:794-846) runs per frame with viewingCosLimit 0.5, ORBMatcher(0.8), th 1 (5 after a relocalisation).
 *   pose15      Rcw (9 floats, row major) | tcw (3) | Ow (3): Frame::mRcw / mtcw / mOw as Frame::UpdatePoseMatrices leaves them
 *   pos, normal MapPoint::mWorldPos / mNormalVector (3 floats each); min_dist / max_dist = mfMinDistance / mfMaxDistance
 *   outputs     in_view = mbTrackInView, proj_x/y = mTrackProjX/Y (-1 when not in view), level = mnTrackScaleLevel, view_cos
 * The reference's matching loop is sequential -- a key point taken by one map point is skipped by all later ones -- and the
 * device reproduces exactly that result (cms_track_kernels.hip explains how).  kp_mp holds one int per key point: >= 0 on entry
 * means "already holds a map point with observations" (ORBMatcher.cpp:91-93); a new match stores the map point's list index.
 * cms_search_local_points is the one-frame entry with host buffers: frame b's key points/descriptors are the ones the last
 * cms_frames_process left on the device, or cms_area_set_keypoints + cms_area_set_descriptors put there (cms_area_grid first).
 * The _device entries take device pointers, work on all frames of a batch at once and are asynchronous on the ctx stream:
 * cms_is_in_frustum_device also writes the window of every point (qr < 0: not in view) for cms_features_in_area_batch_device;
 * cms_search_local_points_device takes that CSR (indices = batch rows), mp_off[B+1] (map points grouped by frame, list order
 * inside a frame), scratch pair_dist (2 bytes per candidate) and kp_mp over all batch rows; mp_match = batch row or -1.
 * Limit: at most 4096 key points per frame for the greedy projection searches (CMS_ERR_UNSUPPORTED; the frame grid itself and
 * cms_search_for_initialization take up to 16383, i.e. the 3 x nFeatures extractor); any number of map points per frame (a thread of the greedy kernel
 * takes every 1024th point of its frame). */
int cms_area_set_descriptors(cms_ctx* ctx, int b, int n, const uint8_t* desc);
/* What the caller hands over as min_dist / max_dist of a map point (cms_search_local_points, cms_is_in_frustum_device, cms_fuse_search,
 * cms_kfstore_fuse_search, cms_search_by_projection_keyframe and, for the frame context, cms_kfstore_search_by_projection of this context): scaled = 0 (default) MapPoint::mfMinDistance / mfMaxDistance themselves -- private members, a binding
 * needs two one-line accessors; scaled = 1 the public MapPoint::GetMinDistanceInvariance() / GetMaxDistanceInvariance() (src/MapPoint.cpp:375-385:
 * 0.8f / 1.2f already applied), so that the reference's headers stay byte-identical.  With scaled = 1 the bounds of Frame::isInFrustum / Fuse
 * are exactly the getters' values; mfMaxDistance (the numerator of MapPoint::PredictScale, :387-419) is recovered as the float r with
 * 1.2f * r == bound -- where the product crossed a power of two, two neighbouring r share a bound and the smaller is taken: the predicted
 * level can then differ from the reference only if log(ratio) / log(scale factor) sits within an ulp of an integer. */
int cms_set_distance_bounds_mode(cms_ctx* ctx, int scaled);
/* ORBMatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono) (src/ORBMatcher.cpp:130-251), the matcher of
 * Tracking::TrackWithMotionModel, whole on the device: the last frame's map points are projected with the current pose (Rcw | tcw of
 * CurrentFrame.mTcw; z < cosFovTh and UNKNOWN_FACE are dropped), windows th * scale[octave] over octave -1 .. +1, greedy best match
 * <= TH_HIGH (a key point taken by one map point is skipped by the later ones), then the rotation-consistency histogram
 * (ComputeThreeMaxima, :905-946).  valid[i]: key point i of the last frame holds a map point and is not an outlier.  kp_mp as in
 * cms_search_local_points.  The _device entries are the batched pieces: cms_project_last_frame_device writes the windows of all
 * queries (q_frame = current frame each one searches), cms_features_in_area_batch_device and cms_search_local_points_device
 * (nnratio < 0: no second-best test) follow, cms_rotation_filter_device applies the histogram per frame and counts the matches. */
int cms_search_by_projection(cms_ctx* ctx, int b, const float* pose12, int nlast, const uint8_t* valid, const float* Xw, const int* octave,
                             const float* angle, const uint8_t* mp_desc, float th, int check_orientation, int th_high, int nkp, int* kp_mp,
                             int* match, int* n_matches);
/* ORBMatcher::SearchForInitialization(Frame& F1, Frame& F2, vector<cv::Point2f>& vbPrevMatched, vector<int>& vnMatches12, int windowSize)
 * (include/ORBMatcher.h:58, src/ORBMatcher.cpp:676-794), the matcher of Tracking::MonocularInitialization (Tracking.cpp:428-429:
 * ORBMatcher(0.9, true), window 100).  F2 = frame slot b2 on the device (cms_area_grid first), F1 = the caller's key points and
 * descriptors.  Level-0 key points of F1 only; a key point of F2 is taken over by a later strictly better match; rotation histogram
 * over every accepted match; prev_matched (n1 x 2 floats = vbPrevMatched) is updated for the matched key points. */
int cms_search_for_initialization(cms_ctx* ctx, int b2, int n1, const cms_keypoint* kps1, const uint8_t* desc1, float* prev_matched,
                                  int window_size, float nnratio, int check_orientation, int* matches12, int* n_matches);
int cms_project_last_frame_device(cms_ctx* ctx, int n, const void* d_qframe, const void* d_pose12, const void* d_valid, const void* d_Xw,
                                  const void* d_oct, float th, void* d_qx, void* d_qy, void* d_qr, void* d_qmin, void* d_qmax);
int cms_rotation_filter_device(cms_ctx* ctx, int B, const void* d_mp_off, const void* d_last_angle, void* d_kp_mp, void* d_mp_match,
                               void* d_n_matches, int check_orientation);
int cms_search_local_points(cms_ctx* ctx, int b, const float* pose15, int nmp, const float* pos, const float* normal,
                            const float* min_dist, const float* max_dist, const uint8_t* mp_desc, float viewing_cos_limit, float th,
                            float nnratio, int th_high, int nkp, int* kp_mp, uint8_t* in_view, float* proj_x, float* proj_y, int* level,
                            float* view_cos, int* mp_match, int* n_matches, int* rounds);
int cms_is_in_frustum_device(cms_ctx* ctx, int nmp, const void* d_mp_frame, const void* d_pose15, const void* d_pos, const void* d_normal,
                             const void* d_min_dist, const void* d_max_dist, float viewing_cos_limit, float th, void* d_in_view,
                             void* d_proj_x, void* d_proj_y, void* d_level, void* d_view_cos, void* d_qr, void* d_qmin, void* d_qmax);
int cms_search_local_points_device(cms_ctx* ctx, int B, const void* d_mp_off, const void* d_mp_desc, const void* d_cand_off,
                                   const void* d_cand_idx, void* d_pair_dist, float nnratio, int th_high, void* d_kp_mp, void* d_mp_match,
                                   void* d_rounds);

/* ---- mapping thread, either side of the local BA.
 * cms_create_new_map_points: numeric core of LocalMapping::CreateNewMapPoints (src/LocalMapping.cpp:209-386, bearing-vector version):
 * for every neighbour of a current key frame, in the order given (GetBestCovisibilityKeyFrames), the baseline test (:238-247),
 * ComputeE12 (:469-482), ORBMatcher::SearchForTriangulation (src/ORBMatcher.cpp:971-1125; CheckDistEpipolarLine :388-407,
 * CamModelGeneral::GetVectorSigma src/CamModelGeneral.cpp:307-333) and the triangulation of every match on its key rays with all of
 * the reference's tests (:266-357).  A feature triangulated with one neighbour is taken for the following ones, as
 * KeyFrame::AddMapPoint makes it.  njobs current key frames (independent maps / streams) are ONE launch.
 *   cms_keyframe   what these functions read of a KeyFrame: mvKeys, mDescriptors, mvKeyRays, mp[i] >= 0 <=> GetMapPoint(i) != NULL,
 *                  GetRotation / GetTranslation / GetCameraCenter (float), mFeatVec as CSR (node ids ascending; DBoW2 is only
 *                  needed to produce it), ComputeSceneMedianDepth(2)
 *   neigh_off      njobs + 1 offsets into neigh[]
 *   outputs        n_new[j]; records j * cap_per_job + k, k < n_new[j], in creation order: neighbour index (within job j),
 *                  idx1, idx2, x3D.  check_orientation = ORBMatcher's mbCheckOrientation (false at this call site, :217).
 * cms_fuse_search: search half of ORBMatcher::Fuse(pKF, vpMapPoints, th) (src/ORBMatcher.cpp:1127-1226) against key-frame slot b
 * (cms_area_set_keypoints + cms_area_set_descriptors + cms_area_grid first): projection, image / distance / viewing-angle tests,
 * PredictScale, KeyFrame::GetFeaturesInArea(u, v, th * scale), level and reprojection gates, Hamming minimum <= TH_LOW.
 * skip[i] != 0 <=> !pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF).  best_idx[i] = key point to fuse with or -1; the Replace /
 * AddObservation bookkeeping (:1216-1241) stays with the caller, in list order. */
typedef struct {
  int n; const cms_keypoint* kps; const uint8_t* desc; const float* rays; const int* mp;
  float Rcw[9], tcw[3], Ow[3];
  int nnodes; const int* node_id; const int* node_off; const int* node_feat;
  float median_depth;
} cms_keyframe;
int cms_create_new_map_points(cms_ctx* ctx, int njobs, const cms_keyframe* cur, const int* neigh_off, const cms_keyframe* neigh,
                              int check_orientation, int cap_per_job, int* n_new, int* out_neigh, int* out_idx1, int* out_idx2,
                              float* out_x3d);
/* ORBMatcher::SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, cv::Mat E12, vector<pair<size_t, size_t>>& vMatchedPairs) (include/ORBMatcher.h:61,
 * src/ORBMatcher.cpp:971-1125) on its own -- the call of LocalMapping.cpp:254 for callers that triangulate themselves: for every feature of kf1
 * without a map point, the best feature of kf2 (same vocabulary node, no map point, Hamming <= TH_LOW, away from the epipole, inside the
 * epipolar gate), then the rotation histogram if check_orientation.  E12: the 3 x 3 essential matrix the caller computed (row major), NULL =
 * LocalMapping::ComputeE12 of the two poses.  matches12[i1] = index in kf2 or -1 (kf1->n entries); *n_matches = their number. */
int cms_search_for_triangulation(cms_ctx* ctx, const cms_keyframe* kf1, const cms_keyframe* kf2, const float* E12, int check_orientation,
                                 int* matches12, int* n_matches);
/* Resident key frames: the map's key frames stay on the device in fixed-size slots, a CreateNewMapPoints call names slots and only
 * ~100 bytes per (current, neighbour) pair travel.  cms_kfstore_put uploads / replaces a key frame; cms_kfstore_update refreshes what
 * changes between calls (pose after a local BA, median depth, map-point slots; NULL = unchanged).  Results as above. */
typedef struct cms_kfstore cms_kfstore;
int cms_kfstore_create(cms_kfstore** out, cms_ctx* ctx, int max_keyframes, int max_features, int max_nodes);
void cms_kfstore_destroy(cms_kfstore* st);
int cms_kfstore_put(cms_kfstore* st, int slot, const cms_keyframe* kf);
int cms_kfstore_update(cms_kfstore* st, int slot, const float* Rcw, const float* tcw, const float* Ow, const float* median_depth, const int* mp);
/* LocalMapping::ProcessNewKeyFrame's device half (src/LocalMapping.cpp:52-117: the frame Tracking turned into a key frame enters the map): the key
 * points, descriptors, key rays (Frame::mvKeyRays) and the frame grid of frame b of `src`'s last batch are already on the device (cms_frames_process
 * + cms_area_grid left them there); one kernel copies them device to device into `slot` -- no trip through the host, no second grid build, no
 * synchronisation -- and reads what only the host has from a pinned block: the FeatureVector (KeyFrame::ComputeBoW, DBoW2 on the host) and the
 * map-point slots mp[n] (NULL: none).  n = the frame's key-point count (what cms_frames_fetch reports).  Asynchronous: the copy is enqueued on `src`'s
 * stream -- behind the work that produced frame b and in front of the next batch, like the KeyFrame constructor's copy on the Tracking thread
 * (Tracking.cpp:1015-1017) -- and the store's stream waits for it on the device; `src` may be the store's own context.  Equivalent to cms_kfstore_put of the
 * fetched frame (tests/test_gpu_parity.py::test_kfstore_put_from_frame_equals_put). */
int cms_kfstore_put_from_frame(cms_kfstore* st, int slot, cms_ctx* src, int b, int n, const float* Rcw, const float* tcw, const float* Ow, float median_depth,
                               const int* mp, int nnodes, const int* node_id, const int* node_off, const int* node_feat);
/* ... several key frames of one batch in one call (one per camera stream and step when a process tracks many streams per GPU) */
typedef struct {
  int slot, b, n;
  const float* Rcw; const float* tcw; const float* Ow; float median_depth;
  const int* mp; int nnodes; const int* node_id; const int* node_off; const int* node_feat;
} cms_kf_from_frame;
int cms_kfstore_put_from_frames(cms_kfstore* st, cms_ctx* src, int n_items, const cms_kf_from_frame* items);
/* the poses of n resident key frames after a local BA (Optimizer.cpp:419-431 writes them back into the KeyFrames): Rcw n x 9, tcw n x 3, Ow n x 3.
 * One kernel reading a pinned block, asynchronous -- cms_kfstore_update per key frame costs a copy and a stream wait each. */
int cms_kfstore_update_poses(cms_kfstore* st, int n, const int* slots, const float* Rcw, const float* tcw, const float* Ow);
/* developer / test aid: what a slot holds on the device (any pointer may be NULL): kps / desc / rays / mp / feat_node / sorted n entries (n = header[1]),
 * node_id nnodes, node_off nnodes + 1, node_feat node_off[nnodes], cell_start 5 x 50 x 50 + 1, header = the slot's 21-word record (f0, n, node0, nnodes,
 * noff0, nfeat0, Rcw, tcw, Ow), misc[2] = valid grid entries, stored key-point count */
int cms_kfstore_debug_fetch(cms_kfstore* st, int slot, cms_keypoint* kps, uint8_t* desc, float* rays, int* mp, int* feat_node, uint16_t* sorted,
                            int* node_id, int* node_off, int* node_feat, int* cell_start, uint32_t* header, int* misc);
/* SearchInNeighbors' Fuse calls (src/LocalMapping.cpp:388-467) on resident key frames in one launch sequence: job j searches the map points
 * [mp_off[j], mp_off[j+1]) of the concatenated host arrays in the key frame of slot job_slot[j]; arguments and results as cms_fuse_search. */
int cms_kfstore_fuse_search(cms_kfstore* st, int njobs, const int* job_slot, const int* mp_off, const uint8_t* skip, const float* pos,
                            const float* normal, const float* min_dist, const float* max_dist, const uint8_t* mp_desc, float th, int* best_idx,
                            int* best_dist);
/* SearchInNeighbors' shape (src/LocalMapping.cpp:388-466): one key frame's map points go into each of its ~20 neighbours, so the same positions /
 * normals / descriptors would travel 20 times.  Here they are uploaded ONCE as sets: set s = map points set_off[s] .. set_off[s + 1] of pos / normal /
 * min_dist / max_dist / mp_desc; job j searches key frame slot job_slot[j] with set job_set[j].  skip (may be NULL), best_idx, best_dist are per
 * ENTRY: job after job, a job's entries in the order of its set.  Results as cms_kfstore_fuse_search's. */
int cms_kfstore_fuse_search_sets(cms_kfstore* st, int nsets, const int* set_off, const float* pos, const float* normal, const float* min_dist,
                                 const float* max_dist, const uint8_t* mp_desc, int njobs, const int* job_slot, const int* job_set, const uint8_t* skip,
                                 float th, int* best_idx, int* best_dist);
int cms_kfstore_create_new_map_points(cms_kfstore* st, int njobs, const int* cur_slot, const int* neigh_off, const int* neigh_slot,
                                      int check_orientation, int cap_per_job, int* n_new, int* out_neigh, int* out_idx1, int* out_idx2,
                                      float* out_x3d);
/* Per-map-point bookkeeping the mapping thread runs over the points it created, fused or optimised, batched:
 * MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cpp:243-308): obs_off[npts+1] into the concatenated descriptors of each
 * point's non-bad observations (std::map order); best_idx[p] = the observation whose descriptor has the least median distance to the
 * rest (first on ties), -1 without observations.  MapPoint::UpdateNormalAndDepth (:332-373): obs_Ow = camera centres of the observing
 * key frames (same order), ref_Ow / ref_level = centre of mpRefKF and octave of its observation; normal / min_dist / max_dist are
 * in/out (points without observations stay untouched). */
int cms_distinctive_descriptors(cms_ctx* ctx, int npts, const int* obs_off, const uint8_t* desc, int* best_idx);
int cms_update_normal_and_depth(cms_ctx* ctx, int npts, const int* obs_off, const float* pos, const float* obs_Ow, const float* ref_Ow,
                                const int* ref_level, float* normal, float* min_dist, float* max_dist);
int cms_fuse_search(cms_ctx* ctx, int b, const float* pose15, int nmp, const uint8_t* skip, const float* pos, const float* normal,
                    const float* min_dist, const float* max_dist, const uint8_t* mp_desc, float th, int* best_idx, int* best_dist);

/* ---- ORBMatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches) (include/ORBMatcher.h:67, src/ORBMatcher.cpp:409-539),
 * the matcher of Tracking::TrackReferenceKeyFrame (Tracking.cpp:567-618, ORBMatcher(0.7, true)) and of Tracking::Relocalization's candidate loop
 * (:995-1040, ORBMatcher(0.75, true)).  Only vocabulary nodes present in both FeatureVectors take part, in ascending id order; per common node the
 * key frame's features with a map point (mp >= 0) that is not bad (kf_skip == NULL or kf_skip[i] == 0: pMP->isBad()) are taken in list order, each
 * against the node's frame features not matched yet (best < second best, both from 256; best <= TH_LOW and (float)best < nnratio * (float)second);
 * then the rotation histogram when check_orientation (HISTO_LENGTH 12, ComputeThreeMaxima).  kf_idx[i] (one per frame key point) = the key-frame
 * feature whose map point frame key point i receives, or -1: the caller maps it to its MapPoint*.  *n_matches = nmatches after the histogram.
 * The frame's FeatureVector (Frame::ComputeBoW, DBoW2 on the host) comes as CSR like cms_keyframe's; a feature listed twice in it, node ids that
 * do not ascend or an index >= n are CMS_ERR_ARG.  The frame is row b of the context's last batch: the key points and descriptors cms_frames_process
 * left on the device, or cms_area_set_keypoints + cms_area_set_descriptors put there.  Limits: n <= 16383 (the frame grid's CMS_AREA_MAXKP), key
 * frames up to 4096 features (stand-alone) or the store's max_features (resident); more is CMS_ERR_UNSUPPORTED.  Synchronous: Tracking decides on
 * nmatches at once.
 * cms_search_by_bow: the key frame from the host (cms_keyframe as for cms_search_for_triangulation; rays and pose are not read), on ctx's stream. */
int cms_search_by_bow(cms_ctx* ctx, int b, int n, int nnodes, const int* node_id, const int* node_off, const int* node_feat,
                      const cms_keyframe* kf, const uint8_t* kf_skip, float nnratio, int check_orientation,
                      int* kf_idx /* n */, int* n_matches);
/* cms_kfstore_search_by_bow: resident key frames, many jobs, ONE launch (Relocalization's candidate loop, or one TrackReferenceKeyFrame per camera
 * stream).  A key-frame feature has a map point where the slot's mp (as put / updated) is >= 0.  Runs on src's stream -- the frame thread's -- and
 * enqueues nothing on the store's: src's stream waits on the device for the copies of cms_kfstore_put_from_frame(s) that filled the named slots.
 * Threading: the call may run on the frame thread while the mapping thread uses the store, provided no concurrent call refills, updates or
 * releases a slot that the search names. */
typedef struct {
  int slot;                 /* key frame: store slot */
  int b, n;                 /* frame: row b of src's last batch, n key points */
  int nnodes; const int* node_id; const int* node_off; const int* node_feat;   /* Frame::ComputeBoW output, CSR */
  const uint8_t* kf_skip;   /* NULL, or one byte per key-frame feature: != 0 <=> pMP->isBad() */
} cms_bow_job;
int cms_kfstore_search_by_bow(cms_kfstore* st, cms_ctx* src, int njobs, const cms_bow_job* jobs, float nnratio,
                              int check_orientation, int* kf_idx /* sum of jobs[j].n, job after job */, int* n_matches /* njobs */);

/* ---- ORBMatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12) (include/ORBMatcher.h:68, src/ORBMatcher.cpp:541-674),
 * the matcher of LoopClosing::ComputeSim3 (LoopClosing.cpp:251-279, ORBMatcher(0.75, true), once per loop candidate), between cms_kfdb_detect and
 * cms_sim3_iterate, on resident key frames: all candidates of a pass in ONE launch.  A contract of its own, not cms_kfstore_search_by_bow with other
 * parameters: only vocabulary nodes present in both FeatureVectors take part, in ascending id order; per common node key frame 1's features with a
 * map point (the slot's mp >= 0) that is not bad (skip1) are taken in list order, each against the node's key-frame-2 features that are not taken
 * yet (vbMatched2), hold a map point and are not bad (skip2) -- a feature filtered this way is neither best nor second best; best < second best,
 * both from 256, the first minimum in list order wins; accepted when best < TH_LOW (50, strict) and (float)best < nnratio * (float)second (one float
 * multiply); then the rotation histogram over angle1 - angle2 when check_orientation (HISTO_LENGTH 12, ComputeThreeMaxima).  idx2[i] (one per key
 * point of key frame 1) = the key-frame-2 feature whose map point it receives, or -1: the caller maps it to its MapPoint*.  *n_matches = nmatches
 * after the histogram.  Malformed FeatureVectors (the store accepts any CSR): an entry of a node's list takes part only if that node is the one the
 * slot's feat_node records for the feature (the last entry that lists it), and a feature of key frame 1 that holds a match is not matched again.
 * For every FeatureVector DBoW2 produces this changes nothing; for one that lists a feature twice the result is defined by the store's contents.
 * Runs on src's stream -- the loop-closing thread's -- and enqueues nothing on the store's: src's stream waits on the device for the copies of
 * cms_kfstore_put_from_frame(s) that filled the named slots.  Synchronous: the caller decides on nmatches < 20 at once.  One copy up (skip flags, job
 * records), one launch, one copy back.  Checked before anything is enqueued, CMS_ERR_ARG with the reason in cms_last_error: a slot out of range or not
 * filled, n1 / n2 that is not the slot's stored key-point count, a context on another device than the store's.  njobs == 0 is CMS_OK with no launch;
 * slot1 == slot2 is allowed (the search only reads the store); a slot without nodes gives zero matches.  Threading as cms_kfstore_search_by_bow: no
 * concurrent call refills, updates or releases a slot that the search names. */
typedef struct {
  int slot1, n1;            /* mpCurrentKF: store slot and its stored key-point count */
  int slot2, n2;            /* the candidate */
  const uint8_t* skip1;     /* NULL, or n1 bytes: != 0 <=> pMP->isBad() */
  const uint8_t* skip2;     /* NULL, or n2 bytes */
} cms_bow_kf_job;
int cms_kfstore_search_by_bow_keyframes(cms_kfstore* st, cms_ctx* src, int njobs, const cms_bow_kf_job* jobs,
                                        float nnratio, int check_orientation,
                                        int* idx2 /* sum of n1, job after job */, int* n_matches /* njobs */);

/* ---- Frame::ComputeBoW (src/Frame.cpp:719-726; Tracking.cpp:570, :993) and KeyFrame::ComputeBoW (src/KeyFrame.cpp:94-103; LocalMapping.cpp:142,
 * Tracking.cpp:472-473): mpORBvocabulary->transform(descriptors, mBowVec, mFeatVec, 4) (DBoW2 TemplatedVocabulary.h:1127-1259) on the device, so that
 * SearchByBoW and CreateNewMapPoints take the FeatureVector from where the descriptors already are.  The numeric definition is csrc/cms_vocab_core.h
 * (one source for the host build and the kernels); every output is bit-equal to the host build's: word ids ascending with their double values,
 * node ids ascending, a node's features in feature order.  A feature whose word has weight <= 0 enters neither vector.  A descent that ends on a leaf
 * above level L - levelsup reports that leaf as the feature's node (the reference leaves the id unset).
 *
 * cms_vocab: the tree on one device, read-only after creation, shared by any number of contexts and stores of that device.  The arrays are the text
 * format's (loadFromTextFile, :1338-1424): node 0 is the root (its entries are not read), node i > 0 has parent[i] < i, is_leaf[i] != 0 marks a word, word
 * ids count the leaves in node order, children are in ascending node id, desc is n_nodes x 32 bytes, weight n_nodes doubles.  CMS_ERR_ARG (with the
 * reason in cms_last_error) for k outside 0..20, L outside 1..10, scoring outside 0..5, weighting outside 0..3, a parent id that is not smaller than the
 * node's own, a leaf with children, an inner node without, more than k children, no words, or more than 2^21 nodes.
 * cms_vocab_info: info[7] = k, L, scoring, weighting, nodes, words, device. */
typedef struct cms_vocab cms_vocab;
int cms_vocab_create(cms_vocab** out, int device, int k, int L, int scoring, int weighting, int n_nodes, const int* parent, const uint8_t* is_leaf,
                     const uint8_t* desc, const double* weight);
void cms_vocab_destroy(cms_vocab* v);
int cms_vocab_info(const cms_vocab* v, int* info);
/* Developer aid (tools/prof_bow_transform.py), one thread at a time: while on, every ComputeBoW call of the process records events around its two
 * launches; after the call cms_vocab_profile_get gives ms2[0] = k_vocab_descend and ms2[1] = k_vocab_build of the last one. */
int cms_vocab_profile_enable(int on);
int cms_vocab_profile_get(float* ms2);
/* Stand-alone: n descriptors from the host (n x 32 bytes, n <= 16383: more is CMS_ERR_UNSUPPORTED), on ctx's stream.  word_id / word_val / node_id /
 * node_feat hold up to n entries, node_off n + 1; node_off[*nnodes] is the number of features listed.  levelsup >= 0. */
int cms_vocab_transform(cms_vocab* v, cms_ctx* ctx, int n, const uint8_t* desc, int levelsup, int* nwords, int* word_id, double* word_val, int* nnodes,
                        int* node_id, int* node_off, int* node_feat);
/* Frame rows rows[i] of ctx (n[i] key points each, as cms_frames_fetch reports them), all in one launch sequence on ctx's stream; the descriptors
 * are read where cms_frames_process (or cms_area_set_descriptors) left them and the results stay resident per row until the next batch is processed.  Synchronous: the call
 * returns with the rows' counts known to the host.  A row named twice, a count beyond the row or a vocabulary on another device is CMS_ERR_ARG. */
int cms_frames_compute_bow(cms_ctx* ctx, cms_vocab* v, int levelsup, int n_rows, const int* rows, const int* n);
/* What the host needs for mBowVec, mFeatVec and KeyFrameDatabase.  *nwords / *nnodes are always delivered; a capacity that cannot hold its array
 * (node_off needs node_cap + 1 entries, node_feat up to the row's key-point count) makes the call CMS_ERR_OVERFLOW with nothing copied.  A row without
 * a computed BoW is CMS_ERR_ARG. */
int cms_frames_fetch_bow(cms_ctx* ctx, int b, int* nwords, int* word_id, double* word_val, int word_cap, int* nnodes, int* node_id, int* node_off,
                         int* node_feat, int node_cap, int feat_cap);
/* KeyFrame::ComputeBoW on the resident descriptors of the named slots: writes feat_node / node_feat / node_id / node_off and the record's node count
 * in the slot's layout -- after cms_kfstore_put_from_frames(... nnodes = 0 ...) and this call a slot is byte-identical to one put with the
 * host-computed FeatureVector -- and keeps the BowVector per slot (cms_kfstore_fetch_bow).  On the store's stream, synchronous.  If any slot's
 * FeatureVector has more nodes than the store's max_nodes the call is CMS_ERR_OVERFLOW and NO slot is changed. */
int cms_kfstore_compute_bow(cms_kfstore* st, cms_vocab* v, int levelsup, int n_slots, const int* slots);
/* The slot's BowVector and, when node_off is not NULL, its FeatureVector (nnodes may be NULL), with capacities as cms_frames_fetch_bow.  A slot that
 * was refilled (cms_kfstore_put / put_from_frame(s)) since its last cms_kfstore_compute_bow has no BowVector: CMS_ERR_ARG. */
int cms_kfstore_fetch_bow(cms_kfstore* st, int slot, int* nwords, int* word_id, double* word_val, int word_cap, int* nnodes, int* node_id, int* node_off,
                          int* node_feat, int node_cap, int feat_cap);
/* cms_kfstore_search_by_bow with the frame side's FeatureVector taken from the row's resident result (cms_frames_compute_bow): the jobs' nnodes /
 * node_id / node_off / node_feat are not read.  A row without a computed BoW, or one computed for another n, is CMS_ERR_ARG. */
int cms_kfstore_search_by_bow_frames(cms_kfstore* st, cms_ctx* src, int njobs, const cms_bow_job* jobs, float nnratio, int check_orientation,
                                     int* kf_idx, int* n_matches);

/* ---- KeyFrameDatabase (src/KeyFrameDatabase.cpp) over the resident key frames of a store: DetectRelocalizationCandidates (:204-314; Tracking.cpp:997)
 * and DetectLoopCandidates (:81-202; LoopClosing.cpp:140) on the device, between cms_frames_compute_bow and cms_kfstore_search_by_bow_frames, so that
 * Relocalization's chain never fetches a BowVector.  The numeric definition is csrc/cms_kfdb_core.h (one source for the host build and the kernels);
 * candidates, common-word counts and scores are bit-equal to the host build's.  Scoring is L1 (ScoringObject.cpp:23-68), the reference's; there is no
 * other.
 *
 * An entry is a slot with a BowVector, a group >= 0 (one per map or camera stream: a query sees its own group only), its add order, a persistent
 * reloc_score (KeyFrame::mRelocScore; 0.0f from add on, where the reference reads an uninitialised float) and up to 10 covisible slots.
 * lKFsSharingWords is ordered by (smallest common word id, add order) -- the order in which the reference meets the key frames in its inverted
 * file -- and the candidates come back as a subsequence of it.  Several jobs of one call are evaluated as if one after the other in job order.
 *
 * Threading: cms_kfdb_add / erase / clear / set_covisibles touch a host table under the database's mutex and enqueue nothing; the mapping thread may
 * call them while the frame thread is in cms_kfdb_detect, which takes its snapshot under the same mutex.  Calls of cms_kfdb_detect on one store
 * are serialised. */
/* cms_kfstore_set_bow: the BowVector the host computed for the key frame in `slot` (KeyFrame::mBowVec; cms_kfstore_compute_bow gives a slot its own).
 * Ids >= 0 and strictly ascending, at most max_features entries, the slot filled and not in the database: otherwise CMS_ERR_ARG and the slot is
 * unchanged.  On the store's stream, synchronous. */
int cms_kfstore_set_bow(cms_kfstore* st, int slot, int nwords, const int* word_id, const double* word_val);
/* KeyFrameDatabase::add (:45-51; LoopClosing.cpp:115, :145, :214), erase (:53-72; KeyFrame.cpp:569) and clear (:74-78; Tracking.cpp:1176; group -1:
 * every group).  add of a slot without a BowVector, in the database already or named twice is CMS_ERR_ARG and adds none; erase of a slot that is not
 * in it does nothing, as in the reference; erase + add moves an entry to the back of the add order and zeroes its reloc_score.  A slot that is
 * refilled (cms_kfstore_put / put_from_frame(s)) leaves the database and loses its covisibles: both belonged to the key frame it held. */
int cms_kfdb_add(cms_kfstore* st, int n, const int* slots, const int* groups);
int cms_kfdb_erase(cms_kfstore* st, int n, const int* slots);
int cms_kfdb_clear(cms_kfstore* st, int group);
/* pKF->GetBestCovisibilityKeyFrames(10) (:156, :270) per named slot as slots: neigh holds n x 10, best first, padded with -1.  A covisible that is not
 * in the database, or not in the query's group, contributes nothing. */
int cms_kfdb_set_covisibles(cms_kfstore* st, int n, const int* slots, const int* neigh);
#define CMS_KFDB_RELOC 0
#define CMS_KFDB_LOOP 1
#define CMS_KFDB_QUERY_ROW 0     /* row b of src's last batch, its resident BowVector (cms_frames_compute_bow) */
#define CMS_KFDB_QUERY_SLOT 1    /* the BowVector of a store slot (DetectLoopCandidates' pKF) */
#define CMS_KFDB_QUERY_WORDS 2   /* nwords / word_id / word_val from the host: ids >= 0, strictly ascending, at most 16383 */
typedef struct cms_kfdb_job {
  int mode, group, query;
  int b, slot;
  int nwords; const int* word_id; const double* word_val;
  float min_score; int n_connected; const int* connected;      /* LOOP: minScore and the slots of pKF->GetConnectedKeyFrames() (:83) */
} cms_kfdb_job;
/* One upload, one launch sequence on src's stream -- the frame thread's, under the rules of cms_kfstore_search_by_bow: nothing is enqueued on the
 * store's stream -- one copy back, one wait.  cand_slot receives njobs x cand_cap slots, n_cand[j] is always delivered; a job with more candidates than
 * cand_cap makes the call CMS_ERR_OVERFLOW (the first cand_cap are delivered).  diag_common / diag_score may be NULL; otherwise njobs x max_keyframes
 * each: common words per slot, and `float si` with -1 where the slot was not scored.  RELOC: every scored entry's reloc_score is overwritten; a
 * covisible that shares a word with the query adds its reloc_score (:278-286) -- the one an EARLIER query left if it fell under this query's
 * threshold.  LOOP: connected slots never enter the list; an entry below min_score is left out but still adds to a neighbour's sum (:164-171);
 * bestAccScore starts at min_score.  CMS_ERR_ARG: a row without a computed BoW, an empty slot or one without a BowVector, unsorted words, a store on
 * another device than src.  More than 16384 key frames in the database is CMS_ERR_UNSUPPORTED. */
int cms_kfdb_detect(cms_kfstore* st, cms_ctx* src, int njobs, const cms_kfdb_job* jobs, int cand_cap, int* cand_slot, int* n_cand, int* diag_common,
                    float* diag_score);
/* The score() loop of LoopClosing::DetectLoop (LoopClosing.cpp:125-138): score[i] = mpORBVocabulary->score(BowVec of slot_a[i], BowVec of slot_b[i]), the
 * same ordered sum as a double.  On the store's stream, synchronous. */
int cms_kfstore_bow_score(cms_kfstore* st, int npairs, const int* slot_a, const int* slot_b, double* score);
/* Developer aid (tools/prof_kfdb.py), one thread at a time: while on, every cms_kfdb_detect records events around its launch sequence; after the call
 * cms_kfdb_profile_get gives its milliseconds. */
int cms_kfdb_profile_enable(int on);
int cms_kfdb_profile_get(float* ms);

/* ---- ORBMatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, const float th, const int ORBdist)
 * (include/ORBMatcher.h:64, src/ORBMatcher.cpp:253-378), the guided search of Tracking::Relocalization: twice per accepted PnP pose
 * (src/Tracking.cpp:1101 with th 10 / ORBdist 100, :1115 with th 3 / ORBdist 64), between the PoseOptimization calls (cms_pose_*) and behind the candidate
 * loop (cms_kfstore_search_by_bow).  The caller lists, in the order of pKF->GetMapPointMatches() (:268-276), the key frame's map points that are non-NULL,
 * not bad and not in sAlreadyFound: kf_feat (their key-frame feature indices, strictly ascending -- the order decides the greedy), pos = GetWorldPos(),
 * min_dist / max_dist as cms_set_distance_bounds_mode says (default: mfMinDistance / mfMaxDistance), mp_desc = GetDescriptor().  Per listed point:
 * x3Dc = Rcw*x3Dw+tcw; dropped when zc < cosFovTh, on UNKNOWN_FACE, or when dist3D = norm(x3Dw - Ow) is outside the invariance bounds (there is no
 * viewing-angle test and no image-bounds test); PredictScale; window th * mvScaleFactors[level] over levels level - 1 .. level + 1; candidates in
 * GetFeaturesInArea's order, key points with kp_mp >= 0 skipped (CurrentFrame.mvpMapPoints[i2] != NULL: ANY map point, no Observations() test), first
 * strict minimum, accepted when bestDist <= ORBdist (no second-best test); an accepted key point is taken for all later entries; then the rotation
 * histogram over pKF->mvKeys[i].angle - CurrentFrame.mvKeys[bestIdx2].angle when check_orientation (ComputeThreeMaxima, :905-946).
 * pose12 = Rcw (9 floats, row major) | tcw (3) of CurrentFrame.mTcw.  Ow is derived from it on the device exactly as :259 does (-Rcw.t()*tcw: cv::gemm
 * with a transposed operand accumulates in double and rounds once) -- the caller hands no camera centre over.
 * kp_mp: one int per key point of the frame, in/out: >= 0 on entry <=> CurrentFrame.mvpMapPoints[i] != NULL; a new match stores the index into the
 * job's list; a match the histogram removes is back to -1.  n (nkp) is the row's key-point count: key points of the row from n on count as free, and a
 * match with one of them is reported in match[] but has no entry in kp_mp.  match[k] = frame key point of listed point k or -1 (after the histogram); n_matches =
 * nmatches as returned by the reference.  The frame is row b of the context's last batch (cms_frames_process, or cms_area_set_keypoints +
 * cms_area_set_descriptors; cms_area_grid first).  Limit: kp_cap <= 4096 as for the sibling greedy searches (CMS_ERR_UNSUPPORTED); any number of
 * listed points.  Synchronous: Tracking decides on nGood + nadditional at once.
 * cms_kfstore_search_by_projection: resident key frames, many (key frame, frame) pairs -- one lost camera stream each -- as ONE launch sequence on
 * src's stream: one upload, projection, window query, greedy, histogram, one read-back.  The slot supplies mvKeys[].angle and the feature count.
 * Two jobs naming the same frame row are CMS_ERR_ARG (the reference's second call sees the first one's matches and another pose), so are kf_feat that
 * do not strictly ascend or reach the slot's feature count.  nmp == 0: zero matches, kp_mp untouched.  Stream rule as cms_kfstore_search_by_bow:
 * nothing is enqueued on the store's stream; src's stream waits on the device for the cms_kfstore_put_from_frame(s) copies that filled the named slots.
 * cms_search_by_projection_keyframe: one pair with a key frame that is not resident; kf_angle[k] = pKF->mvKeys[kf_feat[k]].angle from the caller. */
typedef struct {
  int slot;                  /* resident key frame */
  int b, n;                  /* frame: row b of src's last batch, n key points */
  float pose12[12];          /* Rcw | tcw of CurrentFrame.mTcw */
  int nmp;                   /* listed map points */
  const int* kf_feat;        /* nmp key-frame feature indices, strictly ascending */
  const float* pos; const float* min_dist; const float* max_dist; const uint8_t* mp_desc;   /* per listed point (pos: 3 floats, mp_desc: 32 bytes) */
  int* kp_mp;                /* n ints, in/out */
  int* match;                /* nmp ints, out */
} cms_kfproj_job;
int cms_kfstore_search_by_projection(cms_kfstore* st, cms_ctx* src, int njobs, const cms_kfproj_job* jobs, float th, int orb_dist,
                                     int check_orientation, int* n_matches /* njobs */);
int cms_search_by_projection_keyframe(cms_ctx* ctx, int b, const float* pose12, int nmp, const float* kf_angle, const float* pos,
                                      const float* min_dist, const float* max_dist, const uint8_t* mp_desc, float th, int orb_dist,
                                      int check_orientation, int nkp, int* kp_mp, int* match, int* n_matches);

/* ---- PnPsolver (include/PnPsolver.h, src/PnPsolver.cpp), the EPnP RANSAC of Tracking::Relocalization (src/Tracking.cpp:1034-1060), between
 * cms_kfstore_search_by_bow and cms_pose_optimize.  The result of a four-point EPnP is defined by the SVD that picks a basis of MtM's null space
 * (DESIGN.md "PnPsolver"), so the definition of record is the project's own core, csrc/cms_pnp_core.h: one source, built for the host
 * (libcubemapslam_host.so: hm_pnp_iterate_host) and for the device, which is held to the host build bit for bit.
 * cms_pnp_ransac_parameters: SetRansacParameters (:123-159) without the per-point part: int truncation of N*epsilon (float product), the two lower
 *   bounds, epsilon raised to min_inliers/N (float), nIterations = 1 if min_inliers == N else ceil(log(1-p)/log(1-pow(epsilon,3))) in double (a value
 *   no int holds -- NaN for N < minSet -- converts as x86 does, to INT_MIN), max_its = max(1, min(nIterations, maxIterations)).  Host only.
 * cms_pnp_iterate: PnPsolver::iterate (:167-261) with Refine (:263-309) and CheckInliers (:312-343) for njobs solvers -- one lost camera stream and
 *   candidate key frame each -- as ONE launch sequence on the handle's stream: one pinned block up, every hypothesis of every job in parallel
 *   (compute_pose on the four drawn points), one wavefront per hypothesis for CheckInliers, then one workgroup per job replays the loop in order
 *   (best on >, Refine on the best mask, accepted on > min_inliers, exhaustion), one block back.  Synchronous: Tracking decides on the result at once.
 *   Per job the call may need H = max(max_its - iterations, n_iterations) hypotheses if N >= min_inliers, else 0 (the `while` of :184); the caller
 *   makes the 4*H draws beforehand: draws[4*i + k] = the k-th DUtils::Random::RandomInt(0, size - 1) of iteration i, so 0 <= draws[4*i+k] <= N-1-k.
 *   The contract is "the reference's loop on the same draws": when a call ends early the draws behind the accepting iteration are discarded, and the
 *   process's rand() stream is further along than the reference's would be.
 *   status: 1 = Refine accepted (Tcw = mRefinedTcw, inliers = mvbRefinedInliers, n_inliers = mnRefinedInliers), 2 = iterations used up with a best
 *   (Tcw = mBestTcw, inliers = mvbBestInliers), 0 = empty cv::Mat (Tcw and inliers zeroed).  no_more = bNoMore.  iterations_run = nCurrentIterations.
 *   iterations / best_inliers / best_Tcw / best_mask carry mnIterations / mnBestInliers / mBestTcw / mvbBestInliers from call to call; a new solver
 *   starts with zeros.  Tcw = R (9, row major) | t (3), floats converted from double per element.  inliers / best_mask are per correspondence; the
 *   caller expands them through mvKeyPointIndices.
 *   Checked before anything is enqueued (CMS_ERR_ARG): draws out of range, n_draws < 4*H, a total of correspondences / hypotheses / jobs above what
 *   cms_pnp_create was given, best_mask not consistent with best_inliers, min_inliers < 4 (SetRansacParameters never gives it), max_its or n_iterations
 *   outside [0, 2^20].  min_set != 4 is CMS_ERR_UNSUPPORTED (the reference passes no other value).
 *   ctx supplies the face size F and the device; nothing is enqueued on its stream.
 * cms_pnp_iterate_frames: the same, with the 2-D side of every correspondence gathered on the device from the context's resident rows instead of
 *   travelling from the host: correspondence i of a job is key point kp_idx[i] (mvKeyPointIndices) of row b of ctx's last batch (cms_frames_process /
 *   cms_extract), n = the row's key-point count as the caller fetched it: mvP2D = mvKeys[kp_idx[i]].pt, mvBearings = the key ray (what
 *   cms_frames_fetch_rays reads), mvSigma2 = mvLevelSigma2[octave].  p2d / bearing / sigma2 are ignored.  kp_idx outside [0, n), n above the context's
 *   kp_cap or b beyond its batch are CMS_ERR_ARG.  The whole sequence runs on ctx's stream, behind whatever filled the rows (the rule of
 *   cms_kfstore_search_by_projection); one caller at a time per context and per handle.  Synchronous. */
int cms_pnp_ransac_parameters(int N, double probability, int minInliers, int maxIterations, int minSet, float epsilon,
                              int* min_inliers, int* max_its, float* epsilon_out);
typedef struct cms_pnp cms_pnp;
int cms_pnp_create(cms_pnp** out, int device, int max_jobs, int max_corr_total, int max_hyp_total);
void cms_pnp_destroy(cms_pnp* p);
typedef struct {
  int N;                      /* correspondences (PnPsolver ctor order: key points with a map point that is not bad) */
  const float* p3d;           /* N x 3  mvP3Dw */
  const float* p2d;           /* N x 2  mvP2D   | cms_pnp_iterate_frames: ignored, gathered from the frame row */
  const float* bearing;       /* N x 3  mvBearings = mvKeyRays | same */
  const float* sigma2;        /* N      mvSigma2 (mvLevelSigma2[octave]) | same */
  const int* kp_idx;          /* cms_pnp_iterate_frames only: mvKeyPointIndices (N) */
  int b, n;                   /* cms_pnp_iterate_frames only: row b of ctx's last batch, n key points */
  float th2; int min_inliers, max_its, min_set;
  int n_iterations;           /* iterate()'s argument */
  int n_draws; const int* draws;   /* successive DUtils::Random::RandomInt(0, size-1) values, four per iteration */
  int iterations, best_inliers; float best_Tcw[12]; uint8_t* best_mask;   /* in/out: mnIterations, mnBestInliers, mBestTcw (R row major | t), mvbBestInliers (N bytes) */
  int status, no_more, n_inliers, iterations_run; float Tcw[12]; uint8_t* inliers;   /* out; inliers: N bytes, by correspondence */
} cms_pnp_job;
int cms_pnp_iterate(cms_pnp* p, cms_ctx* ctx /* F */, int njobs, cms_pnp_job* jobs);
int cms_pnp_iterate_frames(cms_pnp* p, cms_ctx* ctx, int njobs, cms_pnp_job* jobs);

/* ---- Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cpp), the Horn RANSAC of LoopClosing::ComputeSim3 (src/LoopClosing.cpp:287-345), behind
 * cms_kfdb_detect.  cv::eigen and cv::Rodrigues are not in the tree and libm's atan2 / sin / cos differ from the device's in ulps (DESIGN.md
 * "Sim3Solver"), so the definition of record is the project's own core, csrc/cms_sim3_core.h: one source, built for the host
 * (libcubemapslam_host.so: hm_sim3_iterate_host) and for the device, which is held to the host build bit for bit.
 * cms_sim3_ransac_parameters: SetRansacParameters (:138-162): epsilon = (float)minInliers / N, nIterations = 1 if minInliers == N else
 *   ceil(log(1-p)/log(1-pow(epsilon,3))) in double (a value no int holds -- NaN, or inf for N = 0 -- converts as x86 does, to INT_MIN),
 *   max_its = max(1, min(nIterations, maxIterations)).  Host only.
 * cms_sim3_iterate: Sim3Solver::iterate (:164-231) with ComputeSim3 (:250-361) and CheckInliers (:364-394) for njobs solvers -- one loop candidate
 *   each -- as ONE launch sequence on the handle's stream: one pinned block up, one wavefront per hypothesis (the Horn solve on the three drawn
 *   pairs, then the two-way inlier test over the correspondences), one wavefront per job replaying the loop in order (best on >=, accepted on
 *   > min_inliers), one block back.  Synchronous.  ctx supplies the face size F and the device; nothing is enqueued on its stream.
 *   x3dc1 / x3dc2 are mvX3Dc1 / mvX3Dc2: the matched map points in the frames of key frame 1 and 2, in the constructor's order (:66-127), both
 *   projecting into a face; max_err1 / max_err2 are mvnMaxError1 / 2 = (float)(9.210 * sigma2).  mvP1im1 / mvP2im2 are computed inside the call.
 *   The loop is `while (mnIterations < max_its && nCurrentIterations < n_iterations)`, so a call evaluates at most
 *   min(max_its - iterations, n_iterations) hypotheses.  The caller makes the draws beforehand, three per iteration: draws[3*i + k] = the k-th
 *   DUtils::Random::RandomInt(0, size - 1) of iteration i, so 0 <= draws[3*i+k] <= N-1-k.  The call asks for 3*H of them with
 *   H = max(max_its - iterations, n_iterations) if N >= min_inliers, else 0, and checks all of them; draws behind the last iteration run are discarded.
 *   status: 1 = a hypothesis with more than min_inliers inliers that is the best so far (T12 = mBestT12, rows 0..2 of the 4 x 4 [sR | t] row
 *   major; inliers = its mask; n_inliers), 0 = empty cv::Mat (T12 and inliers zeroed).  no_more = bNoMore.  iterations_run = nCurrentIterations.
 *   iterations / best_inliers / best_R / best_t / best_s / best_T12 / best_mask carry mnIterations / mnBestInliers / mBestRotation /
 *   mBestTranslation / mBestScale / mBestT12 / mvbBestInliers from call to call; a new solver starts with zeros.  N < min_inliers gives no_more
 *   and touches nothing else.  inliers / best_mask are per correspondence; the caller expands them through mvnIndices1.
 *   Checked before anything is enqueued (CMS_ERR_ARG, the records untouched): a draw out of range, n_draws < 3*H, a total of jobs /
 *   correspondences / hypotheses above what cms_sim3_create was given, best_mask not consistent with best_inliers, min_inliers < 3,
 *   max_its or n_iterations outside [0, 2^20], a null array.  One caller at a time per handle. */
int cms_sim3_ransac_parameters(int N, double probability, int minInliers, int maxIterations, int* max_its);
typedef struct cms_sim3 cms_sim3;
int cms_sim3_create(cms_sim3** out, int device, int max_jobs, int max_corr_total, int max_hyp_total);
void cms_sim3_destroy(cms_sim3* p);
typedef struct {
  int N;                      /* correspondences (Sim3Solver ctor order) */
  const float* x3dc1;         /* N x 3  mvX3Dc1 */
  const float* x3dc2;         /* N x 3  mvX3Dc2 */
  const float* max_err1;      /* N      mvnMaxError1 */
  const float* max_err2;      /* N      mvnMaxError2 */
  int fix_scale, min_inliers, max_its;
  int n_iterations;           /* iterate()'s argument */
  int n_draws; const int* draws;   /* successive DUtils::Random::RandomInt(0, size-1) values, three per iteration */
  int iterations, best_inliers; float best_R[9], best_t[3], best_s, best_T12[12]; uint8_t* best_mask;   /* in/out */
  int status, no_more, n_inliers, iterations_run; float T12[12]; uint8_t* inliers;   /* out; inliers: N bytes, by correspondence */
} cms_sim3_job;
int cms_sim3_iterate(cms_sim3* p, cms_ctx* ctx /* F */, int njobs, cms_sim3_job* jobs);

/* ---- ORBMatcher::SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12, s12, R12, t12, th) (include/ORBMatcher.h,
 * src/ORBMatcher.cpp:1365-1586), the guided matcher LoopClosing::ComputeSim3 runs on every hypothesis Sim3Solver::iterate accepts
 * (src/LoopClosing.cpp:312-322, th = 7.5), behind cms_sim3_iterate, on resident key frames: every accepted hypothesis of a pass in ONE call.
 * Per job: sR12 = s12*R12, sR21 = (1.0/s12)*R12.t(), t21 = -sR21*t12 (:1377-1379; csrc/cms_sim3_search_core.h states the arithmetic).  Direction
 * 1 -> 2 (:1406-1484), per key point i1 of key frame 1 with skip == 0: p3Dc2 = sR21*(R1w*p3Dw + t1w) + t21, dropped on z < 0, projected
 * (TransformRaysToCubemap), dropped outside [0, 3F)^2, dist3D = norm(p3Dc2) against the point's scale-invariance distances, PredictScale, window
 * th * mvScaleFactors[level] in key frame 2 (GetFeaturesInArea without level arguments, its order), candidates of octave level - 1 or level, first
 * strict Hamming minimum from INT_MAX, accepted when <= TH_HIGH (100).  No viewing-angle test, no reprojection gate, no taken flag.  Direction 2 -> 1
 * (:1487-1565) mirrors it with sR12 | t12 into key frame 1.  z_as_written != 0: the depth handed to the projection of direction 2 -> 1 is
 * component 1, line :1507 as the reference has it (`z = p3Dc1.at<float>(1)`); 0: component 2, upstream ORB-SLAM2's text.  The depth test and the norm
 * use the true vector either way.  Agreement (:1567-1583): idx2[i1] = vnMatch1[i1] where vnMatch2[vnMatch1[i1]] == i1, else -1; n_found = their number.
 * One stated difference: a ray no face takes (UNKNOWN_FACE) makes the reference's assert abort; here u = v = -1 and the point is dropped.
 * The poses R1w | t1w, R2w | t2w are the slots' own (cms_kfstore_put*, cms_kfstore_update_poses).  The store holds no world positions, so the map
 * points travel, as for cms_kfstore_fuse_search: record off1 + i1 of the n_mp-long arrays belongs to key point i1 of key frame 1, off2 + i2 to key
 * point i2 of key frame 2.  skip != 0 <=> !pMP || vbAlreadyMatched[i] || pMP->isBad() (the pointer work of :1390-1400 is the caller's); pos, min_dist,
 * max_dist (as src's cms_set_distance_bounds_mode says) and mp_desc are read only where skip == 0.  A job's records are key frame 1's, then key
 * frame 2's, and the jobs' records follow each other in call order: off1 >= the end of the job before, off2 >= off1 + n1, off2 + n2 <= n_mp.
 * idx2: job after job, n1 entries each; n_found[njobs].  Both may be pageable or pinned host memory.
 * Runs on src's stream with src's staging block -- the loop-closing thread's -- and enqueues nothing on the store's: src's stream waits on the
 * device for the copies of cms_kfstore_put_from_frame(s) that filled the named slots.  Four launches (projection, window query, scan, agreement), one
 * synchronisation; a call whose candidate lists did not fit is repeated once with room for them.  Synchronous.  Checked before anything is enqueued,
 * CMS_ERR_ARG with the reason in cms_last_error: a slot out of range or not filled, n1 / n2 that is not the slot's stored key-point count, offsets
 * that do not ascend or reach beyond n_mp, s12 zero or not finite, th negative or not finite, more than 16 levels, a context on another device
 * than the store's.  njobs == 0 is CMS_OK with no launch; n1 == 0 or n2 == 0 gives zero matches; slot1 == slot2 is allowed.  Threading as
 * cms_kfstore_search_by_bow_keyframes. */
typedef struct {
  int slot1, n1, slot2, n2;     /* resident key frames (mpCurrentKF, pKF) and their stored key-point counts */
  float s12, R12[9], t12[3];    /* Sim3Solver::GetEstimatedScale / Rotation (row major) / Translation */
  int off1, off2;               /* first entry of key frame 1's / 2's per-key-point map-point records in the arrays below */
} cms_sim3_search_job;
int cms_kfstore_search_by_sim3(cms_kfstore* st, cms_ctx* src, int njobs, const cms_sim3_search_job* jobs, int n_mp,
                               const uint8_t* skip, const float* pos, const float* min_dist, const float* max_dist, const uint8_t* mp_desc,
                               float th, int z_as_written, int* idx2, int* n_found);

/* ---- The two projection matchers of a loop closure that see a key frame through a similarity Scw instead of its stored pose, on resident key frames:
 *   ORBMatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, vpPoints, vpMatched, th) (src/ORBMatcher.cpp:796-903), the last step of
 *     LoopClosing::ComputeSim3 (src/LoopClosing.cpp:374, th = 10), whose count decides "loop accepted";
 *   the search half of ORBMatcher::Fuse(KeyFrame* pKF, cv::Mat Scw, vpPoints, th, vpReplacePoint) (:1246-1363), which LoopClosing::SearchAndFuse
 *     (src/LoopClosing.cpp:586-612, th = 4) runs once per key frame of CorrectedPosesMap over the same loop map points.
 * Sets of map points are shared between jobs as in cms_kfstore_fuse_search_sets: set s holds records [set_off[s], set_off[s + 1]) of pos (3 floats),
 * normal (3), min_dist, max_dist (as src's cms_set_distance_bounds_mode says) and mp_desc (32 bytes).  A job searches its set in its slot's key frame
 * under its own Scw; its ENTRIES are the set's points in order, job after job.  skip (per entry, may be NULL) != 0 <=> pMP->isBad() ||
 * spAlreadyFound.count(pMP) (:817, :1268; the pointer work of :806-807 / :1256 is the caller's).
 * Per job Scw is decomposed (:799-803; csrc/cms_sim3_proj_core.h states the arithmetic): scw = sqrt(row0 . row0), Rcw = sRcw / scw, tcw = t / scw,
 * Ow = -Rcw.t() * tcw.  Per entry (:817-860 / :1268-1312): p3Dc = Rcw*p3Dw + tcw, dropped on z < 0, projected (TransformRaysToCubemap), dropped outside
 * [0, 3F)^2, dist = norm(p3Dw - Ow) against the point's scale-invariance distances, PO.dot(Pn) < 0.5*dist dropped, PredictScale, window
 * th * mvScaleFactors[level] (GetFeaturesInArea without level arguments, its order), candidates of octave level - 1 or level.  The slot's stored pose
 * is not read.  One stated difference: a ray no face takes (UNKNOWN_FACE) makes the reference's assert abort; here u = v = -1 and the point is dropped.
 *   SearchByProjection (:870-898): candidates with vpMatched[idx] != NULL are passed over -- those of `taken` (per job n bytes, job after job; read,
 *     never written) and those an earlier entry of the same job took; first strict Hamming minimum from 256, accepted when <= TH_LOW (50).
 *     match_kp[entry] = the key point taken or -1, n_matches[job] = nmatches.  The store's max_features must not exceed 4096 (CMS_ERR_ARG).
 *   Fuse (:1323-1345): no taken test and, unlike cms_kfstore_fuse_search, no reprojection gate; first strict minimum, accepted when <= TH_LOW.
 *     best_idx[entry] = bestIdx or -1, best_dist[entry] = bestDist or 256.  What is done with bestIdx (:1347-1358) is the caller's.
 * Both run on src's stream with src's staging block -- the loop-closing thread's -- and enqueue nothing on the store's: src's stream waits on the
 * device for the copies of cms_kfstore_put_from_frame(s) that filled the named slots.  One synchronisation; a call whose candidate lists did not fit
 * is repeated once with room for them.  Synchronous; results may be pageable or pinned host memory; a repeated call gives identical bytes.  Checked
 * before anything is enqueued or written, CMS_ERR_ARG with the reason in cms_last_error: a slot out of range or not filled, n that is not the slot's
 * stored key-point count, a set out of range, set offsets that do not ascend, scw zero or not finite or a non-finite Scw entry, th negative or not
 * finite, more than 16 levels, a context on another device than the store's, a null array where entries exist.  njobs == 0 is CMS_OK with no
 * launch; an empty set or n == 0 gives no match.  Threading as cms_kfstore_search_by_sim3.
 * cms_sim3_proj_last_rounds: the most rounds a job of the calling thread's last cms_kfstore_search_by_projection_sim3 needed (for profiles). */
typedef struct {
  int slot, n;        /* resident key frame and its stored key-point count */
  float Scw[12];      /* rows 0..2 of the 4 x 4 [sR | t], row major, float (mScw / Converter::toCvMat(g2oScw)) */
  int set;            /* which map-point set the job searches */
} cms_sim3_proj_job;
int cms_kfstore_search_by_projection_sim3(cms_kfstore* st, cms_ctx* src, int nsets, const int* set_off, const float* pos, const float* normal,
                                          const float* min_dist, const float* max_dist, const uint8_t* mp_desc, int njobs, const cms_sim3_proj_job* jobs,
                                          const uint8_t* skip, const uint8_t* taken, float th, int* match_kp, int* n_matches);
int cms_kfstore_fuse_search_sim3(cms_kfstore* st, cms_ctx* src, int nsets, const int* set_off, const float* pos, const float* normal,
                                 const float* min_dist, const float* max_dist, const uint8_t* mp_desc, int njobs, const cms_sim3_proj_job* jobs,
                                 const uint8_t* skip, float th, int* best_idx, int* best_dist);
int cms_sim3_proj_last_rounds(void);

/* ---- Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) (src/Optimizer.cpp:888-1091), which LoopClosing::ComputeSim3 runs on
 * every hypothesis behind cms_kfstore_search_by_sim3 (src/LoopClosing.cpp:324-326; the candidate is kept on >= 20 inliers): every accepted hypothesis
 * of a pass as ONE launch, one workgroup per job with both optimize() rounds, the Levenberg accept / reject loop and the two classifications inside
 * the kernel.  g2o is not in the tree and libm's exp / sin / cos differ from the device's in ulps, so the definition of record is the project's own
 * core, csrc/cms_sim3_opt_core.h (DESIGN.md "OptimizeSim3"): one source, built for the host (libcubemapslam_host.so: hm_sim3_optimize_host) and for
 * the device, which is held to the host build bit for bit.
 *   The graph (:939-1028): per kept correspondence k the fixed points x3dc1[k] = R1w*P3D1w + t1w and x3dc2[k] = R2w*P3D2w + t2w (float, widened),
 *   e12 = EdgeSim3ProjectXYZMultiPinhole with obs kp1[k] (face = FaceInCubemap, _measurementInFace = GetPosInFace in double, information =
 *   inv_sigma2_1[k] * I), e21 = EdgeInverseSim3ProjectXYZMultiPinhole with kp2[k] / inv_sigma2_2[k]; Huber on both with delta = (float)sqrt(th2).
 *   The pointer work of :941-978 (!pMP1 || !pMP2, isBad, GetIndexInKeyFrame < 0) is the caller's: the N records are the correspondences the loop
 *   keeps, in key-point order of key frame 1.  The start is Sim3(R12, t12, s12) as :324 builds gScm.
 *   optimize(5); pairs with chi2_12 > th2 || chi2_21 > th2 go (keep[k] = 0 <=> vpMatches1[idx] = NULL); fewer than 10 left: n_inliers = 0 and the
 *   Sim3 out is the start (:1061); else optimize(nBad > 0 ? 10 : 5), the final classification, n_inliers = nIn.  Huber stays on in both rounds.
 *   jacobian: CMS_SIM3_OPT_AS_WRITTEN (0) -- both edges have linearizeOplus commented out, so g2o differentiates them numerically with delta = 1e-9
 *   through a projection that returns float: the Jacobian is almost entirely exact zeros, and the call is mostly an inlier filter around the start.
 *   CMS_SIM3_OPT_ANALYTIC (1): the analytic derivative of the double projection; errors and chi2 go through the float projection either way.
 *   Out: n_inliers (the reference's return value), keep (N bytes), q12 (x y z w) | t12_out | s12_out = the optimised g2oS12, n_correspondences (= N),
 *   n_bad (the first classification's), iterations[2] = Levenberg iterations run by the two optimize() calls.
 *   Synchronous; one launch sequence per call on the handle's stream: one pinned block up, one launch, one block back.  ctx supplies the face size
 *   F and the device; nothing is enqueued on its stream.  Checked before anything is enqueued (CMS_ERR_ARG, the reason in cms_last_error, the
 *   records untouched): a null array, more jobs / correspondences than cms_sim3_opt_create was given, th2 or s12 not finite or <= 0, jacobian
 *   outside {0, 1}, a context on another device, a key point that lies in no face -- one stated difference: the reference's computeError calls
 *   exit() there.  njobs == 0 is CMS_OK with no launch; N == 0 returns 0 inliers.  One caller at a time per handle. */
#define CMS_SIM3_OPT_AS_WRITTEN 0
#define CMS_SIM3_OPT_ANALYTIC 1
typedef struct cms_sim3_opt cms_sim3_opt;
int cms_sim3_opt_create(cms_sim3_opt** out, int device, int max_jobs, int max_corr_total);
void cms_sim3_opt_destroy(cms_sim3_opt* p);
typedef struct {
  int N;                        /* kept correspondences, in key-point order of key frame 1 */
  const float* x3dc1;           /* N x 3  P3D1c */
  const float* x3dc2;           /* N x 3  P3D2c */
  const float* kp1;             /* N x 2  pKF1->mvKeys[i].pt, cubemap image coordinates */
  const float* kp2;             /* N x 2  pKF2->mvKeys[i2].pt */
  const float* inv_sigma2_1;    /* N      pKF1->mvInvLevelSigma2[kp1.octave] */
  const float* inv_sigma2_2;    /* N      pKF2->mvInvLevelSigma2[kp2.octave] */
  double R12[9], t12[3], s12;   /* the start: Sim3Solver's estimate, R row major */
  float th2; int fix_scale, jacobian;
  int n_inliers; uint8_t* keep; double q12[4], t12_out[3], s12_out; int n_correspondences, n_bad, iterations[2];   /* out */
} cms_sim3_opt_job;
int cms_sim3_optimize(cms_sim3_opt* p, cms_ctx* ctx /* F */, int njobs, cms_sim3_opt_job* jobs);

/* ---- Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale)
 * (src/Optimizer.cpp:623-886), the Sim3 pose graph LoopClosing::CorrectLoop runs once a loop is accepted and fused, and the per-point loop
 * correctedSwr.map(Srw.map(P)) around it (:854-885, src/LoopClosing.cpp:470-500).  Every job of a call is one workgroup of ONE launch with the
 * whole optimize(20) inside the kernel.  g2o is not in the tree and libm's log / acos / exp / sin / cos differ from the device's in ulps, so the
 * definition of record is the project's own core, csrc/cms_ess_graph_core.h (DESIGN.md "OptimizeEssentialGraph"): one source, built for the host
 * (libcubemapslam_host.so: hm_essential_graph_optimize_host) and for the device, which is held to the host build bit for bit.
 *   The graph: N VertexSim3Expmap vertices with the estimates Scw (vScw: the CorrectedSim3 value where there is one, else Sim3(Rcw, tcw, 1)),
 *   vertex `fixed` (pLoopKF) fixed; E EdgeSim3 edges (v0, v1, kind) in the reference's order of addEdge, information = I, no robust kernel.
 *   The measurement of an edge is Sji = Sjw * Swi with i = v0, j = v1, from Scw for kind 0 (the loop-connection edges, :693-722) and from Snc
 *   for kind 1 (spanning tree, loop and covisibility edges, :724-825; Snc = the NonCorrectedSim3 value where there is one, else the Scw entry).
 *   The pointer work of :650-825 (vertex compaction, bad key frames, minFeat, sInsertedEdges) is the caller's.
 *   The error is log(C * S_v0 * S_v1^-1) with Sim3::log as written (four branches, a 3 x 3 partial-pivot LU); EdgeSim3 has no linearizeOplus, so
 *   both Jacobians are g2o's central differences with delta = 1e-9; under fix_scale their column 6 is exactly 0 and the scale rows of the system
 *   are lambda alone.  Levenberg with setUserLambdaInit(lambda_init) (the reference: 1e-16) and optimize(iterations) (20).  The normal end is ten
 *   rejected trials at the minimum (flags & 1).
 *   The solve is a block LDL^T inside the row envelope of the unknowns in ascending vertex index, unpivoted -- the ONE stated difference from the
 *   reference's SimplicialLDLT under an AMD ordering: the same factorisation in exact arithmetic, another rounding.  A zero or non-finite pivot
 *   is a failed solve (flags & 8): the trial is rejected and lambda grows, as g2o does when its solver fails.
 *   Out: S_out (N x 8, q(x y z w) | t | s; the fixed vertex gets its input back), Tiw_out (N x 12 floats, [R | t / s] row major, :833-852),
 *   chi2_initial, chi2_final, lambda_final, iterations_run, trials_run, flags (1 ended on ten rejected trials, 2 on rho == 0, 4 on three
 *   iterations without progress, 8 a failed solve).  iterations == 0 returns the input and chi2_initial; E == 0 with N == 1 returns the input.
 *   Synchronous; one launch sequence per call on the handle's stream: one pinned block up, one launch, one block back.  ctx supplies the device;
 *   nothing is enqueued on its stream.  Checked before anything is enqueued or written (CMS_ERR_ARG, the reason in cms_last_error, the records
 *   untouched): a null array, N < 1, fixed out of range, an edge index out of range or v0 == v1, a kind outside {0, 1}, a non-finite entry or a
 *   scale <= 0 in Scw / Snc, iterations < 0, lambda_init not positive and finite, a context on another device, more jobs / vertices / edges than
 *   cms_ess_graph_create was given, a vertex with no path to `fixed` (stated difference: g2o would factor a singular matrix).  The jobs' envelopes
 *   exceeding max_envelope_blocks_total is CMS_ERR_OVERFLOW with the needed block count in the message, before any launch.  njobs == 0 is CMS_OK
 *   with no launch.  One caller at a time per handle.
 * cms_sim3_correct_points: pos_out[k] = S_new[ref[k]]^-1.map(S_old[ref[k]].map(pos_in[k])) in double, narrowed once; ref[k] < 0 copies the point.
 * S_old / S_new are K x 8.  Synchronous on ctx's stream.  CMS_ERR_ARG: a null array with n > 0, n < 0, K < 0, ref[k] >= K. */
typedef struct cms_ess_graph cms_ess_graph;
int cms_ess_graph_create(cms_ess_graph** out, int device, int max_jobs, int max_vertices_total, int max_edges_total, int max_envelope_blocks_total);
void cms_ess_graph_destroy(cms_ess_graph* p);
typedef struct {
  int N; const double* Scw; const double* Snc;    /* N x 8: q(x y z w) | t | s */
  int fixed;                                      /* vertex index of pLoopKF */
  int E; const int* edges;                        /* E x 3: v0, v1, kind (0 = measurement from Scw, 1 = from Snc) */
  int fix_scale, iterations; double lambda_init;  /* 20, 1e-16 */
  double* S_out; float* Tiw_out;                  /* N x 8, N x 12 */
  double chi2_initial, chi2_final, lambda_final; int iterations_run, trials_run, flags;   /* out */
} cms_ess_graph_job;
int cms_essential_graph_optimize(cms_ess_graph* h, cms_ctx* ctx, int njobs, cms_ess_graph_job* jobs);
int cms_sim3_correct_points(cms_ctx* ctx, int n, const float* pos_in, const int* ref, int K, const double* S_old, const double* S_new, float* pos_out);

/* ---- Initializer (include/Initializer.h, src/Initializer.cpp), the two-view essential-matrix RANSAC of Tracking::MonocularInitialization
 * (src/Tracking.cpp:443), behind cms_search_for_initialization.  ComputeE21 takes the last row of a FULL_UV SVD of an 8 x 9 matrix, which OpenCV
 * completes from a basis nobody can pin (DESIGN.md "Initializer"), so the definition of record is the project's own core, csrc/cms_init_core.h: one
 * source, built for the host (libcubemapslam_host.so: hm_init_two_view_host) and for the device, which is held to the host build bit for bit.
 * cms_init_two_view: InitializeWithRays (:53-116) with FindEssential, ComputeE21, CheckEssiential, ReconstructE, DecomposeE, CheckRT and Triangulate
 *   for njobs initializers -- one camera stream each -- as ONE launch sequence on ctx's stream: one pinned block up, every hypothesis of every job
 *   in parallel (k_init_hypotheses), one wavefront per hypothesis for CheckEssiential (k_init_check), one workgroup per job for the selection, DecomposeE
 *   and the four CheckRT passes (k_init_select), one block back; ReconstructE's decision (with the acos of the parallax) is taken on the host.
 *   Synchronous: Tracking decides on the result at once.
 *   keys are pt.x, pt.y pairs; matches12[i] = key point of frame 2 matched to key point i of frame 1, or -1 (the vector SearchForInitialization
 *   fills).  The N matches are those with matches12[i] >= 0, in index order (mvMatches12).  The caller makes the draws: draws[8*it + k] = the k-th
 *   DUtils::Random::RandomInt(0, size - 1) of iteration it, size = N, N-1, ..., N-7, so 0 <= draws[8*it + k] <= N-1-k; the call resolves them by the
 *   reference's swap-and-pop (:92-107).
 *   status 1: initialised -- R21 (row major), t21, p3d (vP3D, n1 x 3) and triangulated (vbTriangulated, n1 bytes), both indexed by the key point of
 *   frame 1; an entry never written is (0,0,0) / 0.  status 0: the reference returns false; R21, t21, p3d and triangulated are zeroed.  Diagnostics
 *   either way: best_iteration (first iteration of maximal score under >, -1 when no score exceeds 0), score, n_inliers of its mask, nGood[4] and
 *   parallax[4] (degrees) of the hypotheses (R1,t) (R2,t) (R1,-t) (R2,-t), winner = 0..3 or -1.
 *   Checked before anything is enqueued (CMS_ERR_ARG, the records untouched): fewer than 8 matches (the reference would index an empty vector;
 *   Tracking asks for 100), iterations < 1, n_draws < 8*iterations, a draw out of range, a match index outside [-1, n2), a null array, totals of
 *   jobs / matches / key points of frame 1 / hypotheses above what cms_init_create was given.
 * cms_init_two_view_frames: the same with frame 2 taken on the device from row b of ctx's last batch (cms_frames_process / cms_extract), n2 = the
 *   row's key-point count as the caller fetched it; keys2 / rays2 are ignored.  n2 above the context's kp_cap or b beyond its batch are CMS_ERR_ARG.
 * One caller at a time per context and per handle. */
typedef struct cms_init cms_init;
int cms_init_create(int device, int max_jobs, int max_matches_total, int max_keys1_total, int max_hyp_total, cms_init** out);
void cms_init_destroy(cms_init* p);
typedef struct {
  int n1, n2;                 /* key points of the reference frame (1) and of the current frame (2) */
  const float* keys1;         /* n1 x 2  mvKeys1[i].pt */
  const float* rays1;         /* n1 x 3  mvKeyRays1 */
  const float* keys2;         /* n2 x 2  | cms_init_two_view_frames: ignored, taken from the frame row */
  const float* rays2;         /* n2 x 3  | same */
  const int* matches12;       /* n1 */
  int b;                      /* cms_init_two_view_frames only: row b of ctx's last batch */
  float sigma; int iterations;
  int n_draws; const int* draws;   /* eight per iteration */
  int status; float R21[9], t21[3]; float* p3d; uint8_t* triangulated;   /* out; p3d n1 x 3 floats, triangulated n1 bytes */
  int best_iteration; float score; int n_inliers, nGood[4]; float parallax[4]; int winner;   /* out: diagnostics */
} cms_init_job;
int cms_init_two_view(cms_init* p, cms_ctx* ctx /* F, field of view, stream */, int njobs, cms_init_job* jobs);
int cms_init_two_view_frames(cms_init* p, cms_ctx* ctx, int njobs, cms_init_job* jobs);

/* ---- pose-only optimisation: Optimizer::PoseOptimization(Frame*) (src/Optimizer.cpp:48-190), the per-frame solver Tracking calls
 * 1-3 times per frame (Tracking.cpp:585,647,688).  Edge = EdgeSE3ProjectXYZMultiPinholeOnlyPose
 * (include/g2o_cubemap_vertices_edges.h:42-88, src/g2o_cubemap_vertices_edges.cpp:61-134).  One workgroup per frame runs all four
 * rounds (10 Levenberg iterations each, chi2 > 5.991 re-classification in between, Huber dropped for the last round) on the device;
 * a batch of nf frames (camera streams) is ONE launch.  The caller prepares, exactly as Optimizer.cpp:80-127 does per matched
 * map point whose key ray passes the FoV test: Xw (world point), obs_uv = GetPosInFace(kp.pt), face = FaceInCubemap(kp.pt),
 * inv_sigma2 = mvInvLevelSigma2[kp.octave]; edge_off[f]..edge_off[f+1] are frame f's edges.  poses7: nf x (tx,ty,tz,qx,qy,qz,qw),
 * world->camera, in/out.  outlier: one byte per edge (pFrame->mvbOutlier).  n_inliers[f] = nInitialCorrespondences - nBad, or 0
 * and an untouched pose when the frame has fewer than 3 edges.
 * A frame's result is a function of the frame and the four intrinsics alone, to the last bit: it does not depend on the frame's position or
 * company in the batch (a frame above 1024 edges sends the whole batch through the kernel that keeps the edges in memory instead of in
 * registers: same bits), nor on the entry point (cms_pose_optimize_batch with few or many frames, upload / launch / fetch, cms_pose_optimize),
 * nor on what the handle was used for before (tests/test_gpu_pose_matrix.py). */
typedef struct cms_pose cms_pose;
typedef struct { int rounds, n_bad; int iterations_done[4]; } cms_pose_stats;
int cms_pose_create(cms_pose** out, int device, int max_frames, int max_edges);
void cms_pose_destroy(cms_pose* p);
void* cms_pose_stream(cms_pose* p);
int cms_pose_optimize_batch(cms_pose* p, int nf, const int* edge_off, const double* Xw, const double* obs_uv, const double* inv_sigma2,
                            const int8_t* face, double fx, double fy, double cx, double cy, double* poses7, uint8_t* outlier,
                            int* n_inliers, cms_pose_stats* stats);
/* the same in three steps, for callers that keep the problem resident: upload once, launch (asynchronous, restarts from the
 * uploaded poses every time; the results' copies into the handle's pinned block are enqueued right behind the kernel), fetch (waits for
 * those copies -- nothing is enqueued at fetch time, so a caller that launches early and fetches late does not wait for a slot on a busy
 * device -- and hands the results out; may be called again for the same launch) */
int cms_pose_upload(cms_pose* p, int nf, const int* edge_off, const double* Xw, const double* obs_uv, const double* inv_sigma2,
                    const int8_t* face, double fx, double fy, double cx, double cy, const double* poses7);
int cms_pose_launch(cms_pose* p);
int cms_pose_fetch(cms_pose* p, double* poses7, uint8_t* outlier, int* n_inliers, cms_pose_stats* stats);
/* one frame, one shot (create + optimize + destroy) */
int cms_pose_optimize(int device, int n, const double* Xw, const double* obs_uv, const double* inv_sigma2, const int8_t* face,
                      double fx, double fy, double cx, double cy, double* pose7, uint8_t* outlier, int* n_inliers, cms_pose_stats* stats);

/* ---- Covisibility on resident key frames: KeyFrame::UpdateConnections (src/KeyFrame.cpp:315-404), LocalMapping::KeyFrameCulling
 * (src/LocalMapping.cpp:561-619), the votes of Tracking::UpdateLocalKeyFrames (src/Tracking.cpp:881-928) and Tracking::UpdateLocalPoints (:855-878).
 * The definition of record is csrc/cms_covis_core.h (DESIGN.md "Covisibility on the device"): one source, built for the host (hm_covis_* of
 * libcubemapslam_host.so) and for the kernels.  Everything is integer work: the results equal the host core's exactly.
 *
 * A cms_covis is an OBSERVATION INDEX over a list of member slots of one store: the key frames of one map that are not bad, in the caller's order.
 * An observation is (id, member position, feature, octave) for every feature of a member with mp >= 0 (ids in [0, 2^30)); Observations(id) is the
 * number of members holding the id (MapPoint::nObs).  A member is named by its POSITION in the list in every query and result.
 * Threading: calls on one cms_covis are serialised by a mutex in the handle; the store must outlive it.
 *
 * cms_covis_build snapshots the members' mp rows and octaves as the store holds them at that moment (on the store's stream, behind pending puts and
 * updates) and builds the index from the snapshot.  Every query answers from the last successful build: a later cms_kfstore_update* is not seen until
 * the next build.  CMS_ERR_ARG: an empty slot, a slot named twice, more members than max_members, or a row that names an id twice
 * (MapPoint::AddObservation's invariant) -- then the previous index stays in place.  CMS_ERR_UNSUPPORTED: more than 16 384 members. */
typedef struct cms_covis cms_covis;
int cms_covis_create(cms_covis** out, cms_kfstore* st, int max_members);
void cms_covis_destroy(cms_covis* cv);
int cms_covis_build(cms_covis* cv, int n_members, const int* member_slots);
/* keyframeCounter (Tracking.cpp:885-901) of njobs frames in one launch: job j lists the ids of its frame's non-NULL, non-bad map points in
 * ids[id_off[j], id_off[j + 1]); votes[j * n_members + m] is the number of entries that member m observes.  An id listed twice counts twice (the
 * reference loops over key points), an id the index does not know adds nothing, a negative id is CMS_ERR_ARG.  On src's stream (the frame thread's),
 * which waits on the device for the last build. */
int cms_covis_votes(cms_covis* cv, cms_ctx* src, int njobs, const int* id_off, const int* ids, int* votes);
/* UpdateConnections up to the pointer work (KeyFrame.cpp:317-394) for the members job_member[j]: weights[j * n_members + m] is KFcounter (ids
 * shared with member m, 0 for the member itself); order[j * n_members + i] lists the members with weight >= th (15 in the reference) in descending
 * weight, ties to the EARLIER member position (the reference sorts pair<int, KeyFrame*>: the pointer decides there), -1 behind them.  Nobody reaches
 * th: the single member of maximal weight, the earliest such (:374-378).  An empty KFcounter: n_connected[j] = 0 (:349).  The first N entries are
 * GetBestCovisibilityKeyFrames(N).  AddConnection on the others, the parent and the spanning tree stay host code.  On the store's stream. */
int cms_covis_connections(cms_covis* cv, int njobs, const int* job_member, int th, int* weights, int* order, int* n_connected);
/* KeyFrameCulling's counters (LocalMapping.cpp:569-618).  Chain c lists the candidates of ONE KeyFrameCulling call in the reference's order
 * (GetVectorCovisibleKeyFrames() minus mnId == 0) as job_member[chain_off[c], chain_off[c + 1]); chains are independent.  Per job: n_mps the
 * features with a live id, n_redundant those with Observations(id) > th_obs (3) that at least th_obs OTHER live members observe at
 * octave_i <= octave + 1 (:588-610), redundant = (double)n_redundant > 0.9 * (double)n_mps (:616).  The jobs of a chain are evaluated as if one
 * after the other: a redundant job with erasable[j] != 0 (!mbNotErase) leaves before the next one, each of its ids loses an observation, and an id
 * that falls to <= 2 becomes bad and vanishes from every member (MapPoint.cpp:115-136, KeyFrame.cpp:494-496).  All of that lives in scratch of the
 * call: the index is unchanged afterwards; the caller applies SetBadFlag on the host and rebuilds.  A member twice in a chain is CMS_ERR_ARG.  On the
 * store's stream. */
int cms_covis_culling(cms_covis* cv, int n_chains, const int* chain_off, const int* job_member, const uint8_t* erasable, int th_obs, int* n_mps,
                      int* n_redundant, uint8_t* redundant);
/* UpdateLocalPoints (Tracking.cpp:857-877): job j lists its local key frames as members in kf_members[kf_off[j], kf_off[j + 1]) (each once);
 * ids_out[j * cap + i] are the ids of their rows in member order, then feature order, each id once at its first occurrence; n_out[j] their number.
 * More than cap: CMS_ERR_OVERFLOW with n_out delivered and the first cap ids written.  Stream rules of cms_covis_votes. */
int cms_covis_local_points(cms_covis* cv, cms_ctx* src, int njobs, const int* kf_off, const int* kf_members, int cap, int* ids_out, int* n_out);
/* n (slot, feature, new id) triples into the slots' mp rows (ORBMatcher::Fuse's Replace, MapPointCulling: a handful of entries in many key frames),
 * id in [-1, 2^30): one kernel reading a pinned block, asynchronous on the store's stream like cms_kfstore_update_poses.  All triples are checked
 * first (a (slot, feature) named twice is CMS_ERR_ARG): on an error nothing is written. */
int cms_kfstore_update_map_points(cms_kfstore* st, int n, const int* slot, const int* feat, const int* mp);

/* ---- Map points on resident key frames: MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cpp:243-308) and MapPoint::UpdateNormalAndDepth
 * (:332-373) from the observation index, and the two per-key-frame consumers of map-point attributes taking ids.  The definition of record is
 * csrc/cms_mappoint_core.h (DESIGN.md "Map points on the device"): one source, built for the host (hm_mpstore_* of libcubemapslam_host.so) and for
 * the kernels.  Descriptors, indices and status equal the host core's exactly, normal and bounds bit for bit.
 *
 * A cms_mpstore is a TABLE OF ROWS next to one store, indexed directly by the map point's id: 0 <= id < max_points (otherwise CMS_ERR_ARG), the ids
 * the store's mp rows and a cms_covis hold; a binding hands out rows the way it hands out key-frame slots.  A row holds the world position, the
 * normal, mfMinDistance / mfMaxDistance, the 32-byte descriptor, mpRefKF as a store slot and the (member, feature) the descriptor came from.
 *
 * The observations of an id are the index's entries for it, taken in ASCENDING MEMBER POSITION (the reference iterates a std::map<KeyFrame*, size_t>:
 * the pointer decides there).  cms_distinctive_descriptors / cms_update_normal_and_depth called with observations listed in member order give the
 * same results.  The descriptor is the observation of least median Hamming distance, the earliest member on ties; the normal is summed in member
 * order in k_update_normal_depth's float arithmetic; the bounds come from the observation whose member lives in the reference slot.  Camera centres
 * are what the store holds when the refresh runs (behind pending cms_kfstore_update_poses); features and octaves are the index's snapshot: a
 * cms_kfstore_update_map_points is not seen before the next cms_covis_build.
 *
 * Every entry checks all its arguments on the host before anything is enqueued (ids in range, an id named twice in set / erase / refresh, a consumer
 * naming a row without descriptor or normal): on an error nothing is written and cms_last_error names the reason.
 * Threading: calls on one cms_mpstore are serialised by a mutex in the handle; the store and any cms_covis passed in must outlive the call, and a
 * refresh also holds the cms_covis's mutex.  set / erase / refresh / fetch and the Fuse entry run on the store's stream. */
typedef struct cms_mpstore cms_mpstore;
#define CMS_MP_DESCRIPTOR 1
#define CMS_MP_NORMAL_DEPTH 2
int cms_mpstore_create(cms_mpstore** out, cms_kfstore* st, int max_points);
void cms_mpstore_destroy(cms_mpstore* mp);
/* n rows named by id: world position (3 floats each, NULL = unchanged) and mpRefKF as a store slot (NULL = unchanged; any slot index of the store).
 * A row is created by its first set, which wants both.  One kernel reading a pinned block, asynchronous on the store's stream. */
int cms_mpstore_set(cms_mpstore* mp, int n, const int* ids, const float* pos, const int* ref_slot);
/* SetBadFlag / Replace: the row is empty again.  Asynchronous like cms_mpstore_set. */
int cms_mpstore_erase(cms_mpstore* mp, int n, const int* ids);
/* Rows of n ids (each set, none twice) from the index cv of the same store, one wavefront per map point; what = CMS_MP_DESCRIPTOR, CMS_MP_NORMAL_DEPTH
 * or both (the reference calls UpdateNormalAndDepth alone after a bundle adjustment).  status[i]: 0 done; 1 the index knows no observation of the id,
 * the row is untouched (the reference's early return); 2 normal and depth were asked for and the reference slot is not a member that observes the id,
 * the row is untouched (descriptor included).  Synchronous, one wait. */
int cms_mpstore_refresh(cms_mpstore* mp, cms_covis* cv, int n, const int* ids, int what, uint8_t* status);
/* The rows of n ids as the table holds them (MapPoint::mDescriptor, mNormalVector, mfMin/MaxDistance back on the host); any output may be NULL.
 * An empty row reads zeros, best (-1, -1).  Synchronous. */
int cms_mpstore_fetch(cms_mpstore* mp, int n, const int* ids, float* pos, float* normal, float* min_dist, float* max_dist, uint8_t* desc,
                      int* best_member, int* best_feature);
/* cms_search_local_points with the map points named by id: one gather kernel writes their rows into the staged block, then the unchanged launch
 * chain.  Every row must hold a descriptor and a normal (CMS_ERR_ARG otherwise).  Table values are the raw mfMinDistance / mfMaxDistance:
 * cms_set_distance_bounds_mode does not apply.  On ctx's stream, which waits on the device for the table's last write; ctx must be on the store's
 * device (CMS_ERR_ARG). */
int cms_search_local_points_ids(cms_ctx* ctx, int b, const float* pose15, cms_mpstore* mp, int nmp, const int* ids, float viewing_cos_limit, float th,
                                float nnratio, int th_high, int nkp, int* kp_mp, uint8_t* in_view, float* proj_x, float* proj_y, int* level,
                                float* view_cos, int* mp_match, int* n_matches, int* rounds);
/* cms_kfstore_fuse_search_sets with the sets' map points named by id (ids: set_off[nsets] entries); mp must belong to st.  Rows and distance bounds
 * as for cms_search_local_points_ids.  On the store's stream. */
int cms_kfstore_fuse_search_sets_ids(cms_kfstore* st, cms_mpstore* mp, int nsets, const int* set_off, const int* ids, int njobs, const int* job_slot,
                                     const int* job_set, const uint8_t* skip, float th, int* best_idx, int* best_dist);

/* ---- Local BA window from the resident stores: what Optimizer::LocalBundleAdjustment collects before it optimises (src/Optimizer.cpp:194-357), built
 * on the device from the observation index, the store's slots and the map-point table.  The definition of record is csrc/cms_ba_window_core.h
 * (DESIGN.md "Local BA window from the resident stores"): one source, built for the host (hm_ba_window_* of libcubemapslam_host.so) and for the
 * kernels.  Every output equals the host core's bit for bit.
 *
 * A job names lLocalKeyFrames as member POSITIONS of the index in the reference's order -- the current key frame first, then its
 * GetVectorCovisibleKeyFrames() (`order` of cms_covis_connections) -- and first_member, the member whose mnId is 0, or -1.  Job j owns row j of every
 * output, with strides cap_kf, cap_points and cap_edges (times 7, 3 or 2 for poses, points and e_obs):
 *   counts[j]   {K, n_local, P, E}
 *   point_id    the local points: the ids of the local members' rows in list order, then feature order, each once (cms_covis_local_points)
 *   kf_member   the window's key frames as members: the locals in list order, then the fixed ones -- every other member that observes a local point --
 *               in ascending (list position of the first local point it observes, member position), the order in which the reference meets them
 *   fixed       k >= n_local || kf_member[k] == first_member
 *   poses       (t, q) per key frame: Converter::toSE3Quat of the slot's float Rcw | tcw
 *   points      the table's float positions, widened
 *   e_*         one edge per observation of a local point whose key ray has z >= cos_fov and whose key point lies on a face: points in list order,
 *               a point's observations in ascending member position.  e_pose indexes kf_member, e_point the point list; e_obs is the position in
 *               the face, e_invsig2 mvInvLevelSigma2 of the octave; e_feat is the feature index inside the key frame, so (kf_member[e_pose], e_feat)
 *               names the observation to erase.  A point that keeps no edge stays in the list.
 * The arrays of a job are cms_ba_create's arguments as they lie.
 *
 * What the call sees: rows, features and octaves are the index's SNAPSHOT (a cms_kfstore_update_map_points is not seen before the next
 * cms_covis_build); key points, rays and poses are what the slots hold when the call runs, positions what the table holds then.  It runs on the
 * store's stream, behind the last cms_covis_build, cms_kfstore_update_poses and cms_mpstore_set.  A member slot must not be refilled between the build
 * and the call (cms_mpstore_refresh's contract).
 *
 * All jobs of a call are one launch sequence with one wait.  Outputs may be plain host arrays (copied back through the index's staging block) or ALL
 * lie in pinned memory (cms_host_alloc): then the kernels store into them and the window can go to cms_ba_create_many with CMS_BA_INPUTS_PINNED.
 *
 * CMS_ERR_ARG with nothing written, checked on the host before anything is enqueued: no index built, an index and a table of different stores,
 * n_local < 1, a member out of range or named twice in a job, first_member outside [-1, M), a cap < 1.  A local point whose table row holds no
 * position is found on the device: CMS_ERR_ARG after the wait, the message names the job (plain host outputs are untouched, pinned ones are not).
 * CMS_ERR_OVERFLOW: a job has more key frames, points or edges than a cap; counts holds the true numbers of every job, jobs that fit are complete,
 * and nothing is written at or beyond any cap.  Holds the mutexes of both handles. */
typedef struct { int n_local; const int* local_members; int first_member; } cms_ba_window_job;
typedef struct { int K, n_local, P, E; } cms_ba_window_counts;
int cms_covis_local_ba_windows(cms_covis* cv, cms_mpstore* mp, int njobs, const cms_ba_window_job* jobs, int cap_kf, int cap_points, int cap_edges,
                               cms_ba_window_counts* counts, int* kf_member, int* point_id, double* poses, uint8_t* fixed, double* points, int* e_pose,
                               int* e_point, double* e_obs, double* e_invsig2, int8_t* e_face, int* e_feat);

/* ---- Map-point statistics on the resident stores: LocalMapping::MapPointCulling (src/LocalMapping.cpp:175-206), KeyFrame::TrackedMapPoints
 * (src/KeyFrame.cpp:276-301), KeyFrame::ComputeSceneMedianDepth (:1064-1094) and the mnVisible / mnFound counting of Tracking (src/Tracking.cpp:698,
 * :808, :829).  The definition of record is csrc/cms_mpstats_core.h (DESIGN.md "Map-point statistics on the device"): one source, built for the host
 * (hm_mpstats_* of libcubemapslam_host.so) and for the kernels.  Counts and verdicts equal the host core's by value, depths bit for bit.
 *
 * A table row carries three more columns: mnVisible, mnFound and mnFirstKFid.  An empty row holds (1, 1, -1), what both MapPoint constructors leave;
 * cms_mpstore_erase restores it.  Every entry checks all its arguments on the host before anything is enqueued: a refused call writes nothing. */
#define CMS_MP_VISIBLE 1      /* Tracking.cpp:808 and :829: IncreaseVisible() */
#define CMS_MP_FOUND 2        /* Tracking.cpp:698 (and :264): IncreaseFound() */
/* Absolute values for n set rows (none named twice); any array may be NULL = unchanged.  visible >= 1, found >= 0, first_kf >= -1, otherwise
 * CMS_ERR_ARG.  mnFirstKFid at creation; the counters when a map is loaded.  One kernel reading the pinned record ring of cms_mpstore_set,
 * asynchronous on the store's stream. */
int cms_mpstore_set_stats(cms_mpstore* mp, int n, const int* ids, const int* first_kf, const int* visible, const int* found);
/* MapPoint::Replace's transfer (MapPoint.cpp:209-210) and any host-side IncreaseVisible(n) / IncreaseFound(n): adds; d_* >= 0, NULL = 0.
 * Asynchronous like cms_mpstore_set_stats. */
int cms_mpstore_add_stats(cms_mpstore* mp, int n, const int* ids, const int* d_visible, const int* d_found);
/* The three columns as the table holds them (any output may be NULL); synchronous; an empty row reads (1, 1, -1). */
int cms_mpstore_fetch_stats(cms_mpstore* mp, int n, const int* ids, int* visible, int* found, int* first_kf);
/* The per-frame counting of all frames of a tick.  Job j owns the entries [off[j], off[j + 1]) of ids and of flag; entry i adds 1 to column `which`
 * of row ids[i] iff ids[i] >= 0 and (flag == NULL or (flag[i] != 0) == (count_if != 0)).  A frame's kp_mp row can be passed as it lies (-1 = no
 * point): for CMS_MP_VISIBLE the local ids given to cms_search_local_points_ids with its in_view and count_if = 1, for CMS_MP_FOUND the frame's ids
 * with the pose optimiser's outlier flags and count_if = 0.  An id listed twice counts twice.  CMS_ERR_ARG with nothing written: an id >=
 * max_points or < -1, a counted id whose row was never set.  One launch for all jobs (global atomicAdd), ids and flags read from a pinned ring of
 * four blocks; asynchronous on src's stream (src on the store's device), which waits on the device for the table's last write.  Every later entry
 * on the store's stream that reads or resets the counters (culling, fetch_stats, set_stats, add_stats, set, erase) waits on the device for the
 * call's event: a culling issued after a count returns sees that count completely.  Calls from two frame contexts may overlap. */
int cms_mpstore_count(cms_mpstore* mp, cms_ctx* src, int which, int njobs, const int* off, const int* ids, const uint8_t* flag, int count_if);
/* Job j is one MapPointCulling call: mlpRecentAddedMapPoints as ids in [off[j], off[j + 1]) and mpCurrentKeyFrame->mnId in current_kf[j]; no id
 * twice in the call.  verdict[i] is cms_mpstats_verdict on the row's counters and Observations(id) of the index's snapshot (0 for an id the index
 * does not know): 1 bad by the found ratio, 2 bad by too few observations two key frames on (th_obs: 2 in the reference), 3 leaves the list alive,
 * 0 stays; 4 for an empty row (already bad).  Verdicts of one call do not influence one another.  With apply != 0 the call performs
 * MapPoint::SetBadFlag (MapPoint.cpp:115-136) for verdicts 1 and 2: -1 into the mp row of every observing slot at the recorded feature, only where
 * the row still holds the id, then the table row is emptied (counters included) and refused by later consumers like an erased one.  The index is
 * unchanged and stale until the next cms_covis_build (cms_covis_culling's contract).  One launch, one wavefront per id.  Synchronous with one wait
 * on the store's stream, behind the last build and the last count; holds both handles' mutexes.  CMS_ERR_ARG with nothing written: no index
 * built, an index of another store, an id out of range or named twice, th_obs < 0. */
int cms_mpstore_culling(cms_mpstore* mp, cms_covis* cv, int njobs, const int* off, const int* ids, const int* current_kf, int th_obs, int apply,
                        uint8_t* verdict);
/* count[j] = KeyFrame::TrackedMapPoints(min_obs[j]) of member job_member[j]: the features of the member's snapshot row with an id >= 0 and, when
 * min_obs[j] > 0, Observations(id) >= min_obs[j].  A bad point is one that has left the rows.  One wavefront per job.  Stream rules of
 * cms_covis_votes. */
int cms_covis_tracked_map_points(cms_covis* cv, cms_ctx* src, int njobs, const int* job_member, const int* min_obs, int* count);
/* KeyFrame::ComputeSceneMedianDepth(q) of n slots (each once, none empty): the depths (cms_mpstats_depth of the slot's Rcw, tcw and the row's position) of every feature whose
 * CURRENT mp row entry names an id with a position in the table (an id whose table row is empty takes no part: the reference does not test isBad()
 * here), the element at index (n_depths - 1) / q in ascending order, selected by bisection on the depth key (-0.0f before +0.0f).  A slot without a
 * depth returns -1.0f and n_depths 0.  q >= 1.  With store != 0 every slot with a depth gets the value as its median_depth, as by
 * cms_kfstore_update(..., &median, NULL): the next cms_kfstore_create_new_map_points reads it.  One workgroup per slot, the keys in LDS.
 * Synchronous with one wait on the store's stream, behind pending cms_kfstore_update_poses, cms_kfstore_update_map_points and cms_mpstore_set;
 * holds the table's mutex. */
int cms_kfstore_scene_median_depth(cms_kfstore* st, cms_mpstore* mp, int n, const int* slots, int q, int store, float* depth, int* n_depths);

#ifdef __cplusplus
}
#endif
#endif
