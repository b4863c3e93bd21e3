// cms_api_ess_graph.hip -- host side of Optimizer::OptimizeEssentialGraph (src/Optimizer.cpp:623-886): the cms_ess_graph handle,
// cms_essential_graph_optimize and cms_sim3_correct_points; included by cms_lib.hip behind cms_api_frames.hip (cms_ctx, cms_fail, HIPCHK, CmsBlock,
// CmsStage), cms_api_ransac.h (the handle base and the check at the head of an entry) and cms_ess_graph_kernels.hip.  All jobs of a call are ONE
// launch on the handle's stream: one pinned block up (the job records, the estimates, the edges and the structure of every job's system:
// incidence lists, envelope rows, column lists), k_ess_graph_optimize, one pinned block back.  Everything that becomes a device index is checked
// on the host before anything is enqueued or written (cms_ess_graph_job_check.h).
#include <cstring>
#include <string>
#include <vector>
#include "cms_ess_graph_job_check.h"

struct cms_ess_graph : CmsRansacHandle {
  int max_vertices = 0, max_edges = 0, max_blocks = 0;
};

extern "C" int cms_ess_graph_create(cms_ess_graph** out, int device, int max_jobs, int max_vertices_total, int max_edges_total, int max_envelope_blocks_total) {
  if (!out || max_jobs < 1 || max_vertices_total < 1 || max_edges_total < 0 || max_envelope_blocks_total < 0) return cms_fail(CMS_ERR_ARG, "cms_ess_graph_create: bad argument");
  const int rcd = cms_check_device(device, "cms_ess_graph_create: no HIP device (OptimizeEssentialGraph's device path has no CPU fallback)");
  if (rcd) return rcd;
  cms_ess_graph* p = new cms_ess_graph();
  p->max_vertices = max_vertices_total; p->max_edges = max_edges_total; p->max_blocks = max_envelope_blocks_total;
  const int rc = p->open(device, max_jobs, true, "cms_ess_graph_create");
  if (rc) { cms_ransac_free(p); return rc; }
  *out = p;
  return CMS_OK;
}
extern "C" void cms_ess_graph_destroy(cms_ess_graph* p) { cms_ransac_free(p); }

extern "C" int cms_essential_graph_optimize(cms_ess_graph* p, cms_ctx* c, int njobs, cms_ess_graph_job* jobs) {
  int rc = cms_ransac_check_entry(p, c, njobs, jobs, "cms_essential_graph_optimize");
  if (rc || njobs == 0) return rc;
  long long V = 0, E = 0, B = 0;
  std::vector<CmsEgStructure> st((size_t)njobs);
  for (int j = 0; j < njobs; ++j) {
    const cms_ess_graph_job& q = jobs[j];
    const char* why = cms_ess_graph_check_job(q);
    if (why) return cms_fail(CMS_ERR_ARG, (std::string("cms_essential_graph_optimize: ") + why).c_str());
    V += q.N; E += q.E;
    if (V > p->max_vertices) return cms_fail(CMS_ERR_ARG, "cms_essential_graph_optimize: more vertices than the handle was created for");
    if (E > p->max_edges) return cms_fail(CMS_ERR_ARG, "cms_essential_graph_optimize: more edges than the handle was created for");
    B += cms_eg_envelope(q.N, q.fixed, q.E, q.edges, st[(size_t)j].first);
  }
  if (B > p->max_blocks)
    return cms_fail(CMS_ERR_OVERFLOW, ("cms_essential_graph_optimize: the jobs' envelopes need " + std::to_string(B) + " blocks, the handle has " + std::to_string(p->max_blocks)).c_str());
  for (int j = 0; j < njobs; ++j) cms_eg_structure(jobs[j].N, jobs[j].fixed, jobs[j].E, jobs[j].edges, st[(size_t)j]);
  const size_t V_ = (size_t)V, E_ = (size_t)E, B_ = (size_t)B, J_ = (size_t)njobs, F_ = V_ - J_;      // F_: free vertices
  CmsBlock blk;
  const size_t o_work = blk.take(J_ * sizeof(CmsEgWork)), o_scw = blk.take(V_ * 64), o_snc = blk.take(V_ * 64), o_edges = blk.take(E_ * 12), o_incoff = blk.take((V_ + J_) * 4),
               o_inc = blk.take(E_ * 8), o_first = blk.take(F_ * 4), o_rowp = blk.take(F_ * 8), o_colp = blk.take(V_ * 4), o_coli = blk.take((B_ - F_) * 4);
  const size_t in_bytes = blk.size;
  const size_t o_out = blk.take(J_ * sizeof(CmsEgOut)), o_sout = blk.take(V_ * 64), o_tiw = blk.take(V_ * 48);
  const size_t out_begin = o_out, out_end = blk.size;
  const size_t o_S = blk.take(V_ * 64), o_T = blk.take(V_ * 64), o_P = blk.take(V_ * 14 * 64), o_C = blk.take(E_ * 64), o_err = blk.take(E_ * 56), o_chi = blk.take(E_ * 8),
               o_J = blk.take(E_ * 98 * 8), o_H = blk.take(B_ * 392), o_L = blk.take(B_ * 392), o_D = blk.take(F_ * 56), o_RD = blk.take(F_ * 56), o_b = blk.take(F_ * 56),
               o_x = blk.take(F_ * 56), o_sc = blk.take(F_ * 8);
  HIPCHK(hipSetDevice(p->device));
  hipStream_t s = p->stream;
  rc = p->blocks.reserve(s, blk.size, out_end);
  if (rc) return rc;
  uint8_t* h = p->blocks.h;
  uint8_t* d = p->blocks.d;
  std::memset(h, 0, in_bytes);
  size_t v0 = 0, e0 = 0, b0 = 0, f0 = 0;
  for (int j = 0; j < njobs; ++j) {
    const cms_ess_graph_job& q = jobs[j];
    const CmsEgStructure& t = st[(size_t)j];
    const size_t n = (size_t)q.N, ne = (size_t)q.E, nf = n - 1, nb = (size_t)t.blocks, ji = (size_t)j;
    std::memcpy(h + o_scw + 64 * v0, q.Scw, 64 * n); std::memcpy(h + o_snc + 64 * v0, q.Snc, 64 * n);
    if (ne) { std::memcpy(h + o_edges + 12 * e0, q.edges, 12 * ne); std::memcpy(h + o_inc + 8 * e0, t.inc.data(), 8 * ne); }
    std::memcpy(h + o_incoff + 4 * (v0 + ji), t.inc_off.data(), 4 * (n + 1));
    std::memcpy(h + o_colp + 4 * v0, t.colp.data(), 4 * n);      // Nf + 1 = N entries
    if (nf) { std::memcpy(h + o_first + 4 * f0, t.first.data(), 4 * nf); std::memcpy(h + o_rowp + 8 * f0, t.rowp.data(), 8 * nf); }
    if (nb > nf) std::memcpy(h + o_coli + 4 * (b0 - f0), t.coli.data(), 4 * (nb - nf));
    CmsEgWork w = {};
    w.N = q.N; w.fixed = q.fixed; w.E = q.E; w.fix_scale = q.fix_scale ? 1 : 0; w.iterations = q.iterations; w.Nf = q.N - 1; w.lambda_init = q.lambda_init; w.B = t.blocks;
    w.Scw = (const CmsS3*)(d + o_scw) + v0; w.Snc = (const CmsS3*)(d + o_snc) + v0; w.edges = (const int*)(d + o_edges) + 3 * e0;
    w.inc_off = (const int*)(d + o_incoff) + v0 + ji; w.inc = (const int*)(d + o_inc) + 2 * e0; w.first = (const int*)(d + o_first) + f0;
    w.rowp = (const long long*)(d + o_rowp) + f0; w.colp = (const int*)(d + o_colp) + v0; w.coli = (const int*)(d + o_coli) + (b0 - f0);
    w.S = (CmsS3*)(d + o_S) + v0; w.T = (CmsS3*)(d + o_T) + v0; w.P = (CmsS3*)(d + o_P) + 14 * v0; w.C = (CmsS3*)(d + o_C) + e0;
    w.err = (double*)(d + o_err) + 7 * e0; w.chi = (double*)(d + o_chi) + e0; w.J = (double*)(d + o_J) + 98 * e0;
    w.H = (double*)(d + o_H) + 49 * b0; w.L = (double*)(d + o_L) + 49 * b0;
    w.D = (double*)(d + o_D) + 7 * f0; w.RD = (double*)(d + o_RD) + 7 * f0; w.b = (double*)(d + o_b) + 7 * f0; w.x = (double*)(d + o_x) + 7 * f0; w.sc = (double*)(d + o_sc) + f0;
    w.S_out = (CmsS3*)(d + o_sout) + v0; w.Tiw_out = (float*)(d + o_tiw) + 12 * v0; w.out = (CmsEgOut*)(d + o_out) + ji;
    std::memcpy(h + o_work + ji * sizeof(CmsEgWork), &w, sizeof(w));
    v0 += n; e0 += ne; b0 += nb; f0 += nf;
  }
  rc = p->blocks.up(s, in_bytes, "cms_essential_graph_optimize");
  if (rc) return rc;
  hipLaunchKernelGGL(k_ess_graph_optimize, dim3(njobs), dim3(CMS_EG_THREADS), 0, s, (const CmsEgWork*)(d + o_work), njobs);
  HIPCHK(hipGetLastError());
  rc = p->blocks.back_and_wait(s, out_begin, out_end, "cms_essential_graph_optimize");
  if (rc) return rc;
  v0 = 0;
  for (int j = 0; j < njobs; ++j) {
    cms_ess_graph_job& q = jobs[j];
    const CmsEgOut& o = reinterpret_cast<const CmsEgOut*>(h + o_out)[j];
    const size_t n = (size_t)q.N;
    std::memcpy(q.S_out, h + o_sout + 64 * v0, 64 * n); std::memcpy(q.Tiw_out, h + o_tiw + 48 * v0, 48 * n);
    q.chi2_initial = o.chi2_initial; q.chi2_final = o.chi2_final; q.lambda_final = o.lambda_final;
    q.iterations_run = o.iterations_run; q.trials_run = o.trials_run; q.flags = o.flags;
    v0 += n;
  }
  return CMS_OK;
}

// the per-point loop around the optimisation (:854-885, LoopClosing.cpp:470-500), on ctx's stream through ctx's staging block
extern "C" int cms_sim3_correct_points(cms_ctx* c, int n, const float* pos_in, const int* ref, int K, const double* S_old, const double* S_new, float* pos_out) {
  if (!c || n < 0 || K < 0 || (n > 0 && (!pos_in || !ref || !pos_out))) return cms_fail(CMS_ERR_ARG, "cms_sim3_correct_points: bad argument");
  for (int k = 0; k < n; ++k)
    if (ref[k] >= K || (ref[k] >= 0 && (!S_old || !S_new))) return cms_fail(CMS_ERR_ARG, "cms_sim3_correct_points: ref out of range");
  if (n == 0) return CMS_OK;
  const size_t n_ = (size_t)n, K_ = (size_t)K;
  CmsBlock blk;
  const size_t o_pos = blk.take(n_ * 12), o_ref = blk.take(n_ * 4), o_old = blk.take(K_ * 64), o_new = blk.take(K_ * 64);
  const size_t in_bytes = blk.size;
  const size_t o_out = blk.take(n_ * 12);
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  int rc = c->stage.reserve(s, blk.size, blk.size);
  if (rc) return rc;
  uint8_t* h = c->stage.h;
  uint8_t* d = c->stage.d;
  std::memcpy(h + o_pos, pos_in, n_ * 12); std::memcpy(h + o_ref, ref, n_ * 4);
  if (K_) { std::memcpy(h + o_old, S_old, K_ * 64); std::memcpy(h + o_new, S_new, K_ * 64); }
  rc = c->stage.up(s, in_bytes, "cms_sim3_correct_points");
  if (rc) return rc;
  CmsEgPointArgs a = {n, (const float*)(d + o_pos), (const int*)(d + o_ref), (const CmsS3*)(d + o_old), (const CmsS3*)(d + o_new), (float*)(d + o_out)};
  hipLaunchKernelGGL(k_sim3_correct_points, dim3((n + 255) / 256), dim3(256), 0, s, a);
  HIPCHK(hipGetLastError());
  rc = c->stage.back_and_wait(s, o_out, blk.size, "cms_sim3_correct_points");
  if (rc) return rc;
  std::memcpy(pos_out, h + o_out, n_ * 12);
  return CMS_OK;
}
