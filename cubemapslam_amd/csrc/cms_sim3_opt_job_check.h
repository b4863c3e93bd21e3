// cms_sim3_opt_job_check.h -- what cms_sim3_optimize checks per job before anything is enqueued.  Host code, shared by the C-ABI entry
// (cms_api_sim3_opt.hip) and the host loop (host/sim3_opt_host.cpp), so both refuse the same records with the same words.  Needs
// cms_sim3_opt_job (include/cubemapslam_hip.h) and cms_sim3_opt_core.h before it.  Returns NULL or the reason.
#pragma once

static inline const char* cms_sim3_opt_check_job(int F, const cms_sim3_opt_job& q) {
  if (q.N < 0) return "N < 0";
  if (q.N > 0 && (!q.x3dc1 || !q.x3dc2 || !q.kp1 || !q.kp2 || !q.inv_sigma2_1 || !q.inv_sigma2_2 || !q.keep)) return "a null array";
  if (!(q.th2 > 0.0f) || !(q.th2 - q.th2 == 0.0f)) return "th2 not finite or <= 0";
  if (!(q.s12 > 0.0) || !(q.s12 - q.s12 == 0.0)) return "s12 not finite or <= 0";
  if (q.jacobian != CMS_SIM3_OPT_AS_WRITTEN && q.jacobian != CMS_SIM3_OPT_ANALYTIC) return "jacobian outside {0, 1}";
  for (int k = 0; k < q.N; ++k)
    if (cms_s3o_face_in_cubemap(F, q.kp1[2 * k], q.kp1[2 * k + 1]) < 0 || cms_s3o_face_in_cubemap(F, q.kp2[2 * k], q.kp2[2 * k + 1]) < 0)
      return "a key point that lies in no face (the reference's computeError would exit)";
  return nullptr;
}
