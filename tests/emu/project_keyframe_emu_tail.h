// the driver of tests/test_project_keyframe_emu_cpu.py: every thread of every block, one after the other
extern "C" void emu_project(int n, const int* pt_job, const float* pose12, const int* job_frame, const int* job_kp0, const CmsKeyPoint* kf_kp, const int* kf_feat,
  const float* kf_angle, const float* pos, const float* mn, const float* mx, float th, float cos_fov, float log_scale, int nlevels, int F, int scaled, const float* sf,
  int* q_frame, float* qx, float* qy, float* qr, int* qmin, int* qmax, float* angle, int* level) {
  CmsProjectKfArgs a; a.n=n; a.pt_job=pt_job; a.pose12=pose12; a.job_frame=job_frame; a.job_kp0=job_kp0; a.kf_kp=kf_kp; a.kf_feat=kf_feat; a.kf_angle=kf_angle;
  a.pos=pos; a.min_dist=mn; a.max_dist=mx; a.th=th; a.cos_fov=cos_fov; a.log_scale=log_scale; a.nlevels=nlevels; a.F=F; a.bounds_scaled=scaled;
  for (int l=0;l<16;++l) a.sf[l]= l<nlevels? sf[l]:0.f;
  a.q_frame=q_frame; a.qx=qx; a.qy=qy; a.qr=qr; a.qmin=qmin; a.qmax=qmax; a.angle=angle; a.level=level;
  blockDim.x=256;
  for (int b=0;b<(n+255)/256;++b) for (int t=0;t<256;++t) { blockIdx.x=b; threadIdx.x=t; k_project_keyframe(a); }
}
