// init_host.cpp -- Initializer::InitializeWithRays (src/Initializer.cpp:53-521) on the CPU over the job records of cms_init_two_view: the literal loop,
// one hypothesis after the other, through the host build of csrc/cms_init_core.h.  This is the definition of record the device entry is held to bit
// for bit (tests/test_gpu_init.py), and the stage accessors the CPU tests compare with the numpy restatement.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "cubemapslam_hip.h"
#include "../csrc/cms_init_core.h"
#include "../csrc/cms_init_job_check.h"

namespace {
struct Match { int first, second; };

// CheckRT (:395-499) for one (R, t): vP3D / vbGood sized n1, the selected cosine instead of its acos
int check_rt(int F, float cos_fov, const cms_init_job& q, const std::vector<Match>& m, const std::vector<uint8_t>& inl, const float* R, const float* t, float th2,
             float* vP3D, uint8_t* vbGood, float* cos_sel) {
  std::memset(vP3D, 0, sizeof(float) * 3 * (size_t)q.n1);
  std::memset(vbGood, 0, (size_t)q.n1);
  std::vector<unsigned> keys;
  float O2[3];
  cms_init_o2(R, t, O2);
  int nGood = 0;
  for (size_t i = 0; i < m.size(); ++i) {
    if (!inl[i]) continue;
    float p[3], c;
    int good;
    if (!cms_init_check_rt_match(F, cos_fov, th2, R, t, O2, q.rays1 + 3 * (size_t)m[i].first, q.rays2 + 3 * (size_t)m[i].second, q.keys1 + 2 * (size_t)m[i].first,
                                 q.keys2 + 2 * (size_t)m[i].second, p, &c, &good))
      continue;
    keys.push_back(cms_init_cos_key(c));
    for (int k = 0; k < 3; ++k) vP3D[3 * (size_t)m[i].first + k] = p[k];
    nGood++;
    if (good) vbGood[m[i].first] = 1;
  }
  *cos_sel = 0.0f;
  if (nGood > 0) {
    std::sort(keys.begin(), keys.end());
    const size_t idx = (size_t)std::min(50, (int)keys.size() - 1);
    *cos_sel = cms_init_cos_from_key(keys[idx]);
  }
  return nGood;
}

void two_view_one(int F, float cos_fov, cms_init_job& q) {
  std::vector<Match> m;
  for (int i = 0; i < q.n1; ++i)
    if (q.matches12[i] >= 0) m.push_back({i, q.matches12[i]});
  const int N = (int)m.size();
  // FindEssential (:118-156)
  float score = 0.0f, E21[9] = {0};
  int best = -1;
  std::vector<uint8_t> inliers((size_t)N, 0), cur((size_t)N, 0);
  for (int it = 0; it < q.iterations; ++it) {
    int idx[8];
    cms_init_resolve_draws(N, q.draws + 8 * (size_t)it, idx);
    float At[72], Vt[81], E[9];
    double W[9];
    for (int j = 0; j < 8; ++j) cms_init_fill_row(j, q.rays1 + 3 * (size_t)m[(size_t)idx[j]].first, q.rays2 + 3 * (size_t)m[(size_t)idx[j]].second, At);
    cms_init_e21_from_rows(At, Vt, W, E, nullptr);
    float currentScore = 0;
    for (int i = 0; i < N; ++i) {
      float t1, t2;
      bool a1, a2;
      cur[(size_t)i] = cms_init_check_terms(F, E, q.sigma, q.rays1 + 3 * (size_t)m[(size_t)i].first, q.rays2 + 3 * (size_t)m[(size_t)i].second,
                                            q.keys1 + 2 * (size_t)m[(size_t)i].first, q.keys2 + 2 * (size_t)m[(size_t)i].second, &t1, &a1, &t2, &a2) ? 1 : 0;
      if (a1) currentScore += t1;
      if (a2) currentScore += t2;
    }
    if (currentScore > score) {
      std::memcpy(E21, E, sizeof(E21));
      inliers = cur;
      score = currentScore;
      best = it;
    }
  }
  int n_inliers = 0;
  for (int i = 0; i < N; ++i) n_inliers += inliers[(size_t)i];
  int nGood[4] = {0, 0, 0, 0};
  float cosv[4] = {0, 0, 0, 0}, R1[9] = {0}, R2[9] = {0}, t[3] = {0}, tn[3];
  std::vector<float> p3d(12 * (size_t)q.n1, 0.0f);
  std::vector<uint8_t> good(4 * (size_t)q.n1, 0);
  if (best >= 0) {
    // ReconstructE (:279-303)
    cms_init_decompose_e(E21, R1, R2, t);
    for (int k = 0; k < 3; ++k) tn[k] = -t[k];
    const float th2 = cms_init_th2(q.sigma);
    for (int h = 0; h < 4; ++h)
      nGood[h] = check_rt(F, cos_fov, q, m, inliers, (h & 1) ? R2 : R1, h >= 2 ? tn : t, th2, p3d.data() + (size_t)h * 3 * (size_t)q.n1,
                          good.data() + (size_t)h * (size_t)q.n1, &cosv[h]);
  }
  cms_init_finish_job(q, best, score, n_inliers, nGood, cosv, R1, R2, t, p3d.data(), good.data());
}
}  // namespace

// CamModelGeneral::SetCosFovTh (CamModelGeneral.h:224-229) as the library's cms_cos_fov computes it
extern "C" float hm_init_cos_fov(double fov_deg) {
  const float fov = (float)fov_deg;
  const float pif = 3.1415926535897932384626f;
  return std::cos(fov / 2 * (pif / 180));
}

extern "C" int hm_init_two_view_host(int F, float cos_fov, int njobs, cms_init_job* jobs) {
  if (F <= 0 || njobs < 0 || (njobs > 0 && !jobs)) return CMS_ERR_ARG;
  for (int j = 0; j < njobs; ++j) {
    int N = 0;
    const int rc = cms_init_check_job(jobs[j], &N);
    if (rc) return rc;
  }
  for (int j = 0; j < njobs; ++j) two_view_one(F, cos_fov, jobs[j]);
  return CMS_OK;
}

// ---- stage accessors (tests)
// ComputeE21 on eight ray pairs (8 x 3 each) with every stage handed out
extern "C" void hm_init_compute_e21(const float* rays1, const float* rays2, float* E, CmsInitStages* st) {
  float At[72], Vt[81];
  double W[9];
  for (int j = 0; j < 8; ++j) cms_init_fill_row(j, rays1 + 3 * j, rays2 + 3 * j, At);
  cms_init_e21_from_rows(At, Vt, W, E, st);
}
// CheckEssiential over N matches given as parallel arrays; returns the score, inliers[N]
extern "C" float hm_init_check_essential(int F, const float* E, float sigma, int N, const float* rays1, const float* rays2, const float* keys1, const float* keys2,
                                         uint8_t* inliers, float* terms /* 2N, 0 where not added */) {
  float score = 0;
  for (int i = 0; i < N; ++i) {
    float t1, t2;
    bool a1, a2;
    inliers[i] = cms_init_check_terms(F, E, sigma, rays1 + 3 * i, rays2 + 3 * i, keys1 + 2 * i, keys2 + 2 * i, &t1, &a1, &t2, &a2) ? 1 : 0;
    if (a1) score += t1;
    if (a2) score += t2;
    if (terms) { terms[2 * i] = t1; terms[2 * i + 1] = t2; }
  }
  return score;
}
// CheckRT for a pose of the caller's over a job's matches (all taken as inliers); returns nGood
extern "C" int hm_init_check_rt(int F, float cos_fov, const cms_init_job* q, const float* R, const float* t, float* vP3D, uint8_t* vbGood, float* cos_sel) {
  if (!q) return CMS_ERR_ARG;
  std::vector<Match> m;
  for (int i = 0; i < q->n1; ++i) {
    if (q->matches12[i] >= q->n2) return CMS_ERR_ARG;
    if (q->matches12[i] >= 0) m.push_back({i, q->matches12[i]});
  }
  std::vector<uint8_t> inl(m.size(), 1);
  return check_rt(F, cos_fov, *q, m, inl, R, t, cms_init_th2(q->sigma), vP3D, vbGood, cos_sel);
}
extern "C" void hm_init_decompose_e(const float* E, float* R1, float* R2, float* t) { cms_init_decompose_e(E, R1, R2, t); }
extern "C" void hm_init_triangulate(const float* ray1, const float* ray2, const float* Ra, const float* ta, const float* Rb, const float* tb, float* x3D) {
  cms_init_triangulate(ray1, ray2, Ra, ta, Rb, tb, x3D);
}
extern "C" float hm_init_vector_sigma(int F, float kx, float ky, const float* n) { return cms_init_vector_sigma(F, kx, ky, n[0], n[1], n[2]); }
extern "C" int hm_init_decide(const int* nGood, const float* cosines, int N, float* parallax) { return cms_init_decide(nGood, cosines, N, parallax); }
extern "C" void hm_init_resolve_draws(int N, const int* draws, int* idx) { cms_init_resolve_draws(N, draws, idx); }
extern "C" void hm_init_svd3(const float* A, float* w, float* u, float* vt) { cms_init_svd3(A, w, u, vt); }
extern "C" int hm_init_stages_size() { return (int)sizeof(CmsInitStages); }
