// ba_window_core_emu.cpp -- csrc/cms_ba_window_core.h's host build as a stand-alone program, for sanitizer builds (tests/test_ba_window_cpu.py compiles it
// with -fsanitize=address,undefined).  It reads cases written by ba_window_cases.to_text: the map, the jobs, the caps and the counts the Python
// side got from libcubemapslam_host.so; runs every case with output arrays of exactly njobs x cap entries (a store past a cap is a heap overflow the
// sanitizer reports), once with the case's caps and once with every cap cut to one below the largest count; and checks the counts and the ranges.
//   text format, per case:  case NAME F COSFOV_BITS M MAX_POINTS NPOS NJOBS CAP_KF CAP_POINTS CAP_EDGES
//                           16 x INVSIGMA2_BITS
//                           per member: N, then N x (mp octave X_BITS Y_BITS RAYZ_BITS), then 9 + 3 pose bits
//                           NPOS x (id X_BITS Y_BITS Z_BITS)
//                           per job: N_LOCAL FIRST members...  K N_LOCAL P E
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>
#include "../../cubemapslam_amd/csrc/cms_ba_window_core.h"

static float bits(std::istream& in) { uint32_t u; in >> u; float f; std::memcpy(&f, &u, 4); return f; }

struct Out {
  std::vector<CmsBaWindowCounts> counts; std::vector<int> kf_member, point_id, e_pose, e_point, e_feat; std::vector<double> poses, points, e_obs, e_inv;
  std::vector<uint8_t> fixed; std::vector<int8_t> e_face;
  CmsBaWindowHostOut make(int nj, int ck, int cp, int ce) {
    const size_t Q = (size_t)nj;
    counts.assign(Q, CmsBaWindowCounts{0, 0, 0, 0}); kf_member.assign(Q * ck, -7); point_id.assign(Q * cp, -7); poses.assign(7 * Q * ck, 0); fixed.assign(Q * ck, 9);
    points.assign(3 * Q * cp, 0); e_pose.assign(Q * ce, -7); e_point.assign(Q * ce, -7); e_obs.assign(2 * Q * ce, 0); e_inv.assign(Q * ce, 0); e_face.assign(Q * ce, 9);
    e_feat.assign(Q * ce, -7);
    return CmsBaWindowHostOut{ck, cp, ce, counts.data(), kf_member.data(), point_id.data(), poses.data(), fixed.data(), points.data(), e_pose.data(), e_point.data(),
                              e_obs.data(), e_inv.data(), e_face.data(), e_feat.data()};
  }
};

int main(int argc, char** argv) {
  if (argc < 2) { std::puts("usage: ba_window_core_emu CASES.txt"); return 2; }
  std::ifstream in(argv[1]);
  std::string word, name;
  int ncases = 0;
  while (in >> word) {
    if (word != "case") { std::printf("bad file at '%s'\n", word.c_str()); return 2; }
    CmsBaWindowHostData D;
    int M, max_points, npos, nj, ck, cp, ce;
    in >> name >> D.F; D.cos_fov = bits(in);
    in >> M >> max_points >> npos >> nj >> ck >> cp >> ce;
    for (int l = 0; l < 16; ++l) D.inv_sigma2[l] = bits(in);
    std::vector<std::vector<int>> mp((size_t)M), oct((size_t)M);
    D.kx.resize((size_t)M); D.ky.resize((size_t)M); D.ray_z.resize((size_t)M); D.Rcw.resize(9 * (size_t)M); D.tcw.resize(3 * (size_t)M);
    std::vector<int> n((size_t)M);
    for (int m = 0; m < M; ++m) {
      in >> n[(size_t)m];
      for (int f = 0; f < n[(size_t)m]; ++f) {
        int a, b; in >> a >> b;
        mp[(size_t)m].push_back(a); oct[(size_t)m].push_back(b);
        D.kx[(size_t)m].push_back(bits(in)); D.ky[(size_t)m].push_back(bits(in)); D.ray_z[(size_t)m].push_back(bits(in));
      }
      for (int i = 0; i < 9; ++i) D.Rcw[9 * (size_t)m + (size_t)i] = bits(in);
      for (int i = 0; i < 3; ++i) D.tcw[3 * (size_t)m + (size_t)i] = bits(in);
    }
    D.has_pos.assign((size_t)max_points, 0); D.pos.assign(3 * (size_t)max_points, 0.0f);
    for (int i = 0; i < npos; ++i) { int id; in >> id; D.has_pos[(size_t)id] = 1; for (int c = 0; c < 3; ++c) D.pos[3 * (size_t)id + (size_t)c] = bits(in); }
    std::vector<std::vector<int>> members((size_t)nj);
    std::vector<CmsBaWindowHostJob> jobs((size_t)nj);
    std::vector<CmsBaWindowCounts> want((size_t)nj);
    for (int j = 0; j < nj; ++j) {
      int nl, first; in >> nl >> first;
      members[(size_t)j].resize((size_t)nl);
      for (int k = 0; k < nl; ++k) in >> members[(size_t)j][(size_t)k];
      jobs[(size_t)j] = CmsBaWindowHostJob{nl, members[(size_t)j].data(), first};
      in >> want[(size_t)j].K >> want[(size_t)j].n_local >> want[(size_t)j].P >> want[(size_t)j].E;
    }
    if (!in) { std::printf("%s: truncated\n", name.c_str()); return 2; }
    std::vector<const int*> rows((size_t)M), octs((size_t)M);
    for (int m = 0; m < M; ++m) { rows[(size_t)m] = mp[(size_t)m].data(); octs[(size_t)m] = oct[(size_t)m].data(); }
    CmsCovisHost ix;
    if (ix.build(M, n.data(), rows.data(), octs.data())) { std::printf("%s: the index refuses the rows\n", name.c_str()); return 1; }
    int maxK = 1, maxP = 1, maxE = 1;
    for (int j = 0; j < nj; ++j) { maxK = std::max(maxK, want[(size_t)j].K); maxP = std::max(maxP, want[(size_t)j].P); maxE = std::max(maxE, want[(size_t)j].E); }
    const int caps[2][3] = {{ck, cp, ce}, {std::max(1, maxK - 1), std::max(1, maxP - 1), std::max(1, maxE - 1)}};
    for (int round = 0; round < 2; ++round) {
      Out o;
      std::string why;
      const CmsBaWindowHostOut ho = o.make(nj, caps[round][0], caps[round][1], caps[round][2]);
      const int rc = cms_ba_window_host(ix, D, nj, jobs.data(), ho, &why);
      bool over = false;
      for (int j = 0; j < nj; ++j) {
        const CmsBaWindowCounts& c = o.counts[(size_t)j];
        if (c.K != want[(size_t)j].K || c.n_local != want[(size_t)j].n_local || c.P != want[(size_t)j].P || c.E != want[(size_t)j].E) {
          std::printf("%s round %d job %d: counts %d %d %d %d\n", name.c_str(), round, j, c.K, c.n_local, c.P, c.E);
          return 1;
        }
        over = over || c.K > ho.cap_kf || c.P > ho.cap_points || c.E > ho.cap_edges;
        for (int e = 0; e < std::min(c.E, ho.cap_edges); ++e) {
          const size_t at = (size_t)j * (size_t)ho.cap_edges + (size_t)e;
          if (o.e_pose[at] < 0 || o.e_pose[at] >= c.K || o.e_point[at] < 0 || o.e_point[at] >= c.P || o.e_face[at] < 0 || o.e_face[at] > 4 || o.e_feat[at] < 0) {
            std::printf("%s round %d job %d: edge %d out of range\n", name.c_str(), round, j, e);
            return 1;
          }
        }
      }
      if (rc != (over ? -4 : 0)) { std::printf("%s round %d: code %d (%s)\n", name.c_str(), round, rc, why.c_str()); return 1; }
    }
    ++ncases;
  }
  std::printf("ba_window_core_emu: ok (%d cases)\n", ncases);
  return 0;
}
