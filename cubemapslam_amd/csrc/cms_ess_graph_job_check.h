// cms_ess_graph_job_check.h -- what cms_essential_graph_optimize checks per job before anything is enqueued or written, and the structure of a
// job's linear system (incidence lists, row envelope, column lists).  Host code, shared by the C-ABI entry (cms_api_ess_graph.hip) and the host loop
// (host/ess_graph_host.cpp), so both refuse the same records with the same words and factor inside the same envelope.  Needs cms_ess_graph_job
// (include/cubemapslam_hip.h) before it.
#pragma once
#include <vector>

// NULL or the reason
static inline const char* cms_ess_graph_check_job(const cms_ess_graph_job& q) {
  if (q.N < 1) return "N < 1";
  if (q.E < 0) return "E < 0";
  if (!q.Scw || !q.Snc || !q.S_out || !q.Tiw_out || (q.E > 0 && !q.edges)) return "a null array";
  if (q.fixed < 0 || q.fixed >= q.N) return "fixed out of range";
  if (q.iterations < 0) return "iterations < 0";
  if (!(q.lambda_init > 0.0) || !(q.lambda_init - q.lambda_init == 0.0)) return "lambda_init not positive and finite";
  for (int e = 0; e < q.E; ++e) {
    const int v0 = q.edges[3 * e], v1 = q.edges[3 * e + 1], kind = q.edges[3 * e + 2];
    if (v0 < 0 || v0 >= q.N || v1 < 0 || v1 >= q.N) return "an edge index out of range";
    if (v0 == v1) return "an edge with v0 == v1";
    if (kind != 0 && kind != 1) return "an edge kind outside {0, 1}";
  }
  for (int pass = 0; pass < 2; ++pass) {
    const double* S = pass ? q.Snc : q.Scw;
    for (int i = 0; i < 8 * q.N; ++i)
      if (!(S[i] - S[i] == 0.0)) return "a non-finite entry";
    for (int v = 0; v < q.N; ++v)
      if (!(S[8 * v + 7] > 0.0)) return "a scale <= 0";
  }
  // every vertex needs a path to `fixed`: a union-find over the edges (the reference's spanning tree excludes the other case; g2o would factor a
  // singular matrix there)
  std::vector<int> parent((size_t)q.N);
  for (int v = 0; v < q.N; ++v) parent[(size_t)v] = v;
  auto find = [&](int v) {
    while (parent[(size_t)v] != v) { parent[(size_t)v] = parent[(size_t)parent[(size_t)v]]; v = parent[(size_t)v]; }
    return v;
  };
  for (int e = 0; e < q.E; ++e) {
    const int a = find(q.edges[3 * e]), b = find(q.edges[3 * e + 1]);
    if (a != b) parent[(size_t)(a > b ? a : b)] = a > b ? b : a;
  }
  const int root = find(q.fixed);
  for (int v = 0; v < q.N; ++v)
    if (find(v) != root) return "a vertex with no path to fixed";
  return nullptr;
}

struct CmsEgStructure {
  std::vector<int> inc_off, inc, first, colp, coli;
  std::vector<long long> rowp;
  long long blocks = 0;
};
// the free index of a vertex that is not `fixed`: the unknowns are the non-fixed vertices in ascending vertex index
static inline int cms_eg_free_of(int v, int fixed) { return v - (v > fixed ? 1 : 0); }
// only `first` and the block count: what the entry needs to refuse a call whose envelopes exceed the handle's
static inline long long cms_eg_envelope(int N, int fixed, int E, const int* edges, std::vector<int>& first) {
  const int Nf = N - 1;
  first.resize((size_t)Nf);
  for (int f = 0; f < Nf; ++f) first[(size_t)f] = f;
  for (int e = 0; e < E; ++e) {
    const int v0 = edges[3 * e], v1 = edges[3 * e + 1];
    if (v0 == fixed || v1 == fixed) continue;
    const int a = cms_eg_free_of(v0, fixed), b = cms_eg_free_of(v1, fixed);
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    if (lo < first[(size_t)hi]) first[(size_t)hi] = lo;
  }
  long long blocks = 0;
  for (int f = 0; f < Nf; ++f) blocks += f - first[(size_t)f] + 1;
  return blocks;
}
static inline void cms_eg_structure(int N, int fixed, int E, const int* edges, CmsEgStructure& s) {
  const int Nf = N - 1;
  s.inc_off.assign((size_t)N + 1, 0);
  for (int e = 0; e < E; ++e) { ++s.inc_off[(size_t)edges[3 * e] + 1]; ++s.inc_off[(size_t)edges[3 * e + 1] + 1]; }
  for (int v = 0; v < N; ++v) s.inc_off[(size_t)v + 1] += s.inc_off[(size_t)v];
  s.inc.assign(2 * (size_t)E, 0);
  std::vector<int> at(s.inc_off.begin(), s.inc_off.end() - 1);
  for (int e = 0; e < E; ++e)
    for (int k = 0; k < 2; ++k) s.inc[(size_t)at[(size_t)edges[3 * e + k]]++] = e;      // ascending e per vertex
  s.blocks = cms_eg_envelope(N, fixed, E, edges, s.first);
  s.rowp.assign((size_t)Nf, 0);
  s.colp.assign((size_t)Nf + 1, 0);
  long long at_block = 0;
  for (int f = 0; f < Nf; ++f) {
    s.rowp[(size_t)f] = at_block;
    at_block += f - s.first[(size_t)f] + 1;
    for (int j = s.first[(size_t)f]; j < f; ++j) ++s.colp[(size_t)j + 1];
  }
  for (int j = 0; j < Nf; ++j) s.colp[(size_t)j + 1] += s.colp[(size_t)j];
  s.coli.assign((size_t)(s.blocks - Nf), 0);
  std::vector<int> cat(s.colp.begin(), s.colp.end() - 1);
  for (int f = 0; f < Nf; ++f)      // ascending rows per column
    for (int j = s.first[(size_t)f]; j < f; ++j) s.coli[(size_t)cat[(size_t)j]++] = f;
}
