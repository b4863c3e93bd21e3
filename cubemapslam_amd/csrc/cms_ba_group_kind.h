// Which windows cms_ba_optimize_many may put into one group, and which of the two slice-summing trial-solve kernels a window runs.
// Plain integers only, no HIP: tests/emu/ba_group_kind_emu.cpp compiles this header with g++ (tests/test_ba_group_kind_cpu.py).
//
// A group's rounds are ONE sequence of launches, so everything that selects a kernel or a launch size which changes a window's sums must be
// equal for all windows of the group -- otherwise a deterministic window's bits depend on its company.  The key below holds exactly those things.
#pragma once
#include <stddef.h>

// LDS the three-lane trial solve needs for np free key frames (the layout comment in ba_trial_solve3_body, cms_ba_fused.hip): L panels
// [np (np - 1) / 2][stride] | diagonal factors [np][36] | W double buffer [2][np][stride] | diag staging [36] | y, 1/D, bp [6 np] each | 8 spare doubles
static inline size_t ba_solve3_lds(int np, int stride) {
  return ((size_t)stride * (size_t)(np * (np - 1) / 2) + 36 * (size_t)np + 2 * (size_t)stride * (size_t)np + 36 + 18 * (size_t)np + 8) * sizeof(double);
}
// ... and with the slices' sums behind it (kb_ba_trial_solve3rp: every thread adds the slices element by element into LDS first): npairs2 x 42 more doubles
static inline size_t ba_solve3_presum_lds(size_t solve3_lds, int npairs2) { return solve3_lds + (size_t)npairs2 * 42 * sizeof(double); }
// Does a window's solve kernel sum the slices into LDS first?  Decided from the window ALONE (its own LDS, its own dense pair count np (np + 1) / 2),
// when it is created: the presummed kernel forms v = s0 + s1 + ... and then a -= v, the other one a -= s0, a -= s1, ... -- different roundings,
// so the choice must not follow from the largest window of whatever group the window is optimised in.
static inline bool ba_solve_presum_fits(bool solve3_ok, size_t solve3_lds, int npairs2, size_t lds_ceiling) {
  return solve3_ok && ba_solve3_presum_lds(solve3_lds, npairs2) <= lds_ceiling;
}

// Does the solve kernel sum a window's slices itself (kb_ba_trial_solve3r / 3rp, slice after slice), or does kb_ba_schur_edges_reduce in a launch of its
// own (four strided partial sums per element, then their sum: a third rounding)?  From the window's OWN slice count -- the workgroups of its share of the
// Schur launch, which for a deterministic window is the same in every group -- and not from the largest count in the group.
static inline bool ba_solve_sums_slices(int own_slices, int solve_reduce_max) { return own_slices <= solve_reduce_max; }

struct BaKindIn {
  int device;
  bool fast_plan;          // planned by ba_plan_fast / the plan kernel: the per-edge arrays exist on the device only
  bool edge_list;          // carries the edge-major work list (se.nchunks > 0)
  bool deterministic;
  // the rest is looked at for deterministic windows only
  bool det_points;         // through the pair-owner kernel instead of the fused chain
  bool has_runs;           // rm_lds > 0: signature runs, the run-major body
  int se_waves;            // wavefronts per Schur workgroup that fit
  int det_ranges;          // workgroups the window is cut into
  bool solve_presum;       // ba_solve_presum_fits
  bool solve_sums_slices;  // ba_solve_sums_slices
};
// Two windows may share a group iff their keys are equal.
static inline int ba_group_kind(const BaKindIn& w) {
  int k = w.device * 8 + (w.fast_plan ? 4 : 0) + (w.edge_list ? 2 : 0) + (w.deterministic ? 1 : 0);
  if (w.deterministic) {
    const int waves = w.se_waves < 0 ? 0 : (w.se_waves > 15 ? 15 : w.se_waves);
    k += 1024 * (1 + (w.det_points ? 1 : 0) + 2 * (w.has_runs ? 1 : 0) + 4 * waves + 64 * w.det_ranges);      // (det_ranges <= 128: below 2^24)
    k += (w.solve_presum ? 1 : 0) << 24;
    k += (w.solve_sums_slices ? 1 : 0) << 25;
  }
  return k;
}
