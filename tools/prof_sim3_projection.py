"""Host-to-host time of loop closing's two projection matchers on the device (cms_kfstore_search_by_projection_sim3, cms_kfstore_fuse_search_sim3): the
calls are synchronous, so the wall clock around the library call covers staging, the copies up, the launches, the copy back and the
synchronisation.  The argument arrays are laid out once, outside the clock: what is timed is the C entry, not the Python wrapper.  The shapes,
warmed up, the median of >= 20 repetitions:

  (a) SearchByProjection(Scw): one job, 1031 key points, 1543 and 4001 map points (the last step of LoopClosing::ComputeSim3)
  (b) Fuse(Scw): 30 jobs over one 4001-point set in ONE call (LoopClosing::SearchAndFuse over the current key frame and its covisibles), against
      30 single-job calls

Next to them the host build of the shared chain (hm_sim3p_project: decomposition and projection of the same points, no window query and no scan --
the only host code of these functions in the tree), and the rounds k_sim3p_greedy needed on the seeded test cases.

    python tools/prof_sim3_projection.py [--reps 50] [--out FILE.json]

Kernel time: run the same under `rocprofv3 --kernel-trace --stats -d DIR -o sim3p -- python tools/prof_sim3_projection.py` (k_sim3p_project,
k_area_query, k_area_lists, k_sim3p_greedy, k_sim3p_scan)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cubemapslam_amd import api, synth  # noqa: E402
import sim3_projection_cases as cases  # noqa: E402
import sim3_projection_hostlib as host  # noqa: E402


def timed(fn, reps, warm=10):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e6 * (time.perf_counter() - t0))
    t = np.array(t)
    return dict(reps=reps, median_us=float(np.median(t)), p10_us=float(np.percentile(t, 10)), p90_us=float(np.percentile(t, 90)), min_us=float(t.min()), max_us=float(t.max()))


def put(st, slot, kf):
    n = len(kf["kx"])
    K, keep = api.make_keyframe(dict(x=kf["kx"], y=kf["ky"], octave=kf["koct"], angle=np.zeros(n, np.float32), desc=kf["kdesc"], rays=np.zeros((n, 3), np.float32),
                                     mp=np.full(n, -1, np.int32), R=kf["pose12"][:9].reshape(3, 3), t=kf["pose12"][9:], Ow=np.zeros(3, np.float32), median_depth=1.0,
                                     node_id=np.zeros(0, np.int32), node_off=np.zeros(1, np.int32), node_feat=np.zeros(0, np.int32)))
    st.put(slot, K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 20
    cg = api.Context(cases.CAMD, nfeatures=2000, max_batch=1)         # the store's context
    ctx = api.Context(cases.CAMD, nfeatures=2000, max_batch=1)        # the loop-closing thread's
    st = api.KeyframeStore(cg, max_keyframes=30, max_features=2048, max_nodes=8)
    L = api.lib()
    p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
    res = {}

    def entry_call(greedy, sets, jobs, th):
        """-> (call, hits) over prepared arrays"""
        first = (st.search_by_projection_sim3 if greedy else st.fuse_search_sim3)(ctx, sets, jobs, th=th)      # through the wrapper once: declares the argument types
        soff, arrs, arr, eoff, skip = st._sim3_proj_args(sets, jobs)
        E = int(eoff[-1])
        o1 = np.zeros(E, np.int32); o2 = np.zeros(max(E, len(jobs)), np.int32)
        taken = np.ascontiguousarray(np.concatenate([np.asarray(j["taken"], np.uint8) for j in jobs]))
        hold = (soff, arrs, arr, skip, taken, o1, o2)
        if greedy:
            def call():
                rc = L.cms_kfstore_search_by_projection_sim3(st.h, ctx.h, len(sets), p(soff), *[p(v) for v in arrs], len(jobs), arr, p(skip), p(taken), float(th), p(o1), p(o2))
                assert rc == 0, rc
        else:
            def call():
                rc = L.cms_kfstore_fuse_search_sim3(st.h, ctx.h, len(sets), p(soff), *[p(v) for v in arrs], len(jobs), arr, p(skip), float(th), p(o1), p(o2))
                assert rc == 0, rc
        call()
        assert np.array_equal(o1, np.concatenate([g[0] for g in first]))
        return call, int((o1 >= 0).sum()), hold

    def host_chain(c, th):
        pts = c["pts"]
        return lambda: host.project(cases.F, c["Scw"], pts["pos"], pts["normal"], pts["min_dist"], pts["max_dist"], th, c["sf"])

    # ---- (a) SearchByProjection: one job
    for npts in (1543, 4001):
        c = cases.seeded(1031, npts, 333 if npts == 1543 else 334)
        put(st, 0, c["kf"])
        job = dict(slot=0, n=len(c["kf"]["kx"]), Scw=c["Scw"], set=0, skip=c["skip"], taken=c["taken"])
        call, hits, hold = entry_call(True, [c["pts"]], [job], 10.0)
        res["search_by_projection_1031kp_%dpts" % npts] = dict(timed(call, a.reps), jobs=1, entries=npts, hits=hits, greedy_rounds=int(L.cms_sim3_proj_last_rounds()))
        res["host_chain_only_%dpts" % npts] = dict(timed(host_chain(c, 10.0), a.reps), entries=npts)
    # ---- (b) Fuse: 30 key frames (the 4001-point case's key frame under 30 nearby similarities) over one set
    rng = np.random.default_rng(5)
    jobs = []
    for s in range(30):
        put(st, s, c["kf"])
        S = c["Scw"].astype(np.float64).copy()
        S[:, :3] = synth._rot(rng.normal(0, 1, 3), rng.uniform(0.0, 0.03)) @ S[:, :3]
        S[:, 3] += rng.uniform(-0.02, 0.02, 3)
        jobs.append(dict(slot=s, n=len(c["kf"]["kx"]), Scw=S.astype(np.float32), set=0, skip=c["skip"], taken=c["taken"]))
    call, hits, hold = entry_call(False, [c["pts"]], jobs, 4.0)
    res["fuse_30_jobs_one_call"] = dict(timed(call, a.reps), jobs=30, entries=30 * 4001, hits=hits)
    singles = [entry_call(False, [c["pts"]], [j], 4.0) for j in jobs]

    def thirty():
        for one, _, _ in singles:
            one()
    res["fuse_30_single_job_calls"] = dict(timed(thirty, a.reps), jobs=30, entries=30 * 4001, hits=sum(h for _, h, _ in singles))
    res["host_chain_only_30x4001pts"] = dict(timed(lambda: [host.project(cases.F, j["Scw"], c["pts"]["pos"], c["pts"]["normal"], c["pts"]["min_dist"], c["pts"]["max_dist"], 4.0,
                                                                         c["sf"]) for j in jobs], max(a.reps // 2, 20)), entries=30 * 4001)
    # ---- the greedy kernel's rounds on the seeded test cases
    rounds = {}
    for name, cc in [("seeded_%d" % len(q["kf"]["kx"]), q) for q in cases.family()] + [("dense", cases.dense_case())]:
        put(st, 0, cc["kf"])
        info = {}
        cases.run_sbp(cc, info)
        st.search_by_projection_sim3(ctx, [cc["pts"]], [dict(slot=0, n=len(cc["kf"]["kx"]), Scw=cc["Scw"], set=0, skip=cc["skip"], taken=cc["taken"])], th=cc["th"])
        rounds[name] = dict(greedy_rounds=int(L.cms_sim3_proj_last_rounds()), restatement_chain_depth=info["depth"], entries=len(cc["skip"]))
    res["greedy_rounds"] = rounds
    for k, v in res.items():
        if "median_us" in v:
            print("%-40s median %9.1f us  p10 %9.1f  p90 %9.1f  (entries %d%s)" % (k, v["median_us"], v["p10_us"], v["p90_us"], v["entries"],
                                                                                    ", hits %d" % v["hits"] if "hits" in v else ""), flush=True)
    for k, v in rounds.items():
        print("%-40s %d rounds (chain depth of the restatement %d, %d entries)" % ("greedy " + k, v["greedy_rounds"], v["restatement_chain_depth"], v["entries"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    st.close(); ctx.close(); cg.close()


if __name__ == "__main__":
    main()
