"""Host-to-host time of ORBMatcher::SearchBySim3 on the device (cms_kfstore_search_by_sim3): the call is synchronous, so the wall clock around the
library call covers staging, the copies up, the four launches, the copy back and the synchronisation.  The argument arrays are laid out once,
outside the clock: what is timed is the C entry, not the Python wrapper.  The shapes, warmed up, >= 50 repetitions:

  one job of 2000 against 2000 key points (one accepted hypothesis of LoopClosing::ComputeSim3)
  8 jobs in one call (the current key frame against 8 candidates)
  cms_kfstore_fuse_search over the same number of entries (4000 and 32000 map points), for scale: the search half of Fuse has the same launches
  in front of its scan

    python tools/prof_sim3_search.py [--reps 200] [--out FILE.json]

Kernel time: run the same under `rocprofv3 --kernel-trace --stats -d DIR -o sim3s -- python tools/prof_sim3_search.py` (k_sim3s_project, k_area_query,
k_area_lists, k_sim3s_scan, k_sim3s_agree)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cubemapslam_amd import api, synth  # noqa: E402

F = 550
N = 2000


def flipped(d, rng, flips=6):
    d = d.copy()
    f = rng.integers(0, 256, (len(d), flips))
    for j in range(flips):
        d[np.arange(len(d)), f[:, j] >> 3] ^= (1 << (f[:, j] & 7)).astype(np.uint8)
    return d


def keyframe(rng, P, base, level):
    """a key frame at the identity pose that sees the points P (its camera coordinates) at their projections, a pixel or so off"""
    _, u, v = synth.rays_to_cubemap(F, P)
    ok = u >= 0
    return dict(x=np.where(ok, u + rng.uniform(-1.5, 1.5, N), F + 5.0).astype(np.float32), y=np.where(ok, v + rng.uniform(-1.5, 1.5, N), F + 5.0).astype(np.float32),
                octave=level.astype(np.int32), angle=np.zeros(N, np.float32), desc=flipped(base, rng), rays=np.zeros((N, 3), np.float32), mp=np.arange(N, dtype=np.int32),
                R=np.eye(3, dtype=np.float32), t=np.zeros(3, np.float32), Ow=np.zeros(3, np.float32), median_depth=1.0, node_id=np.zeros(0, np.int32),
                node_off=np.zeros(1, np.int32), node_feat=np.zeros(0, np.int32))


def map_points(rng, P, seen_from, base, level):
    """one map point per key point: position P, distance members that predict `level` at the distance it has in the OTHER camera"""
    mx = (np.linalg.norm(seen_from, axis=1) * 1.2 ** (level - 0.5)).astype(np.float32)
    return dict(skip=np.zeros(N, np.uint8), pos=P.astype(np.float32), min_dist=(mx / np.float32(1.2 ** 7)).astype(np.float32), max_dist=mx, desc=flipped(base, rng),
                normal=(P / np.linalg.norm(P, axis=1, keepdims=True)).astype(np.float32))


def candidate(rng, X, base, level):
    """a loop candidate: a similarity from its camera to key frame 1's, the N physical points as its own (drifted) map has them"""
    s12 = np.float32(rng.uniform(0.8, 1.25))
    R12 = synth._rot(rng.normal(0, 1, 3), rng.uniform(0.05, 0.2)).astype(np.float32)
    t12 = rng.uniform(-0.3, 0.3, 3).astype(np.float32)
    Y = (X - t12.astype(np.float64)) @ R12.astype(np.float64) / float(s12)                      # sR21 X + t21
    return dict(s12=s12, R12=R12, t12=t12, kf2=keyframe(rng, Y, base, level), mp1=map_points(rng, X, Y, base, level), mp2=map_points(rng, Y, X, base, level))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    camd = synth.camera("lafida", F)
    cg = api.Context(camd, nfeatures=2000, max_batch=1)               # the store's context
    ctx = api.Context(camd, nfeatures=2000, max_batch=1)              # the loop-closing thread's
    st = api.KeyframeStore(cg, max_keyframes=9, max_features=2048, max_nodes=8)
    X = np.stack([rng.uniform(-0.9, 0.9, N), rng.uniform(-0.9, 0.9, N), np.ones(N)], 1) * rng.uniform(2.0, 9.0, (N, 1))
    base = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    level = rng.integers(0, 8, N)
    K1, keep1 = api.make_keyframe(keyframe(rng, X, base, level))
    st.put(0, K1)                                                     # the current key frame: key frame 1 of every job
    cands = [candidate(rng, X, base, level) for _ in range(8)]
    keep = []
    for c, cd in enumerate(cands):
        K2, k2 = api.make_keyframe(cd["kf2"])
        keep.append(k2)
        st.put(1 + c, K2)
    L = api.lib()
    p = lambda v: v.ctypes.data_as(C.c_void_p)
    res = {}

    def sim3_call(njobs):
        jobs = [dict(slot1=0, slot2=1 + c, s12=cands[c]["s12"], R12=cands[c]["R12"], t12=cands[c]["t12"], mp1=cands[c]["mp1"], mp2=cands[c]["mp2"]) for c in range(njobs)]
        first = st.search_by_sim3(ctx, jobs, z_as_written=False)      # through the wrapper once: declares the entry's argument types, gives the counts
        arr = (api.Sim3SearchJob * njobs)()
        parts = []
        for c, (q, j) in enumerate(zip(arr, jobs)):
            q.slot1 = 0; q.n1 = N; q.slot2 = 1 + c; q.n2 = N; q.s12 = float(j["s12"]); q.off1 = 2 * N * c; q.off2 = 2 * N * c + N
            q.R12[:] = [float(x) for x in j["R12"].reshape(9)]; q.t12[:] = [float(x) for x in j["t12"]]
            parts += [j["mp1"], j["mp2"]]
        cat = lambda k: np.ascontiguousarray(np.concatenate([m[k] for m in parts]))
        arrs = [cat("skip"), cat("pos"), cat("min_dist"), cat("max_dist"), cat("desc")]
        idx2 = np.zeros(N * njobs, np.int32); nf = np.zeros(njobs, np.int32)
        ptrs = [p(v) for v in arrs] + [p(idx2), p(nf)]

        def call():
            rc = L.cms_kfstore_search_by_sim3(st.h, ctx.h, njobs, arr, 2 * N * njobs, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], 7.5, 0, ptrs[5], ptrs[6])
            assert rc == 0, rc
        call()
        assert [int(v) for v in nf] == [g[1] for g in first]
        return call, int(nf.sum()), (arr, arrs, idx2, nf)

    def fuse_call(njobs):
        """the same number of entries through the search half of Fuse: per job the candidate's own map points, twice, into the candidate's key frame"""
        slots = np.arange(1, 1 + njobs, dtype=np.int32)
        off = (2 * N * np.arange(njobs + 1)).astype(np.int32)
        parts = [m for c in range(njobs) for m in (cands[c]["mp2"], cands[c]["mp2"])]
        cat = lambda k: np.ascontiguousarray(np.concatenate([m[k] for m in parts]))
        arrs = [cat("skip"), cat("pos"), cat("normal"), cat("min_dist"), cat("max_dist"), cat("desc")]
        bi = np.zeros(2 * N * njobs, np.int32); bd = np.zeros(2 * N * njobs, np.int32)
        ptrs = [p(slots), p(off)] + [p(v) for v in arrs] + [p(bi), p(bd)]

        def call():
            rc = L.cms_kfstore_fuse_search(st.h, njobs, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], ptrs[6], ptrs[7], 7.5, ptrs[8], ptrs[9])
            assert rc == 0, rc
        call()
        return call, int((bi >= 0).sum()), (slots, off, arrs, bi, bd)

    for name, make, nj in (("sim3_one_job_2000x2000", sim3_call, 1), ("sim3_8_jobs_one_call", sim3_call, 8), ("fuse_search_4000_entries", fuse_call, 1),
                           ("fuse_search_32000_entries", fuse_call, 8)):
        call, found, hold = make(nj)
        res[name] = dict(timed(call, a.reps), jobs=nj, entries=2 * N * nj, n_found=found)
    for k, v in res.items():
        print("%-30s median %8.1f us  p10 %8.1f  p90 %8.1f  (entries %d, found %d)" % (k, v["median_us"], v["p10_us"], v["p90_us"], v["entries"], v["n_found"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    st.close(); ctx.close(); cg.close()


if __name__ == "__main__":
    main()
