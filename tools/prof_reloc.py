"""Host-to-host time of Relocalization's guided search on the device, ORBMatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist)
(cms_search_by_projection_keyframe / cms_kfstore_search_by_projection): each call is synchronous, so the wall clock around it covers staging, the
copy up, the five launches, the copy back and the synchronisation.  The shapes are warmed up and then take turns (40 rounds of 100 calls each by
default: 4000 calls and a window of some 0.3 - 3 s per shape), so that a drift of the machine falls on all of them alike:

  one job: one lost stream, ~500 listed points of a resident key frame against a ~1750-key-point frame, th 10 / ORBdist 100 -- resident and stand-alone
  8 jobs in one call: 8 lost streams (8 frame rows, 8 resident key frames), ~500 listed points each, th 10
  the same 8 jobs as 8 calls of one job, for comparison
  one job with th 3 / ORBdist 64 (the second search of Tracking.cpp:1115)

    python tools/prof_reloc.py [--rounds 40] [--block 100] [--out FILE.json]

Kernel time: run the same under `rocprofv3 --kernel-trace --stats -d DIR -o reloc -- python tools/prof_reloc.py --rounds 2 --block 25` (k_project_keyframe,
k_area_query, k_area_lists, k_search_local, k_rot_filter)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cubemapslam_amd import api, synth  # noqa: E402

KP = api.KP_DTYPE
F = 550


def stream_input(seed, listed=500):
    """one lost stream: a key frame and a frame looking at one synthetic scene (synth.keyframe_set), about `listed` of the key frame's map points"""
    ks = synth.keyframe_set(F, n_kf=2, n_pts=2600, seed=seed, with_mp=0.45)
    a, f = ks["kfs"][0], ks["kfs"][1]
    rng = np.random.default_rng(seed + 1)
    feat = np.flatnonzero(a["mp"] >= 0).astype(np.int32)
    if len(feat) > listed:
        feat = np.sort(rng.choice(feat, listed, replace=False)).astype(np.int32)
    pos = ks["X"][a["mp"][feat]].astype(np.float32)
    pose12 = np.concatenate([f["R"].reshape(-1), f["t"]]).astype(np.float32)
    dist = np.linalg.norm(pos.astype(np.float64) - f["Ow"].astype(np.float64), axis=1)
    mx = (6.0 * 1.2 ** (3 - rng.uniform(0.1, 0.9, len(feat)))).astype(np.float32)      # the level the scene's key points were drawn at
    mn = (mx / 1.2 ** 7).astype(np.float32)
    assert dist.min() > 0
    ang = lambda q: ((q["point"] * 37) % 360).astype(np.float32)
    desc = a["desc"][feat].copy()
    fl = rng.integers(0, 256, (len(feat), 6))
    for j in range(6):
        desc[np.arange(len(feat)), fl[:, j] >> 3] ^= (1 << (fl[:, j] & 7)).astype(np.uint8)
    fk = np.zeros(len(f["x"]), KP); fk["x"] = f["x"]; fk["y"] = f["y"]; fk["octave"] = f["octave"]; fk["angle"] = ang(f)
    kf = dict(a, angle=ang(a), rays=np.zeros((len(a["x"]), 3), np.float32))
    return dict(kf=kf, feat=feat, pos=pos, pose12=pose12, min_dist=mn, max_dist=mx, desc=desc, fk=fk, fd=np.ascontiguousarray(f["desc"]), kf_angle=ang(a)[feat])


def timed_interleaved(shapes, rounds, block, warm=20):
    """shapes: {name: callable}.  Every shape is warmed up, then the shapes take turns: `rounds` rounds, in each a block of `block` calls per shape, every
    call timed on its own -- so a drift of the machine during the run falls on all shapes alike, and each shape's window is rounds x block calls long."""
    for fn in shapes.values():
        for _ in range(warm):
            fn()
    t = {k: [] for k in shapes}
    for _ in range(rounds):
        for k, fn in shapes.items():
            for _ in range(block):
                t0 = time.perf_counter()
                fn()
                t[k].append(1e6 * (time.perf_counter() - t0))
    out = {}
    for k, v in t.items():
        v = np.array(v)
        out[k] = dict(calls=len(v), window_ms=float(v.sum() / 1e3), median_us=float(np.median(v)), p10_us=float(np.percentile(v, 10)), p90_us=float(np.percentile(v, 90)),
                      min_us=float(v.min()), max_us=float(v.max()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40, help="rounds in which the shapes take turns")
    ap.add_argument("--block", type=int, default=100, help="calls per shape and round")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B = 8
    camd = synth.camera("lafida", F)
    ctx = api.Context(camd, nfeatures=2400, max_batch=B)
    cg = api.Context(camd, nfeatures=2000, max_batch=1)
    st = api.KeyframeStore(cg, max_keyframes=B, max_features=4096, max_nodes=2048)
    S = [stream_input(100 + b) for b in range(B)]
    keep = []
    for b, s in enumerate(S):
        assert len(s["fk"]) <= ctx.geom.kp_cap
        ctx.area_set_keypoints(b, s["fk"]); ctx.area_set_descriptors(b, s["fd"])
        K, k = api.make_keyframe(s["kf"])
        keep.append(k)
        st.put(b, K)
    ctx.area_grid(B)

    def job(b):
        s = S[b]
        return dict(slot=b, b=b, pose12=s["pose12"], kf_feat=s["feat"], pos=s["pos"], min_dist=s["min_dist"], max_dist=s["max_dist"], desc=s["desc"],
                    kp_mp=np.full(len(s["fk"]), -1, np.int32))

    def resident(bs, th, orb):
        return sum(r[1] for r in st.search_by_projection(ctx, [job(b) for b in bs], th=th, orb_dist=orb, check_orientation=True))

    def alone(b, th, orb):
        s = S[b]
        return ctx.search_by_projection_keyframe(b, s["pose12"], s["kf_angle"], s["pos"], s["min_dist"], s["max_dist"], s["desc"], np.full(len(s["fk"]), -1, np.int32),
                                                 th=th, orb_dist=orb, check_ori=True)[1]

    def eight_calls():
        return sum(resident([b], 10.0, 100) for b in range(B))

    shape = dict(listed=[int(len(s["feat"])) for s in S], frame_keypoints=[int(len(s["fk"])) for s in S])
    shapes = {"one_job_th10_resident": lambda: resident([0], 10.0, 100), "one_job_th10_standalone": lambda: alone(0, 10.0, 100),
              "one_job_th3_resident": lambda: resident([0], 3.0, 64), "eight_jobs_one_call_th10_resident": lambda: resident(range(B), 10.0, 100),
              "eight_calls_of_one_job_th10_resident": eight_calls}
    res = timed_interleaved(shapes, a.rounds, a.block)
    for k, fn in shapes.items():
        res[k]["n_matches"] = int(fn())
    assert res["eight_jobs_one_call_th10_resident"]["n_matches"] == res["eight_calls_of_one_job_th10_resident"]["n_matches"]
    for k, v in res.items():
        print("%-40s median %8.1f us  p10 %8.1f  p90 %8.1f  (%d calls, %.0f ms, n_matches %s)" % (k, v["median_us"], v["p10_us"], v["p90_us"], v["calls"], v["window_ms"],
                                                                                                  v["n_matches"]), flush=True)
    print("listed points per job %s, frame key points %s" % (shape["listed"], shape["frame_keypoints"]), flush=True)
    res["shape"] = shape
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    st.close(); cg.close(); ctx.close()


if __name__ == "__main__":
    main()
