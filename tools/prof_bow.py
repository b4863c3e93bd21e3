"""Host-to-host time of ORBMatcher::SearchByBoW on the device (cms_search_by_bow / cms_kfstore_search_by_bow, and cms_kfstore_search_by_bow_keyframes
for the (KeyFrame, KeyFrame) overload): each call is synchronous, so the wall clock around it covers staging, the copy up, the launch, the copy back
and the synchronisation.  The shapes, warmed up, >= 50 repetitions:

  one job of 2000 against 2000 features (TrackReferenceKeyFrame), resident and stand-alone
  32 jobs in one call (Relocalization's candidate loop: ~4 candidates for each of 8 frames)
  one job whose frame holds 16383 key points (the frame grid's limit)
  key frame against key frame (LoopClosing::ComputeSim3): one job of 2000 against 2000 features, and 8 candidates in one call

    python tools/prof_bow.py [--reps 200] [--out FILE.json]

Kernel time: run the same under `rocprofv3 --kernel-trace --stats -d DIR -o bow -- python tools/prof_bow.py` (k_search_by_bow, k_search_by_bow_kf)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cubemapslam_amd import api, synth  # noqa: E402

KP = api.KP_DTYPE


def feature_set(rng, n, base=None, flips=8):
    """n key points / descriptors; with base: noisy copies of base's descriptors (a second view of the same points) plus fresh ones"""
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if base is not None:
        m = min(n, len(base))
        d[:m] = base[:m]
        f = rng.integers(0, 256, (m, flips))
        for j in range(flips):
            d[np.arange(m), f[:, j] >> 3] ^= (1 << (f[:, j] & 7)).astype(np.uint8)
    k = np.zeros(n, KP)
    k["x"] = rng.uniform(0, 1600, n); k["y"] = rng.uniform(0, 1600, n); k["octave"] = rng.integers(0, 8, n); k["angle"] = rng.uniform(0, 360, n)
    return k, d


def fv_of(d, nodes=100):
    """FeatureVector stand-in: ~20 features per node at 2000 features (DBoW2 level 4 of a 10^6-word vocabulary gives tens per node)"""
    node = (d[:, 0].astype(np.int32) * 256 + d[:, 1]) % nodes
    order = np.lexsort((np.arange(len(d)), node))
    ids, starts = np.unique(node[order], return_index=True)
    return dict(node_id=ids.astype(np.int32), node_off=np.concatenate([starts, [len(d)]]).astype(np.int32), node_feat=order.astype(np.int32))


def timed(fn, reps, warm=10):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e6 * (time.perf_counter() - t0))
    t = np.array(t)
    return dict(reps=reps, median_us=float(np.median(t)), p10_us=float(np.percentile(t, 10)), p90_us=float(np.percentile(t, 90)),
                min_us=float(t.min()), max_us=float(t.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    camd = synth.camera("lafida", 550)
    B = 8
    ctx = api.Context(camd, nfeatures=2000, max_batch=B)              # rows for the 2000-feature frames
    big = api.Context(camd, nfeatures=16347, scale_factor=1.05, nlevels=12, max_batch=1)      # kp_cap = nfeatures + 3 x 12 levels = 16383 (quota per level <= 2045)
    assert big.geom.kp_cap >= 16383, big.geom.kp_cap
    cg = api.Context(camd, nfeatures=2000, max_batch=1)
    st = api.KeyframeStore(cg, max_keyframes=40, max_features=4096, max_nodes=1024)
    kfk, kfd = feature_set(rng, 2000)
    mp = np.where(rng.random(2000) < 0.7, np.arange(2000), -1).astype(np.int32)
    kf = dict(x=kfk["x"], y=kfk["y"], octave=kfk["octave"], angle=kfk["angle"], desc=kfd, rays=np.zeros((2000, 3), np.float32), mp=mp,
              R=np.eye(3, dtype=np.float32), t=np.zeros(3, np.float32), Ow=np.zeros(3, np.float32), median_depth=1.0, **fv_of(kfd))
    K, keep = api.make_keyframe(kf)
    for s in range(32):
        st.put(s, K)
    frames = []
    for b in range(B):
        fk, fd = feature_set(rng, 2000, base=kfd)
        ctx.area_set_keypoints(b, fk); ctx.area_set_descriptors(b, fd)
        frames.append((fk, fd, fv_of(fd)))
    res = {}
    n0 = api.search_by_bow(ctx, 0, 2000, frames[0][2], K)[1]
    res["one_job_2000x2000_standalone"] = dict(timed(lambda: api.search_by_bow(ctx, 0, 2000, frames[0][2], K), a.reps), n_matches=n0)
    job1 = [(0, 0, 2000, frames[0][2], None)]
    res["one_job_2000x2000_resident"] = dict(timed(lambda: st.search_by_bow(ctx, job1), a.reps), n_matches=st.search_by_bow(ctx, job1)[0][1])
    jobs = [(4 * b + c, b, 2000, frames[b][2], None) for b in range(B) for c in range(4)]
    res["relocalisation_32_jobs_resident"] = dict(timed(lambda: st.search_by_bow(ctx, jobs), a.reps), jobs=len(jobs),
                                                  n_matches=int(sum(g[1] for g in st.search_by_bow(ctx, jobs))))
    fk, fd = feature_set(rng, 16383, base=kfd)
    big.area_set_keypoints(0, fk); big.area_set_descriptors(0, fd)
    fvb = fv_of(fd, nodes=800)
    jb = [(0, 0, 16383, fvb, None)]
    res["one_job_16383_frame_keypoints_resident"] = dict(timed(lambda: st.search_by_bow(big, jb), a.reps), n_matches=st.search_by_bow(big, jb)[0][1])
    # LoopClosing::ComputeSim3: the current key frame (slot 0) against 8 loop candidates, second views of the same points with their own map points
    for c in range(8):
        ck, cd = feature_set(rng, 2000, base=kfd)
        cmp_ = np.where(rng.random(2000) < 0.7, np.arange(2000), -1).astype(np.int32)
        cand = dict(kf, x=ck["x"], y=ck["y"], octave=ck["octave"], angle=ck["angle"], desc=cd, mp=cmp_, **fv_of(cd))
        KC, keep_c = api.make_keyframe(cand)
        st.put(32 + c, KC)
    kjob1 = [(0, 2000, 32, 2000, None, None)]
    res["keyframes_one_job_2000x2000"] = dict(timed(lambda: st.search_by_bow_keyframes(ctx, kjob1, nnratio=0.75), a.reps),
                                              n_matches=st.search_by_bow_keyframes(ctx, kjob1, nnratio=0.75)[0][1])
    kjobs = [(0, 2000, 32 + c, 2000, None, None) for c in range(8)]
    res["keyframes_8_jobs_one_call"] = dict(timed(lambda: st.search_by_bow_keyframes(ctx, kjobs, nnratio=0.75), a.reps), jobs=len(kjobs),
                                            n_matches=int(sum(g[1] for g in st.search_by_bow_keyframes(ctx, kjobs, nnratio=0.75))))
    for k, v in res.items():
        print("%-42s median %8.1f us  p10 %8.1f  p90 %8.1f  (n_matches %s)" % (k, v["median_us"], v["p10_us"], v["p90_us"], v["n_matches"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    st.close(); cg.close(); big.close(); ctx.close()


if __name__ == "__main__":
    main()
