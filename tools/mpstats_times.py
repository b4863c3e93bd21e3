"""Time of the map-point statistics entries on the device against the host build of the same core on one thread.

On maps of --small and --keyframes key frames x --features features with prof_covis's tracked observation pattern (tools/prof_mappoints.py's
tracked_map), per entry:

  culling   cms_mpstore_culling of --recent recent points (apply = 0, so that every repetition sees the same table) against hm_mpstats_culling
  median    cms_kfstore_scene_median_depth of --slots slots, q = 2, against hm_mpstats_scene_median_depth
  tracked   cms_covis_tracked_map_points of --members jobs (members in turn) against hm_mpstats_tracked_map_points
  count     ONE cms_mpstore_count for --frames frames x --ids ids with flags, followed by cms_mpstore_fetch_stats of one row (the call is
            asynchronous: the fetch waits for it on the device), against hm_mpstats_count; the fetch alone is timed next to it

Every figure is timed host to host around the library call(s) with the arguments laid out beforehand: the median of --reps calls after a warm-up,
p10 / p90 in brackets.  Before timing, the device's answers are compared with the host core's.  Writes profiles/mpstats.md (or --out).

    python tools/mpstats_times.py [--reps 20] [--keyframes 1000] [--small 60] [--features 2000] [--out profiles/mpstats.md]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from cubemapslam_amd import api, synth  # noqa: E402
import mpstats_hostlib as hl  # noqa: E402
from prof_covis import median_of  # noqa: E402
from prof_mappoints import fmt, tracked_map  # noqa: E402

p = api._p


def figures(cg, fctx, K, F, a, out):
    rng = np.random.default_rng(K)
    rows, octs, P = tracked_map(rng, K, F)
    R = [hl.sc.rotation(1000 + s) for s in range(K)]
    t = rng.normal(0, 3, (K, 3)).astype(np.float32)
    st = api.KeyframeStore(cg, max_keyframes=K, max_features=F, max_nodes=8)
    dev = hl.DeviceBackend(st, [fctx], K, P)
    host = hl.HostBackend(K, F, P)
    for b in (dev, host):
        for s in range(K):
            b.put(s, rows[s], octs[s], R[s], t[s])
        b.build(np.arange(K))
    seen = np.unique(np.concatenate([r[r >= 0] for r in rows]))
    pos = rng.normal(0, 5, (P, 3)).astype(np.float32)
    first = rng.integers(0, K, len(seen)).astype(np.int32)
    visible = rng.integers(1, 50, len(seen)); found = rng.integers(0, 30, len(seen))
    for b in (dev, host):
        b.set(seen, pos[seen], np.zeros(len(seen), np.int32))
        b.set_stats(seen, first_kf=first, visible=visible, found=found)
    L, H = api.lib(), hl.H()
    i32 = lambda v: np.ascontiguousarray(v, np.int32)
    # ---- culling: the points of the last key frames, as mlpRecentAddedMapPoints holds them
    recent = i32(np.unique(np.concatenate([r[r >= 0] for r in rows[K - 3:]]))[:a.recent])
    off = i32([0, len(recent)]); cur = i32([K])
    vd = np.zeros(len(recent), np.uint8); vh = np.zeros(len(recent), np.uint8)

    def d_cull():
        assert L.cms_mpstore_culling(dev.mp.h, dev.cv.h, 1, p(off), p(recent), p(cur), 2, 0, p(vd)) == 0

    def h_cull():
        assert H.hm_mpstats_culling(host.h, 1, p(off), p(recent), p(cur), 2, 0, p(vh)) == 0
    d_cull(); h_cull()
    assert np.array_equal(vd, vh)
    out.append("| %d x %d | culling | %d recent points | %s | %s |" % (K, F, len(recent), fmt(median_of(d_cull, a.reps)), fmt(median_of(h_cull, a.reps))))
    # ---- median depth of the key frame and its neighbours
    slots = i32(np.arange(K - min(a.slots, K), K))
    dd = np.zeros(len(slots), np.float32); dh = np.zeros(len(slots), np.float32); nd = np.zeros(len(slots), np.int32); nh = np.zeros(len(slots), np.int32)

    def d_med():
        assert L.cms_kfstore_scene_median_depth(st.h, dev.mp.h, len(slots), p(slots), 2, 0, p(dd), p(nd)) == 0

    def h_med():
        assert H.hm_mpstats_scene_median_depth(host.h, len(slots), p(slots), 2, 0, p(dh), p(nh)) == 0
    d_med(); h_med()
    assert np.array_equal(dd.view(np.uint32), dh.view(np.uint32)) and np.array_equal(nd, nh)
    out.append("| %d x %d | median depth | %d slots, %d depths | %s | %s |" % (K, F, len(slots), int(nd.sum()), fmt(median_of(d_med, a.reps)), fmt(median_of(h_med, a.reps))))
    # ---- tracked map points
    members = i32(np.arange(a.members) % K); min_obs = i32(np.full(a.members, 3))
    cd = np.zeros(a.members, np.int32); ch = np.zeros(a.members, np.int32)

    def d_trk():
        assert L.cms_covis_tracked_map_points(dev.cv.h, fctx.h, a.members, p(members), p(min_obs), p(cd)) == 0

    def h_trk():
        assert H.hm_mpstats_tracked_map_points(host.h, a.members, p(members), p(min_obs), p(ch)) == 0
    d_trk(); h_trk()
    assert np.array_equal(cd, ch)
    out.append("| %d x %d | tracked count | %d jobs | %s | %s |" % (K, F, a.members, fmt(median_of(d_trk, a.reps)), fmt(median_of(h_trk, a.reps))))
    # ---- one count call for all frames of a tick
    T = a.frames * a.ids
    foff = i32(np.arange(a.frames + 1) * a.ids)
    fids = i32(np.where(rng.random(T) < 0.9, rng.choice(seen, T), -1)); flag = (rng.random(T) < 0.7).astype(np.uint8)
    one = i32(seen[:1]); o = [np.zeros(1, np.int32) for _ in range(3)]

    def d_fetch():
        assert L.cms_mpstore_fetch_stats(dev.mp.h, 1, p(one), p(o[0]), p(o[1]), p(o[2])) == 0

    def d_cnt():
        assert L.cms_mpstore_count(dev.mp.h, fctx.h, 1, a.frames, p(foff), p(fids), p(flag), 1) == 0
        d_fetch()

    def d_cnt_call():
        assert L.cms_mpstore_count(dev.mp.h, fctx.h, 1, a.frames, p(foff), p(fids), p(flag), 1) == 0

    def h_cnt():
        assert H.hm_mpstats_count(host.h, 1, a.frames, p(foff), p(fids), p(flag), 1) == 0
    t_d = median_of(d_cnt, a.reps); t_h = median_of(h_cnt, a.reps)      # (the same number of calls on both sides)
    assert all(np.array_equal(x, y) for x, y in zip(dev.fetch_stats(seen), host.fetch_stats(seen)))
    t_f = median_of(d_fetch, a.reps); t_c = median_of(d_cnt_call, a.reps)
    d_fetch()
    out.append("| %d x %d | count + fetch of one row | %d frames x %d ids | %s | %s |" % (K, F, a.frames, a.ids, fmt(t_d), fmt(t_h)))
    out.append("| %d x %d | (the fetch alone) | | %s | |" % (K, F, fmt(t_f)))
    out.append("| %d x %d | (the count call's return, asynchronous) | | %s | |" % (K, F, fmt(t_c)))
    host.close(); dev.close(); st.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20); ap.add_argument("--keyframes", type=int, default=1000); ap.add_argument("--small", type=int, default=60)
    ap.add_argument("--features", type=int, default=2000); ap.add_argument("--recent", type=int, default=200); ap.add_argument("--slots", type=int, default=21)
    ap.add_argument("--members", type=int, default=256); ap.add_argument("--frames", type=int, default=256); ap.add_argument("--ids", type=int, default=1500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpstats.md"))
    a = ap.parse_args()
    cg = api.Context(synth.camera("lafida", 550), nfeatures=2000, max_batch=1)
    fctx = api.Context(synth.camera("lafida", 550), nfeatures=2000, max_batch=1)
    rows = []
    for K in (a.small, a.keyframes):
        figures(cg, fctx, K, a.features, a, rows)
    text = ["# Map-point statistics on the device against the host core", "",
            "Written by `tools/mpstats_times.py --reps %d`: medians of %d calls after a warm-up, host to host, p10 .. p90 in brackets." % (a.reps, a.reps),
            "`device`: the C-ABI entry.  `host core`: the host build of `csrc/cms_mpstats_core.h` (`hm_mpstats_*`) on one thread, on the same data.", "",
            "| map | entry | input | device | host core |", "|---|---|---|---|---|"] + rows + [""]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    print("\n".join(text))
    fctx.close(); cg.close()


if __name__ == "__main__":
    main()
