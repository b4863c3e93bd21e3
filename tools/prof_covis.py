"""Time of the covisibility entries on the device against the host build of the same core (csrc/cms_covis_core.h through hm_covis_*) on ONE thread,
for two workloads:

  (a) the tracking side of a large map: --keyframes key frames x --features features with synth's tracked observation pattern (a map point is seen by
      a stretch of consecutive key frames), ONE build, then the votes of --frames frames in one call (each frame holds the live points of one key
      frame's row);
  (b) a key frame's sequence on the mapping thread: build, 2 x connections (ProcessNewKeyFrame and the end of SearchInNeighbors) and one culling
      chain of 20 candidates -- on the large map and on a small one (--small key frames).

Both sides are timed host to host around the library call with the arguments laid out beforehand (no Python list handling inside the timed region);
the device figures include the upload, the launches, the copy back and the wait.  Every timed device result is first compared with the host core's.
Medians over --reps calls after a warm-up, p10 / p90 in brackets.  Writes profiles/covisibility.md (or --out).

    python tools/prof_covis.py [--reps 10] [--keyframes 1000] [--features 2000] [--frames 256] [--small 60] [--out profiles/covisibility.md]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cubemapslam_amd import api, synth  # noqa: E402
import covis_hostlib as hl  # noqa: E402

p = lambda a: a.ctypes.data_as(C.c_void_p)


def median_of(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90))


def tracked_rows(rng, K, F, fill=0.97, lo=3, hi=12):
    """rows[k]: the ids of the map points whose stretch of consecutive key frames covers k, at most F of them, padded with -1 and shuffled"""
    P = int(K * F * fill / ((lo + hi) / 2.0)) + 1
    ids = rng.choice(1 << 30, P, replace=False).astype(np.int64)
    start = rng.integers(-hi, K, P); length = rng.integers(lo, hi + 1, P)
    kf = np.concatenate([np.arange(s, s + n) for s, n in zip(start, length)])
    pt = np.repeat(ids, length)
    ok = (kf >= 0) & (kf < K)
    kf, pt = kf[ok], pt[ok]
    order = np.argsort(kf, kind="stable")
    kf, pt = kf[order], pt[order]
    first = np.searchsorted(kf, np.arange(K + 1))
    rows, octs = [], []
    for k in range(K):
        r = np.full(F, -1, np.int32)
        mine = pt[first[k]:first[k + 1]][:F]
        r[:len(mine)] = mine
        rng.shuffle(r)
        rows.append(r); octs.append(rng.integers(0, 8, F).astype(np.int32))
    return rows, octs


class Pair:
    """one table on the device and on the host core, the raw library calls of both"""

    def __init__(self, fctx, mctx, rows, octs):
        K, F = len(rows), len(rows[0])
        self.K, self.fctx = K, fctx
        self.st = api.KeyframeStore(mctx, max_keyframes=K, max_features=F, max_nodes=8)
        self.dev = hl.DeviceBackend(self.st, fctx, K)
        self.host = hl.HostBackend(K, F)
        for s in range(K):
            self.dev.put(s, rows[s], octs[s]); assert self.host.put(s, rows[s], octs[s]) == 0
        self.slots = np.arange(K, dtype=np.int32)
        self.L, self.H = api.lib(), hl.H()

    def build_dev(self): assert self.L.cms_covis_build(self.dev.cv.h, self.K, p(self.slots)) == 0; self.dev.cv.n_members = self.K
    def build_host(self): assert self.H.hm_covis_build(self.host.h, self.K, p(self.slots)) == 0; self.host.M = self.K

    def build_dev_done(self):
        self.build_dev()
        self.st.ctx.sync()      # (the table is built behind the call: wait for the store's stream)

    def close(self):
        self.dev.close(); self.host.close(); self.st.close()


def sequence(pair, kf, reps):
    """workload (b) for key frame `kf`: build + 2 x connections + one culling chain of 20"""
    K = pair.K
    job = np.array([kf], np.int32)
    w = np.zeros(K, np.int32); order = np.zeros(K, np.int32); nc = np.zeros(1, np.int32)
    pair.build_dev(); pair.build_host()
    assert pair.L.cms_covis_connections(pair.dev.cv.h, 1, p(job), 15, p(w), p(order), p(nc)) == 0
    chain = np.ascontiguousarray(order[:min(int(nc[0]), 20)], np.int32)
    n = len(chain)
    off = np.array([0, n], np.int32); er = np.ones(max(n, 1), np.uint8)
    out = [(np.zeros(K, np.int32), np.zeros(K, np.int32), np.zeros(1, np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint8))
           for _ in range(2)]

    def dev():
        o = out[0]
        pair.build_dev()
        for _ in range(2):
            assert pair.L.cms_covis_connections(pair.dev.cv.h, 1, p(job), 15, p(o[0]), p(o[1]), p(o[2])) == 0
        assert pair.L.cms_covis_culling(pair.dev.cv.h, 1, p(off), p(chain), p(er), 3, p(o[3]), p(o[4]), p(o[5])) == 0

    def host():
        o = out[1]
        pair.build_host()
        for _ in range(2):
            assert pair.H.hm_covis_connections(pair.host.h, 1, p(job), 15, p(o[0]), p(o[1]), p(o[2])) == 0
        assert pair.H.hm_covis_culling(pair.host.h, 1, p(off), p(chain), p(er), 3, p(o[3]), p(o[4]), p(o[5])) == 0
    dev(); host()
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    parts = {}
    for name, fn in (("build", pair.build_dev_done), ("build_host", pair.build_host)):
        parts[name] = median_of(fn, reps)
    return median_of(dev, reps), median_of(host, max(3, reps // 2), warm=1), parts, n, int(nc[0]), int(out[0][5][:n].sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--keyframes", type=int, default=1000)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--small", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covisibility.md"))
    a = ap.parse_args()
    rng = np.random.default_rng(31)
    fctx = api.Context(synth.camera("lafida", 150), nfeatures=500, max_batch=1)
    mctx = api.Context(synth.camera("lafida", 150), nfeatures=500, max_batch=1)
    rows, octs = tracked_rows(rng, a.keyframes, a.features)
    n_obs = int(sum((r >= 0).sum() for r in rows))
    big = Pair(fctx, mctx, rows, octs)
    # ---- (a) one build, the votes of --frames frames in one call
    big.build_dev(); big.build_host()
    frames = [rows[int(k)][rows[int(k)] >= 0] for k in rng.integers(0, a.keyframes, a.frames)]
    off = np.zeros(a.frames + 1, np.int32); off[1:] = np.cumsum([len(f) for f in frames])
    ids = np.ascontiguousarray(np.concatenate(frames), np.int32)
    vd = np.zeros((a.frames, a.keyframes), np.int32); vh = np.zeros((a.frames, a.keyframes), np.int32)
    votes_dev = lambda n: big.L.cms_covis_votes(big.dev.cv.h, fctx.h, n, p(off), p(ids), p(vd))
    votes_host = lambda n: big.H.hm_covis_votes(big.host.h, n, p(off), p(ids), p(vh))
    assert votes_dev(a.frames) == 0 and votes_host(a.frames) == 0 and np.array_equal(vd, vh) and vd.sum() > 0
    t_bd = median_of(big.build_dev_done, a.reps); t_bh = median_of(big.build_host, max(3, a.reps // 2), warm=1)
    t_vd = median_of(lambda: votes_dev(a.frames), a.reps); t_vh = median_of(lambda: votes_host(a.frames), a.reps)
    t_v1d = median_of(lambda: votes_dev(1), a.reps); t_v1h = median_of(lambda: votes_host(1), a.reps)
    # ---- (b) a key frame's sequence, on the large map and on a small one
    seq_big = sequence(big, a.keyframes // 2, a.reps)
    big.close()
    srows, socts = tracked_rows(rng, a.small, a.features)
    small = Pair(fctx, mctx, srows, socts)
    seq_small = sequence(small, a.small // 2, a.reps)
    small.close()
    r3 = lambda d, h: d[0] / h[0]
    lines = [
        "# Covisibility: the device entries against the host build of the same core on one thread",
        "",
        "`python tools/prof_covis.py --reps %d --keyframes %d --features %d --frames %d --small %d` on one MI355X.  The map: %d key frames x %d features," % (
            a.reps, a.keyframes, a.features, a.frames, a.small, a.keyframes, a.features),
        "%d observations, a map point tracked by 3..12 consecutive key frames.  Host to host around the library calls, arguments laid out beforehand;" % n_obs,
        "medians, p10 / p90 in brackets.  Every device result timed here was compared with the host core's in the same run.",
        "",
        "## (a) one build, then the votes of %d frames in one call (%d ids in all)" % (a.frames, len(ids)),
        "",
        "| what | device ms | host core, one thread, ms | device / host |",
        "|---|---|---|---|",
        "| `cms_covis_build` of the whole map | %.3f (%.3f / %.3f) | %.3f (%.3f / %.3f) | %.3f |" % (t_bd + t_bh + (r3(t_bd, t_bh),)),
        "| `cms_covis_votes`, %d frames in one call | %.3f (%.3f / %.3f) | %.3f (%.3f / %.3f) | %.3f |" % ((a.frames,) + t_vd + t_vh + (r3(t_vd, t_vh),)),
        "| ... per frame | %.4f | %.4f | |" % (t_vd[0] / a.frames, t_vh[0] / a.frames),
        "| `cms_covis_votes`, 1 frame | %.3f (%.3f / %.3f) | %.3f (%.3f / %.3f) | %.3f |" % (t_v1d + t_v1h + (r3(t_v1d, t_v1h),)),
        "",
        "## (b) a key frame's sequence: build, 2 x connections, one culling chain",
        "",
        "| map | chain | device ms | host core, one thread, ms | device / host | of which the build: device, host |",
        "|---|---|---|---|---|---|",
    ]
    for name, kfs, s in (("large", a.keyframes, seq_big), ("small", a.small, seq_small)):
        d, h, parts, n, nconn, nred = s
        lines.append("| %s, %d key frames | %d of %d connected, %d redundant | %.3f (%.3f / %.3f) | %.3f (%.3f / %.3f) | %.3f | %.3f, %.3f |" % (
            (name, kfs, n, nconn, nred) + d + h + (r3(d, h), parts["build"][0], parts["build_host"][0])))
    qb, qs = seq_big[1][0] - seq_big[2]["build_host"][0], seq_small[1][0] - seq_small[2]["build_host"][0]
    lines += [
        "",
        "## Reading",
        "",
        "The host core's build is a sort of all observations.  The reference pays nothing like it: it keeps its observation maps up to date with every",
        "AddObservation / EraseObservation.  So the build is the price of the snapshot design on either side, and the honest host figure for (b) is the",
        "host core's queries alone: %.3f ms (large map) and %.3f ms (small map), against the device's whole sequence, its build included, of %.3f ms and" % (
            qb, qs, seq_big[0][0]),
        "%.3f ms (ratios %.2f and %.2f).  The reference's own pointer walk was not timed here." % (seq_small[0][0], seq_big[0][0] / qb, seq_small[0][0] / qs),
        "",
        "Workload (a) is the case for the feature: the votes of %d frames cost one launch and %.3f ms, %.0f times less than one host thread needs, and the" % (
            a.frames, t_vd[0], t_vh[0] / t_vd[0]),
        "host that serves many streams per GPU no longer does them at all.  One frame alone is %s on the device (%.3f ms against %.3f ms)." % (
            "faster" if t_v1d[0] < t_v1h[0] else "SLOWER", t_v1d[0], t_v1h[0]),
        "Workload (b) %s it: a single small map's sequence is %s on the device than the host core's queries on one thread (%.3f ms against %.3f ms);" % (
            "supports" if seq_small[0][0] < qs else "does NOT support", "faster" if seq_small[0][0] < qs else "SLOWER", seq_small[0][0], qs),
        "its gain is host time on the mapping thread, a few milliseconds per key frame, not latency.",
        "",
    ]
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    mctx.close(); fctx.close()


if __name__ == "__main__":
    main()
