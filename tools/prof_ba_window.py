"""Time of cms_covis_local_ba_windows on the device against the host build of the same core (csrc/cms_ba_window_core.h through hm_ba_window_run) on ONE
thread, for 1 job and for 16 jobs of a workload-sized window: --local local key frames of --features features plus the fixed key frames that observe
their points, about 80 k edges, the size of bench.py's BA leg.  The map is tests/ba_window_cases.py's windowed generator.

Both sides are timed host to host around the library call with the arguments laid out beforehand; the device figures include the upload of the jobs,
the four launches, the copy back and the wait, once with plain host outputs (everything comes back through the staging block) and once with pinned
outputs (the kernels store into them).  The host figure is the assembly alone: the index is built beforehand on both sides.  Every timed device result
is first compared with the host core's.  Medians over --reps calls after a warm-up, p10 / p90 in brackets.  Writes profiles/ba_window.md (or --out).

    python tools/prof_ba_window.py [--reps 20] [--members 120] [--features 2000] [--local 20] [--out profiles/ba_window.md]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cubemapslam_amd import api  # noqa: E402
import ba_window_cases as bc  # noqa: E402
import ba_window_hostlib as bh  # noqa: E402


def median_of(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--members", type=int, default=120)
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--local", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ba_window.md"))
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    ms = bc.windowed_map(rng, a.members, a.features, int(0.95 * a.features), 120, 3000, 1 << 17)
    jobs16 = [([10 + 5 * j + (7 * k) % a.local for k in range(a.local)], 11 + 5 * j) for j in range(16)]
    c = bc.make("workload", ms, jobs16, 1 << 17, (a.members, a.local * a.features, 16 * a.local * a.features))
    ctx = api.Context(bc.CAMD, nfeatures=500, max_batch=1)
    dm = bh.DeviceMap(ctx, c)
    hw = bh.HostWindows(c)
    rc, want, _ = hw.run(jobs16, c["caps"])
    assert rc == 0
    caps = (max(int(w["counts"][0]) for w in want), max(int(w["counts"][2]) for w in want), max(int(w["counts"][3]) for w in want))
    lines = []
    for nj in (1, 16):
        jobs = jobs16[:nj]
        outs = {kind: api.ba_window_arrays(nj, *caps, pinned=(kind == "pinned")) for kind in ("plain", "pinned", "host")}
        for kind in ("plain", "pinned"):
            got = dm.cv.local_ba_windows(dm.mp, jobs, *caps, out=outs[kind])
            assert bc.difference(want[:nj], got) is None, (kind, bc.difference(want[:nj], got))
        t_plain = median_of(lambda: dm.cv.local_ba_windows(dm.mp, jobs, *caps, out=outs["plain"]), a.reps)
        t_pinned = median_of(lambda: dm.cv.local_ba_windows(dm.mp, jobs, *caps, out=outs["pinned"]), a.reps)
        t_host = median_of(lambda: hw.run(jobs, caps, out=outs["host"]), a.reps)
        K = [int(w["counts"][0]) for w in want[:nj]]; P = [int(w["counts"][2]) for w in want[:nj]]; E = [int(w["counts"][3]) for w in want[:nj]]
        lines.append("| %d | %d..%d | %d..%d | %d..%d | %.3f (%.3f / %.3f) | %.3f (%.3f / %.3f) | %.3f (%.3f / %.3f) |"
                     % ((nj, min(K), max(K), min(P), max(P), min(E), max(E)) + t_plain + t_pinned + t_host))
        print(lines[-1], flush=True)
    text = """# Local BA window from the resident stores: device against one host thread

`python tools/prof_ba_window.py --reps %d --members %d --features %d --local %d` on one MI355X and one CPU thread of the same machine.  Times in ms, median
(p10 / p90), host to host around the library call, Python's argument packing included on both sides.  A call is 1 upload, 4 kernel launches
(`k_covis_local_points`, `k_baw_count`, `k_baw_frames`, `k_baw_fill`), 1 copy back and 1 wait, whatever the number of jobs.

| jobs | K | P | E | device, plain host outputs | device, pinned outputs | host core, one thread |
|---|---|---|---|---|---|---|
%s

The host figure is the assembly alone, with its index already built from host copies of every row, key point, ray, pose and position -- the copies the
resident stores exist to make unnecessary; keeping them current is not in it.
""" % (a.reps, a.members, a.features, a.local, "\n".join(lines))
    with open(a.out, "w") as f:
        f.write(text)
    print("wrote", a.out)
    hw.close(); dm.close(); ctx.close()


if __name__ == "__main__":
    main()
