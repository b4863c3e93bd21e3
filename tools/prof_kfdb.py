"""Time of KeyFrameDatabase::DetectRelocalizationCandidates on the device against the path it replaces, at a relocalisation's shape: 1024 database
entries of ~1650 words each (64 places of 16 key frames: a query shares some 900 words with the key frames of its place and a handful with the rest), one
query and 256 queries per call.

  device   cms_kfdb_detect with the queries resident (store slots outside the database, as a frame row's BowVector is resident): host-to-host time
           of the call (snapshot, one upload, four launches, one copy back, one wait) and, from events around the launches (cms_kfdb_profile_*), the
           launch sequence on its own
  host     what a host-side database does for ONE query: fetch the query's BowVector (cms_kfstore_fetch_bow: the copies cms_frames_fetch_bow makes)
           and run the host build of the same core on one thread (CmsKfdbHost::detect).  That core intersects the query with every entry of its group
           instead of walking an inverted file, so the host figure is an upper bound of what a tuned host database needs.

Writes the figures to profiles/kfdb.md (or --out).  Medians over --reps calls after a warm-up, p10 / p90 as the spread.  --bench PARENT TREE adds the
flagship benchmark's medians (two JSON files with the ms/step of repeated bench.py runs at the parent commit and at this tree).

    python tools/prof_kfdb.py [--reps 30] [--entries 1024] [--queries 256] [--words 1650] [--out profiles/kfdb.md]"""
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
import kfdb_cases as kc  # noqa: E402
import kfdb_hostlib  # noqa: E402


def median_of(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90))


def place_bow(rng, place, n, pool=3000):
    ids = np.sort(place * 10000 + rng.choice(pool, size=n, replace=False)).astype(np.int32)
    v = rng.random(n) + 0.05
    return ids, v / v.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--entries", type=int, default=1024)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--words", type=int, default=1650)
    ap.add_argument("--bench", nargs=2, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kfdb.md"))
    a = ap.parse_args()
    E, Q, K = a.entries, a.queries, a.entries + a.queries
    maxf = 2048
    places = max(E // 16, 1)
    rng = np.random.default_rng(11)
    fctx = api.Context(synth.camera("lafida", 150), nfeatures=500, max_batch=1)
    mctx = api.Context(synth.camera("lafida", 150), nfeatures=500, max_batch=1)
    st = api.KeyframeStore(mctx, max_keyframes=K, max_features=maxf, max_nodes=8)
    dev = kfdb_hostlib.DeviceBackend(st, fctx)
    host = kfdb_hostlib.HostDatabase(K, maxf)
    nw = np.clip(rng.normal(a.words, 40, K).astype(np.int32), 1, maxf)
    bows = []
    for s in range(K):
        dev.refill(s)
        bows.append(place_bow(rng, s % places, int(nw[s])))
        dev.set_bow(s, *bows[s]); host.set_bow(s, *bows[s])
    entries = np.arange(E, dtype=np.int32)
    for b in (dev, host):
        b.add(entries, np.zeros(E, np.int32))
    neigh = np.array([kc.pad10((s + d * places) % E for d in range(1, 11)) for s in range(E)], np.int32)      # the key frames of the same place
    st.db_set_covisibles(entries, neigh)
    for s in range(E):
        host.covis(s, neigh[s])
    jobs = [kc.job(kc.RELOC, ("slot", E + j)) for j in range(Q)]
    hjobs = [kc.job(kc.RELOC, kc.words(*bows[E + j])) for j in range(Q)]
    # correctness first: the first 8 queries equal the host core, bit for bit
    got, want = st.detect_candidates(fctx, jobs[:8]), host.detect(hjobs[:8])
    assert kc.first_difference([want], [got]) is None, kc.first_difference([want], [got])
    n_cand = [len(j[0]) for j in got]
    common_max = int(max(j[1].max() for j in got))
    L = api.lib()
    L.cms_kfdb_profile_enable.argtypes = [C.c_int]
    L.cms_kfdb_profile_get.argtypes = [C.c_void_p]

    def device(n):
        call = median_of(lambda: st.detect_candidates(fctx, jobs[:n], cand_cap=64, diag=False), a.reps)
        lib_ms = []
        L.cms_kfdb_profile_enable(1)
        ev = []
        for _ in range(a.reps):
            st.detect_candidates(fctx, jobs[:n], cand_cap=64, diag=False)
            lib_ms.append(st.last_call_ms)
            ms = C.c_float()
            assert L.cms_kfdb_profile_get(C.byref(ms)) == 0
            ev.append(ms.value)
        L.cms_kfdb_profile_enable(0)
        return call, float(np.median(lib_ms)), float(np.median(ev))
    d1, d1_lib, d1_ev = device(1)
    dq, dq_lib, dq_ev = device(Q)
    fetch = median_of(lambda: st.fetch_bow(E), a.reps)
    hreps = max(3, a.reps // 3)
    hdet = median_of(lambda: host.detect(hjobs[:1], cand_cap=64), hreps, warm=1)
    host_one = fetch[0] + hdet[0]
    lines = [
        "# KeyFrameDatabase: candidate detection on the device against the host path it replaces",
        "",
        "`python tools/prof_kfdb.py --reps %d --entries %d --queries %d --words %d` on one MI355X; %d database entries of %d..%d words in %d places," % (
            a.reps, E, Q, a.words, E, int(nw[:E].min()), int(nw[:E].max()), places),
        "relocalisation queries resident in store slots (up to %d common words with an entry, %s candidates for the first queries)." % (common_max, n_cand),
        "Medians; p10 / p90 in brackets.  The first 8 queries were checked bit for bit against the host core in the same run.",
        "",
        "| what | ms |",
        "|---|---|",
        "| device: `cms_kfdb_detect`, 1 query, Python wrapper included | %.3f (%.3f / %.3f) |" % d1,
        "| ... the library call alone, host to host, with the events recorded | %.3f |" % d1_lib,
        "| ... of which the four launches (events) | %.3f |" % d1_ev,
        "| device: `cms_kfdb_detect`, %d queries in one call, Python wrapper included | %.3f (%.3f / %.3f) |" % ((Q,) + dq),
        "| ... the library call alone, host to host, with the events recorded | %.3f |" % dq_lib,
        "| ... of which the four launches (events) | %.3f |" % dq_ev,
        "| host, one query: fetch of the BowVector (`cms_kfstore_fetch_bow`) | %.3f (%.3f / %.3f) |" % fetch,
        "| host, one query: the host build of the core, one thread (%d reps) | %.3f (%.3f / %.3f) |" % ((hreps,) + hdet),
        "| host, one query: fetch + detect | %.3f |" % host_one,
        "",
        "One query: device call / host path = **%.3f**.  %d queries: %.4f ms per query on the device, %.0f times less than the host's %.3f ms." % (
            d1_lib / host_one, Q, dq_lib / Q, host_one / (dq_lib / Q), host_one),
        "The host core intersects the query with every entry (no inverted file): its figure is an upper bound of a tuned host database's.",
        "",
    ]
    if a.bench:
        runs = [json.load(open(f)) for f in a.bench]
        med = [float(np.median(r)) for r in runs]
        lines += ["## bench.py (the flagship workload does not use the database)", "",
                  "Alternating runs of `bench.py --gpus 1` in one session, ms per step: parent commit %s (median **%.3f**, spread %.3f), this tree %s (median **%.3f**, spread %.3f)." % (
                      ["%.3f" % x for x in runs[0]], med[0], max(runs[0]) - min(runs[0]), ["%.3f" % x for x in runs[1]], med[1], max(runs[1]) - min(runs[1])), ""]
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    host.close(); st.close(); mctx.close(); fctx.close()


if __name__ == "__main__":
    main()
