"""Time of the map-point table's refresh against the path it replaces, and of the local-map search by ids against its host-array sibling.

  (a) cms_mpstore_refresh (both halves) for the points of a local-BA window (the rows of --window consecutive key frames) and for all points of
      the map, on maps of --small and --keyframes key frames x --features features with prof_covis's tracked observation pattern;
  (b) the path of the parent commit for the same points: cms_distinctive_descriptors + cms_update_normal_and_depth on PRE-ASSEMBLED host arrays,
      and separately the host time to assemble them.  The assembly here is numpy's vectorised gather over flat observation arrays (one fancy
      index per array): a lower bound of what a caller pays who walks a std::map per point and copies 32 bytes and a camera centre per observation;
  (c) cms_search_local_points_ids against cms_search_local_points at --local local points (a frame of 2 000 key points, Lafida F = 550).

Every figure is timed host to host around the synchronous library call(s) with the arguments laid out beforehand: the median of --reps calls after a
warm-up, p10 / p90 in brackets.  Before timing, the table's rows are compared with the parent path's results.  Writes profiles/mappoints.md (or --out).

    python tools/prof_mappoints.py [--reps 20] [--keyframes 1000] [--small 60] [--features 2000] [--window 10] [--local 1500] [--out profiles/mappoints.md]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cubemapslam_amd import api, synth  # noqa: E402
import mappoint_cases as mc  # noqa: E402
import mappoint_hostlib as hl  # noqa: E402
from prof_covis import median_of  # noqa: E402


def tracked_map(rng, K, F, fill=0.97, lo=3, hi=12):
    """prof_covis's tracked rows with dense ids: rows[k] = the ids whose stretch of consecutive key frames covers k -> (rows, octs, number of ids)"""
    P = int(K * F * fill / ((lo + hi) / 2.0)) + 1
    start = rng.integers(-hi, K, P); length = rng.integers(lo, hi + 1, P)
    kf = np.concatenate([np.arange(s, s + n) for s, n in zip(start, length)])
    pt = np.repeat(np.arange(P), length)
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
    return rows, octs, P


def fmt(t):
    return "%.3f ms [%.3f .. %.3f]" % t


def map_figures(cg, K, F, window, reps, out):
    rng = np.random.default_rng(K)
    rows, octs, P = tracked_map(rng, K, F)
    descs = [rng.integers(0, 256, (F, 32), dtype=np.uint8) for _ in range(K)]
    Ows = rng.normal(0, 3, (K, 3)).astype(np.float32)
    st = api.KeyframeStore(cg, max_keyframes=K, max_features=F, max_nodes=8)
    for s in range(K):
        kf, keep = hl.keyframe(rows[s], octs[s], descs[s], Ows[s])
        st.put(s, kf)
    cv = api.Covisibility(st, K); cv.build(np.arange(K))
    mp = api.MapPointStore(st, P)
    # flat observation arrays in (id, member) order: what the parent path's caller assembles its staging arrays from
    member = np.repeat(np.arange(K), F); feat = np.tile(np.arange(F), K); ids_flat = np.concatenate(rows)
    keep_ = ids_flat >= 0
    member, feat, ids_flat = member[keep_], feat[keep_], ids_flat[keep_]
    order = np.lexsort((member, ids_flat))
    member, feat, ids_flat = member[order], feat[order], ids_flat[order]
    seen = np.unique(ids_flat)
    first = np.searchsorted(ids_flat, seen)
    pos = rng.normal(0, 5, (P, 3)).astype(np.float32)
    mp.set(seen, pos[seen], member[first].astype(np.int32))      # the reference: the first observer's slot (slot = member here)
    all_desc = np.stack(descs); all_oct = np.stack(octs)
    k0 = K // 2
    win = np.unique(np.concatenate([r[r >= 0] for r in rows[k0:k0 + window]]))
    L = api.lib()
    for label, ids in (("local-BA window (%d key frames)" % window, win), ("whole map", seen)):
        ids = np.ascontiguousarray(ids, np.int32)
        status = np.zeros(len(ids), np.uint8)

        def refresh():
            assert L.cms_mpstore_refresh(mp.h, cv.h, len(ids), api._p(ids), 3, api._p(status)) == 0
        refresh()
        assert (status == 0).all()

        def assemble():
            lo = np.searchsorted(ids_flat, ids); hi = np.searchsorted(ids_flat, ids, side="right")
            obs_off = np.zeros(len(ids) + 1, np.int32); obs_off[1:] = np.cumsum(hi - lo)
            sel = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)])
            m, f = member[sel], feat[sel]
            return (obs_off, np.ascontiguousarray(all_desc[m, f]), np.ascontiguousarray(Ows[m]), np.ascontiguousarray(pos[ids]), np.ascontiguousarray(Ows[member[lo]]),
                    np.ascontiguousarray(all_oct[member[lo], feat[lo]]))
        obs_off, odesc, oOw, p_, refOw, reflev = assemble()
        best = np.zeros(len(ids), np.int32); nrm = np.zeros((len(ids), 3), np.float32); mn = np.zeros(len(ids), np.float32); mx = np.zeros(len(ids), np.float32)

        def parent():
            assert L.cms_distinctive_descriptors(cg.h, len(ids), api._p(obs_off), api._p(odesc), api._p(best)) == 0
            assert L.cms_update_normal_and_depth(cg.h, len(ids), api._p(obs_off), api._p(p_), api._p(oOw), api._p(refOw), api._p(reflev), api._p(nrm), api._p(mn), api._p(mx)) == 0
        parent()
        got = mp.fetch(ids)
        assert np.array_equal(got["desc"], odesc[obs_off[:-1] + best]) and np.array_equal(got["normal"].view(np.uint32), nrm.view(np.uint32))
        assert np.array_equal(got["min_dist"].view(np.uint32), mn.view(np.uint32)) and np.array_equal(got["max_dist"].view(np.uint32), mx.view(np.uint32))
        out.append("| %d x %d | %s | %d | %d | %s | %s | %s |" % (K, F, label, len(ids), int(obs_off[-1]), fmt(median_of(refresh, reps)), fmt(median_of(parent, reps)),
                                                                   fmt(median_of(assemble, reps))))
    mp.close(); cv.close(); st.close()


def search_figures(cg, n_local, reps, out):
    c = mc.search_case(F=550, nkp=2000, maxf=4096, key="search550")
    fctx = api.Context(synth.camera("lafida", 550), nfeatures=2000, max_batch=1)
    st = api.KeyframeStore(cg, max_keyframes=c["K"], max_features=c["maxf"], max_nodes=8)
    b = hl.DeviceBackend(st, 4, max_points=4096)
    b.load(c); b.set(c["ids"], c["pos"], c["ref"])
    assert (b.refresh(c["ids"]) == 0).all()
    ids = np.ascontiguousarray(c["ids"][:n_local], np.int32)
    rows = b.fetch(ids)
    kps = np.zeros(len(c["kx"]), api.KP_DTYPE); kps["x"] = c["kx"]; kps["y"] = c["ky"]; kps["octave"] = c["ko"]
    fctx.area_set_keypoints(0, kps); fctx.area_set_descriptors(0, c["kd"]); fctx.area_grid(1)
    taken = np.full(len(c["kx"]), -1, np.int32)
    res = {}

    def by_ids():
        res["ids"] = fctx.search_local_points_ids(0, c["pose15"], b.mp, ids, taken.copy(), th=5.0)

    def by_arrays():
        res["arr"] = fctx.search_local_points(0, c["pose15"], rows["pos"], rows["normal"], rows["min_dist"], rows["max_dist"], rows["desc"], taken.copy(), th=5.0)
    by_ids(); by_arrays()
    assert np.array_equal(res["ids"]["match"], res["arr"]["match"]) and res["ids"]["n_matches"] > 100
    out.append("| %d local points, %d key points | %d | %s | %s |" % (len(ids), len(kps), res["ids"]["n_matches"], fmt(median_of(by_ids, reps)), fmt(median_of(by_arrays, reps))))
    b.close(); st.close(); fctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20); ap.add_argument("--keyframes", type=int, default=1000); ap.add_argument("--small", type=int, default=60)
    ap.add_argument("--features", type=int, default=2000); ap.add_argument("--window", type=int, default=10); ap.add_argument("--local", type=int, default=1500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mappoints.md"))
    a = ap.parse_args()
    cg = api.Context(synth.camera("lafida", 550), nfeatures=2000, max_batch=1)
    maps, search = [], []
    for K in (a.small, a.keyframes):
        map_figures(cg, K, a.features, a.window, a.reps, maps)
    search_figures(cg, a.local, a.reps, search)
    text = ["# Map points on the device: refresh and the search by ids", "",
            "Written by `tools/prof_mappoints.py --reps %d`: medians of %d synchronous calls after a warm-up, host to host, p10 .. p90 in brackets." % (a.reps, a.reps), "",
            "## Refresh of the table against the parent's path", "",
            "`refresh`: `cms_mpstore_refresh`, both halves.  `parent`: `cms_distinctive_descriptors` + `cms_update_normal_and_depth` on pre-assembled host arrays.",
            "`assemble`: the host time to build those arrays (numpy's vectorised gather: a lower bound of a per-point walk over a `std::map`).", "",
            "| map | points of | ids | observations | refresh | parent | assemble |", "|---|---|---|---|---|---|---|"] + maps + [
            "", "## Local-map search: ids against host arrays", "", "| input | matches | `cms_search_local_points_ids` | `cms_search_local_points` |", "|---|---|---|---|"] + search + [""]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text))
    print("\n".join(text))
    cg.close()


if __name__ == "__main__":
    main()
