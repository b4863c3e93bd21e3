"""Time of ComputeBoW on the device against the path it replaces, at ORBvoc.txt's shape (k = 10, L = 6 complete: 1 111 111 nodes, synthetic descriptors
and weights -- the vocabulary is data) for one batch of 256 frame rows of ~1650 features each:

  device   cms_frames_compute_bow over the 256 rows in ONE call: host-to-host time of the call (row table up, two launches, counts back,
           synchronisation) and, from events around the launches (cms_vocab_profile_*), k_vocab_descend and k_vocab_build on their own
  host     what a host without the device path does for ONE frame: fetch the row's key points and descriptors (cms_frames_fetch), run the host
           build of the same core on one thread (ORBVocabulary::transform, engine HOST_CORE).  The upload of the CSR is not timed: it rides in the
           consumer's staged copy (cms_kfstore_put_from_frames, cms_kfstore_search_by_bow), so the host figure is a lower bound of the replaced path.

Writes the figures and their ratio to profiles/bow_transform.md (or --out).  Medians over --reps calls after a warm-up.

    python tools/prof_bow_transform.py [--reps 30] [--rows 256] [--features 1650] [--out profiles/bow_transform.md]"""
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
import vocab_cases  # noqa: E402
import vocab_hostlib  # noqa: E402

KP = api.KP_DTYPE


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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--features", type=int, default=1650)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bow_transform.md"))
    a = ap.parse_args()
    tree = vocab_cases.case_tree("full_size")
    voc = api.Vocabulary.from_dict(tree)
    host = vocab_hostlib.HostVocabulary(tree)
    ctx = api.Context(synth.camera("lafida", 150), nfeatures=2000, max_batch=a.rows)
    assert ctx.geom.kp_cap >= a.features
    rng = np.random.default_rng(3)
    ns = np.clip(rng.normal(a.features, 40, a.rows).astype(np.int32), 1, ctx.geom.kp_cap)
    kps = np.zeros(int(ns.max()), KP)
    descs = []
    for b in range(a.rows):
        d = rng.integers(0, 256, (int(ns[b]), 32), dtype=np.uint8)      # (the tree's descriptors are independent random bytes too: every level is a real choice)
        descs.append(d)
        ctx.area_set_keypoints(b, kps[:ns[b]]); ctx.area_set_descriptors(b, d)
    rows = np.arange(a.rows, dtype=np.int32)
    L = api.lib()
    L.cms_vocab_profile_enable.argtypes = [C.c_int]
    L.cms_vocab_profile_get.argtypes = [C.c_void_p]
    # correctness first: row 0 of the batch equals the host core
    ctx.compute_bow(voc, rows, ns, 4)
    g, w = ctx.fetch_bow(0), host.transform(descs[0], 4)
    assert all(np.array_equal(g[k], w[k]) for k in ("word_id", "node_id", "node_off", "node_feat")) and np.array_equal(g["word_val"].view(np.uint64), w["word_val"].view(np.uint64))
    call = median_of(lambda: ctx.compute_bow(voc, rows, ns, 4), a.reps)
    L.cms_vocab_profile_enable(1)
    ker = []
    for _ in range(a.reps):
        ctx.compute_bow(voc, rows, ns, 4)
        ms = np.zeros(2, np.float32)
        assert L.cms_vocab_profile_get(api._p(ms)) == 0
        ker.append(ms.copy())
    L.cms_vocab_profile_enable(0)
    ker = np.median(np.array(ker), axis=0)
    one = median_of(lambda: ctx.compute_bow(voc, rows[:1], ns[:1], 4), a.reps)
    fetch = median_of(lambda: ctx.fetch(0), a.reps)
    hreps = max(3, a.reps // 3)
    htr = median_of(lambda: host.transform(descs[0], 4), hreps, warm=1)
    host_frame = fetch[0] + htr[0]
    ratio = call[0] / host_frame
    verdict = "confirmed" if ratio < 1.0 else "refuted"
    lines = [
        "# ComputeBoW: device batch against the host path it replaces",
        "",
        "`python tools/prof_bow_transform.py --reps %d --rows %d --features %d` on one MI355X; synthetic vocabulary of ORBvoc.txt's shape" % (a.reps, a.rows, a.features),
        "(k = 10, L = 6 complete, %d nodes, %d words), levelsup 4, %d rows of %d..%d features (%d in all).  Medians; p10 / p90 in brackets." % (
            len(tree["parent"]), int(tree["is_leaf"].sum()), a.rows, int(ns.min()), int(ns.max()), int(ns.sum())),
        "",
        "| what | ms |",
        "|---|---|",
        "| device: `cms_frames_compute_bow`, %d rows in one call, host to host | %.3f (%.3f / %.3f) |" % (a.rows, call[0], call[1], call[2]),
        "| ... of which `k_vocab_descend` (events) | %.3f |" % ker[0],
        "| ... of which `k_vocab_build` (events) | %.3f |" % ker[1],
        "| device: `cms_frames_compute_bow`, ONE row per call, host to host | %.3f (%.3f / %.3f) |" % one,
        "| host, one frame: `cms_frames_fetch` (key points + descriptors) | %.3f (%.3f / %.3f) |" % fetch,
        "| host, one frame: transform by the host build of the core, one thread (%d reps) | %.3f (%.3f / %.3f) |" % ((hreps,) + htr),
        "| host, one frame: fetch + transform (the CSR's upload not included) | %.3f |" % host_frame,
        "",
        "Device batch of %d rows / host path of ONE frame = **%.3f**.  The expectation \"the device batch costs less than one host transform of one frame\"" % (a.rows, ratio),
        "is **%s** by this run.  Per row the device costs %.4f ms, %.0f times less than the host's %.3f ms." % (verdict, call[0] / a.rows, host_frame / (call[0] / a.rows), host_frame),
        "",
    ]
    text = "\n".join(lines)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    voc.close(); host.close(); ctx.close()


if __name__ == "__main__":
    main()
