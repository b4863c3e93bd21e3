"""Pose optimisation (cms_pose_*, k_pose_optimize / k_pose_optimize_g): parity matrix over sizes, start poses, cameras, outlier shares and
degenerate inputs (tests/pose_cases.py; the two CPU references agree on every family, tests/test_pose_cases_cpu.py), through every way into
the two kernels.

 (a) every case against the oracle, frames of up to 1024 edges through the register kernel, larger ones through the in-memory kernel
 (b) the same batches with one 1025-edge frame appended -- the whole batch then runs the in-memory kernel -- against the oracle and against (a)
 (c) one kernel, one input: the same bits whatever the entry point, the position in the batch and the company
 (d) one handle through calls of growing and shrinking size: every pinned block regrown, every result that of a fresh handle
 (e) (a) and (c) again under the two developer switches, each in a child process
 (f) misuse reported as CMS_ERR_ARG with a message by both entry points, the handle usable afterwards

The bar is the project's: flags, inlier count, rounds identical; iteration counts identical; pose update within 1e-4 of the update
(_pose_close of test_gpu_parity.py).  The one excuse of test_pose_optimization_matches_oracle -- a converged round may run one iteration more
or fewer, accepted only if the poses then agree to 1e-10 of the update -- may be used by at most one problem in fifty per family."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import orc
import pose_cases as pc
from cubemapslam_amd import api, synth
from test_gpu_parity import _pose_close

pytestmark = pytest.mark.gpu

REG_MAX = 1024          # most edges of a frame the register kernel takes (256 threads x PO_MAXJ)
MAX_BATCH = 300
# Measured on an MI355X over every family: the two kernels return the same bits (profiles/pose_parity_matrix.md).
TWINS_BIT_EQUAL = True


def _stats(st):
    return (int(st.rounds), int(st.n_bad)) + tuple(int(i) for i in st.iterations_done)


def _pack(res):
    """(n_inliers, poses, flags per frame, stats) of a batch call -> one (n, pose, flags, stats tuple) per frame"""
    ninl, poses, outs, stats = res
    return [(int(ninl[f]), np.array(poses[f], np.float64), np.array(outs[f], np.uint8), _stats(stats[f])) for f in range(len(outs))]


def _pack1(res):
    n, pose, out, st = res
    return (int(n), np.array(pose, np.float64), np.array(out, np.uint8), _stats(st))


def _bits_equal(a, b):
    return (a[0] == b[0] and a[3] == b[3] and a[2].shape == b[2].shape and np.array_equal(a[2], b[2])
            and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)))


def _resident(probs):
    """upload / launch / fetch on a handle made for exactly this batch (max_frames = nf, max_edges = the batch's edges)"""
    po = api.PoseOptimizer(len(probs), max(sum(len(p["Xw"]) for p in probs), 1))
    try:
        return _pack(po.optimize(probs))
    finally:
        po.close()


def _companion(pr):
    """a 1025-edge frame with the intrinsics of pr: its presence sends the batch through k_pose_optimize_g"""
    c = synth.pose_problem(N=REG_MAX + 1, seed=77, outlier_frac=0.1)
    for k in ("fx", "fy", "cx", "cy"):
        c[k] = pr[k]
    return c


def _run_cases(probs, companion):
    """every problem through the resident path, batched by intrinsics (one set per launch) and by kernel; None for a frame above 1024 edges
    when companion is set (it runs the in-memory kernel without one: nothing new)"""
    out = [None] * len(probs)
    groups = {}
    for i, p in enumerate(probs):
        groups.setdefault((p["fx"], p["fy"], p["cx"], p["cy"], len(p["Xw"]) > REG_MAX), []).append(i)
    for key, idx in groups.items():
        if companion and key[4]:
            continue
        step = MAX_BATCH - 1
        for c0 in range(0, len(idx), step):
            chunk = idx[c0:c0 + step]
            batch = [probs[i] for i in chunk] + ([_companion(probs[chunk[0]])] if companion else [])
            res = _resident(batch)
            for j, i in enumerate(chunk):
                out[i] = res[j]
    return out


def _check(tag, pr, got, want):
    """one problem against the oracle; returns (excuse used, relative pose distance)"""
    n, pose, flags, st = got
    w_n, w_pose, w_out, w_st = want
    w_stats = _stats(w_st)
    N = len(pr["Xw"])
    assert n == w_n and np.array_equal(flags, w_out), (tag, n, w_n, int((flags != w_out).sum()))
    assert st[:2] == w_stats[:2], (tag, st, w_stats)
    same_iters = st[2:] == w_stats[2:]
    if N < 3:                                # Optimizer.cpp:131-132: nothing happens
        assert same_iters and n == 0 and st[0] == 0 and np.array_equal(pose.view(np.uint64), pr["pose0"].view(np.uint64)), (tag, st, pose)
        return False, 0.0
    ref0 = pc.normalized_start(pr)
    du = np.linalg.norm(w_pose - ref0)
    if du <= 1e-12:
        # the oracle made no step at all: the result is the start pose through the SE3Quat constructor.  _pose_close's floor would make this
        # 1e-16 absolute; what the arithmetic allows is: translation untouched, one square root and one division (or a reciprocal and a
        # product) per quaternion component, each within 1 ulp
        assert np.array_equal(w_pose[:3], pr["pose0"][:3]), tag
        assert same_iters, (tag, st, w_stats)
        assert np.array_equal(pose[:3].view(np.uint64), pr["pose0"][:3].view(np.uint64)), (tag, pose[:3], pr["pose0"][:3])
        ulps = np.abs(pose[3:] - w_pose[3:]) / np.spacing(np.abs(w_pose[3:]))
        assert ulps.max() <= 4, (tag, ulps)
        return False, 0.0
    ok, (err, du) = _pose_close(pose, w_pose, ref0, tol=1e-4 if same_iters else 1e-10)
    assert ok, (tag, err, du, st, w_stats)
    return not same_iters, err / du


def _check_twins(tag, pr, a, b):
    """register kernel against in-memory kernel on one problem; returns (excuse used, bit-equal)"""
    assert a[0] == b[0] and np.array_equal(a[2], b[2]) and a[3][:2] == b[3][:2], (tag, a[0], b[0], a[3], b[3])
    bits = _bits_equal(a, b)
    if TWINS_BIT_EQUAL:
        assert bits, (tag, a[1], b[1], a[3], b[3])
        return False, True
    same_iters = a[3] == b[3]
    if len(pr["Xw"]) >= 3:
        ok, info = _pose_close(a[1], b[1], pc.normalized_start(pr), tol=1e-10)
        assert ok, (tag, info, a[3], b[3])
    else:
        assert bits, tag
    return not same_iters, bits


@pytest.mark.parametrize("fam", pc.FAMILIES)
def test_matrix_against_the_oracle_through_both_kernels(fam):
    cases = pc.family(fam)
    probs = [p for _, p in cases]
    want = [orc.pose_optimize(p) for p in probs]
    cap = math.ceil(len(cases) / 50)
    got_a = _run_cases(probs, companion=False)
    got_b = _run_cases(probs, companion=True)
    exc_a = exc_b = exc_t = 0
    worst_a = worst_b = 0.0
    n_b = n_bits = 0
    for (name, pr), w, a, b in zip(cases, want, got_a, got_b):
        tag = "%s: %s" % (fam, name)
        e, rel = _check(tag + " (a)", pr, a, w)
        exc_a += e; worst_a = max(worst_a, rel)
        if b is None:
            continue
        e, rel = _check(tag + " (b)", pr, b, w)
        exc_b += e; worst_b = max(worst_b, rel)
        e, bits = _check_twins(tag + " (a) vs (b)", pr, a, b)
        exc_t += e; n_b += 1; n_bits += bits
    print("pose matrix | %s | problems %d | excuses (a) %d (b) %d twins %d of %d allowed | worst relative pose distance (a) %.2e (b) %.2e | "
          "twins bit-equal %d of %d" % (fam, len(cases), exc_a, exc_b, exc_t, cap, worst_a, worst_b, n_bits, n_b))
    assert exc_a <= cap and exc_b <= cap and exc_t <= cap, (fam, exc_a, exc_b, exc_t, cap)


def _fixed_set():
    return [synth.pose_problem(N=n, seed=200 + i, outlier_frac=o) for i, (n, o) in enumerate(
        ((600, 0.1), (0, 0.0), (3, 0.0), (1024, 0.2), (2, 0.0), (9, 0.0), (257, 0.05), (10, 0.0), (64, 0.3), (1000, 0.1), (40, 0.0), (300, 0.5)))]


def _fillers(n):
    sizes = (50, 120, 333, 7, 600, 0, 200, 1024, 90, 256, 1, 480)
    return [synth.pose_problem(N=sizes[i % len(sizes)], seed=700 + i, outlier_frac=0.1 * (i % 4)) for i in range(n)]


def test_same_bits_whatever_the_route():
    """Neither kernel has an atomic and the order of every sum is fixed: a frame's result is a function of the frame alone."""
    probs = _fixed_set()
    nf = len(probs)
    ref = _resident(probs)                                    # handle with max_frames = nf, max_edges = sum n exactly
    for f, pr in enumerate(probs):                            # ... and it is the right answer
        _check("fixed set %d" % f, pr, ref[f], orc.pose_optimize(pr))
    routes = {}
    po = api.PoseOptimizer(16, 16 * REG_MAX)
    routes["optimize_batch nf=8 + nf=4 (direct)"] = _pack(po.optimize_batch(probs[:8])) + _pack(po.optimize_batch(probs[8:]))
    for k in (9, 10, 11, 12):
        routes["optimize_batch nf=%d (staged)" % k] = _pack(po.optimize_batch(probs[:k])) + ref[k:]
    routes["optimize_batch reversed (staged)"] = _pack(po.optimize_batch(probs[::-1]))[::-1]
    routes["optimize_batch reversed halves (direct)"] = _pack(po.optimize_batch(probs[5::-1]))[::-1] + _pack(po.optimize_batch(probs[:5:-1]))[::-1]
    routes["optimize_batch one frame each"] = [_pack(po.optimize_batch([p]))[0] for p in probs]
    po.close()
    routes["resident reversed"] = _resident(probs[::-1])[::-1]
    routes["resident one frame each"] = [_resident([p])[0] for p in probs]
    routes["one-shot cms_pose_optimize"] = [_pack1(api.pose_optimize(p)) for p in probs]
    fill = _fillers(MAX_BATCH - nf)
    for B in (256, 300):
        batch = list(fill[:B - nf]); where = []
        for j, p in enumerate(probs):
            batch.insert(j * (B // nf) + 5, p)
        for p in probs:
            where.append([i for i, q in enumerate(batch) if q is p][0])
        assert len(batch) == B
        res = _resident(batch)
        routes["resident inside a batch of %d" % B] = [res[i] for i in where]
        po = api.PoseOptimizer(B, sum(len(p["Xw"]) for p in batch))
        res = _pack(po.optimize_batch(batch))
        po.close()
        routes["optimize_batch inside a batch of %d" % B] = [res[i] for i in where]
    for route, res in routes.items():
        assert len(res) == nf, route
        for f in range(nf):
            assert _bits_equal(res[f], ref[f]), (route, f, len(probs[f]["Xw"]), res[f][0], ref[f][0], res[f][3], ref[f][3], res[f][1] - ref[f][1])
    # the in-memory kernel: frames above 1024 edges
    for N, seed in ((1500, 230), (4000, 231)):
        pr = synth.pose_problem(N=N, seed=seed, outlier_frac=0.1)
        r0 = _resident([pr])[0]
        _check("N=%d" % N, pr, r0, orc.pose_optimize(pr))
        po = api.PoseOptimizer(1, N)
        r1 = _pack(po.optimize_batch([pr]))[0]
        po.close()
        r2 = _pack1(api.pose_optimize(pr))
        assert _bits_equal(r1, r0) and _bits_equal(r2, r0), (N, r0[3], r1[3], r2[3])


def test_handle_reuse_and_block_regrowth():
    """ONE handle through calls whose pinned blocks (direct, staging, landing) have to grow, then through smaller calls that reuse the grown blocks,
    then a resident batch with a direct call between launch and two fetches: every result is what a fresh handle gives, and the oracle's."""
    mk = lambda n, N, s: [synth.pose_problem(N=N, seed=s + i, outlier_frac=0.1) for i in range(n)]
    cap_f, cap_e = 12, 12 * REG_MAX
    calls = [("direct 1 x 40", mk(1, 40, 300)), ("direct 8 x 1000", mk(8, 1000, 310)), ("staged 9 x 30", mk(9, 30, 320)),
             ("staged 12 x 1024", mk(12, 1024, 340)), ("staged 1 x 4000", mk(1, 4000, 360)), ("direct 1 x 40 again", mk(1, 40, 300))]

    def fresh(fn):
        h = api.PoseOptimizer(cap_f, cap_e)
        try:
            return fn(h)
        finally:
            h.close()

    def against_oracle(tag, probs, res):
        for f, pr in enumerate(probs):
            _check("%s frame %d" % (tag, f), pr, res[f], orc.pose_optimize(pr))

    po = api.PoseOptimizer(cap_f, cap_e)
    for tag, probs in calls:
        got = _pack(po.optimize_batch(probs))
        want = fresh(lambda h: _pack(h.optimize_batch(probs)))
        assert all(_bits_equal(g, w) for g, w in zip(got, want)), tag
        against_oracle(tag, probs, got)
    resident = mk(10, 500, 370); small = mk(2, 200, 390)
    po.upload(resident); po.launch()
    got_small = _pack(po.optimize_batch(small))
    got_1 = _pack(po.fetch())
    got_2 = _pack(po.fetch())                                  # "may be called again for the same launch"
    po.launch()                                                # ... and launching again restarts from the uploaded poses
    got_3 = _pack(po.fetch())
    po.close()
    want_small = fresh(lambda h: _pack(h.optimize_batch(small)))
    want_res = fresh(lambda h: _pack(h.optimize(resident)))
    assert all(_bits_equal(g, w) for g, w in zip(got_small, want_small))
    for got in (got_1, got_2, got_3):
        assert all(_bits_equal(g, w) for g, w in zip(got, want_res))
    against_oracle("direct call between launch and fetch", small, got_small)
    against_oracle("resident batch", resident, got_1)


@pytest.mark.parametrize("knob", ["CMS_POSE_GLOBAL", "CMS_POSE_COPY_ENGINE"])
def test_matrix_and_routes_under_the_developer_switches(knob):
    """CMS_POSE_GLOBAL: every launch of the resident and staged paths takes k_pose_optimize_g whatever the frame sizes.  CMS_POSE_COPY_ENGINE:
    cms_pose_optimize_batch stages and copies for small calls too.  Both are read once per process: (a) - (c) run again in a child process."""
    env = dict(os.environ)
    env[knob] = "1"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", "matrix_against_the_oracle or same_bits"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def test_pose_error_paths():
    """misuse of cms_pose_upload / cms_pose_optimize_batch / cms_pose_launch / cms_pose_fetch: CMS_ERR_ARG (-1) and a message, nothing read through
    a bad argument, and the handle still works afterwards"""
    L = api.lib()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    pr = synth.pose_problem(N=60, seed=5)
    po = api.PoseOptimizer(2, 200)
    assert L.cms_pose_launch(po.h) == -1 and b"nothing uploaded" in L.cms_last_error()
    assert L.cms_pose_fetch(po.h, None, None, None, None) == -1 and b"nothing launched" in L.cms_last_error()
    Xw = np.ascontiguousarray(np.concatenate([pr["Xw"], pr["Xw"]])); obs = np.ascontiguousarray(np.concatenate([pr["obs"], pr["obs"]]))
    inv = np.ascontiguousarray(np.concatenate([pr["invsig2"], pr["invsig2"]])); face = np.ascontiguousarray(np.concatenate([pr["face"], pr["face"]]))
    bad_face = face.copy(); bad_face[70] = -1
    poses = np.ascontiguousarray(np.stack([pr["pose0"]] * 3))
    I = lambda *v: np.array(v, np.int32)
    good = dict(nf=2, off=I(0, 60, 120), Xw=Xw, obs=obs, inv=inv, face=face)
    cases = [("nf = 0", dict(nf=0), b"bad argument"),
             ("nf > max_frames", dict(nf=3, off=I(0, 40, 80, 120)), b"bad argument"),
             ("null edge_off", dict(off=None), b"bad argument"),
             ("edge_off[0] != 0", dict(off=I(1, 60, 120)), b"cms_pose_upload"),
             ("more edges than the handle holds", dict(off=I(0, 60, 201)), b"capacity"),
             ("decreasing edge_off", dict(off=I(0, 80, 60)), b"decrease"),
             ("null Xw", dict(Xw=None), b"null edge array"), ("null obs", dict(obs=None), b"null edge array"),
             ("null information", dict(inv=None), b"null edge array"), ("null face", dict(face=None), b"null edge array"),
             ("face = -1", dict(face=bad_face), b"unknown face")]
    st = (api.PoseStats * 3)(); out = np.zeros(256, np.uint8); ninl = np.zeros(3, np.int32)
    for tag, change, msg in cases:
        a = dict(good); a.update(change)
        edge = (a["nf"], p(a["off"]), p(a["Xw"]), p(a["obs"]), p(a["inv"]), p(a["face"]), pr["fx"], pr["fy"], pr["cx"], pr["cy"])
        assert L.cms_pose_upload(po.h, *edge, p(poses)) == -1, tag
        assert msg in L.cms_last_error(), (tag, L.cms_last_error())
        got = poses.copy()
        assert L.cms_pose_optimize_batch(po.h, *edge, p(got), p(out), p(ninl), C.byref(st)) == -1, tag
        assert msg in L.cms_last_error(), (tag, L.cms_last_error())
        assert np.array_equal(got, poses), tag
    assert L.cms_pose_optimize_batch(po.h, 2, p(good["off"]), p(Xw), p(obs), p(inv), p(face), pr["fx"], pr["fy"], pr["cx"], pr["cy"], None, p(out),
                                     p(ninl), C.byref(st)) == -1 and b"bad argument" in L.cms_last_error()
    # a failed upload leaves nothing to launch
    assert L.cms_pose_launch(po.h) == -1 and b"nothing uploaded" in L.cms_last_error()
    # the handle still answers, through both entry points
    want = orc.pose_optimize(pr)
    for res in (_pack(po.optimize_batch([pr, pr])), _pack(po.optimize([pr, pr]))):
        for f in range(2):
            _check("after the errors", pr, res[f], want)
    po.close()
