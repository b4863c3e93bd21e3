"""The window query (Frame::GetFeaturesInArea on the device) in two launches: one search that leaves every query's count, its first
CMS_AREA_TMP candidates and one partial sum per workgroup; one kernel that derives the CSR offsets per tile of queries and writes the
lists (copied first hits, or a second search for the few queries with more).  Every expectation here is the oracle's
(orc.features_in_area / orc.fuse_search); the class assertions are conditions on the inputs, checked on the oracle's counts alone."""
import functools

import numpy as np
import pytest

import orc
import test_area_emu as te
from cubemapslam_amd import api, synth

pytestmark = pytest.mark.gpu

TMP = 8            # CMS_AREA_TMP (cubemapslam_amd/csrc/cms_area_kernels.hip): first hits kept per query
GUARD = 64
SENTINEL = -123456789

# (F, key points, their seed, queries); the queries' seed is 30 + the key points' seed
CASES = ((550, 2000, 21, 5000), (150, 2000, 22, 5000), (150, 2000, 22, 40000), (150, 600, 23, 1025))


@functools.lru_cache(maxsize=None)
def _case(F, n, seed, nq):
    """key points, queries and the oracle's lists -- computed once, shared by the tests, never modified"""
    camd = synth.camera("lafida", F)
    ocam = orc.make_camera(camd)
    kx, ky, ko = te._keypoints(F, n, seed)
    q5 = te._queries(F, nq, 30 + seed)[:5]
    off, idx = orc.features_in_area(ocam, kx, ky, ko, *q5, cap=n * nq + 16)
    for a in (kx, ky, ko, off, idx) + tuple(q5):
        a.setflags(write=False)
    return dict(F=F, camd=camd, ocam=ocam, kp=(kx, ky, ko), q5=q5, off=off, idx=idx)


def _prefix(case, nq):
    off = case["off"][:nq + 1]
    return tuple(a[:nq] for a in case["q5"]), off, case["idx"][:off[-1]]


def _assert_classes(cnt, F, what):
    assert (cnt == 0).any(), what
    assert ((cnt >= 1) & (cnt < TMP)).any(), what
    assert (cnt == TMP).any(), what
    assert (cnt == TMP + 1).any(), what
    if F == 150:
        assert (cnt > 64).any(), what            # crowded columns: more than four hits in one cell column


def _context(case, max_batch=2, slot=1):
    ctx = api.Context(case["camd"], nfeatures=2000, max_batch=max_batch)
    kx, ky, ko = case["kp"]
    kps = np.zeros(len(kx), api.KP_DTYPE); kps["x"] = kx; kps["y"] = ky; kps["octave"] = ko
    ctx.area_set_keypoints(slot, kps)
    for b in range(max_batch):
        if b != slot:
            ctx.area_set_keypoints(b, kps[:7])
    ctx.area_grid(max_batch)
    return ctx


def _query(ctx, b, q5, cap, qframe=None, idx_base=0):
    """device-pointer entry -> cnt, off, idx (cap + GUARD words, pre-filled with a sentinel), total"""
    import torch
    dev = torch.device("cuda", 0)
    nq = len(q5[0])
    dq = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in q5]
    d_cnt = torch.full((nq,), SENTINEL, dtype=torch.int32, device=dev)
    d_off = torch.full((nq + 1,), SENTINEL, dtype=torch.int32, device=dev)
    d_idx = torch.full((cap + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    d_tot = torch.full((1,), SENTINEL, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ptrs = [t.data_ptr() for t in dq]
    if qframe is None:
        ctx.features_in_area_device(b, nq, ptrs, d_cnt.data_ptr(), d_off.data_ptr(), d_idx.data_ptr(), cap, idx_base, d_tot.data_ptr())
    else:
        d_qf = torch.from_numpy(np.ascontiguousarray(qframe, np.int32)).to(dev)
        torch.cuda.synchronize()
        ctx.features_in_area_batch_device(nq, d_qf.data_ptr(), ptrs, d_cnt.data_ptr(), d_off.data_ptr(), d_idx.data_ptr(), cap, d_tot.data_ptr())
    ctx.sync()
    return d_cnt.cpu().numpy(), d_off.cpu().numpy(), d_idx.cpu().numpy(), int(d_tot.item())


def _assert_equal(got, want_off, want_idx, cap, what):
    cnt, off, idx, total = got
    n = len(want_idx)
    assert total == n, (what, total, n)
    assert np.array_equal(off, want_off), what
    assert np.array_equal(cnt, np.diff(want_off)), what
    m = min(cap, n)
    assert np.array_equal(idx[:m], want_idx[:m]), (what, int((idx[:m] != want_idx[:m]).sum()))
    assert (idx[m:] == SENTINEL).all(), what                                   # nothing behind the lists, nothing at or beyond cap


def test_lists_at_the_boundaries():
    """0, 1..7, exactly CMS_AREA_TMP, CMS_AREA_TMP + 1 and hundreds of candidates per window; one query, one wavefront of the scan
    more or less, one tile more or less, many tiles; 'no window' queries (r < 0) in between."""
    for spec in CASES:
        case = _case(*spec)
        _assert_classes(np.diff(case["off"]), case["F"], spec)
        ctx = _context(case)
        cap = len(case["idx"])
        _assert_equal(_query(ctx, 1, case["q5"], cap), case["off"], case["idx"], cap, spec)
        if spec == CASES[1]:
            for nq in (1, 31, 32, 33, 1023, 1024):
                q5, off, idx = _prefix(case, nq)
                _assert_equal(_query(ctx, 1, q5, max(len(idx), 1)), off, idx, max(len(idx), 1), (spec, nq))
            # r = -1 on a tenth of the queries: empty lists there, the others' lists move up
            qx, qy, qr, lo, hi = case["q5"]
            none = np.arange(len(qx)) % 10 == 3
            cnt = np.where(none, 0, np.diff(case["off"]))
            assert (np.diff(case["off"])[none] > TMP).any() and (np.diff(case["off"])[none] > 0).sum() > 100
            off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
            keep = np.repeat(~none, np.diff(case["off"]))
            idx = case["idx"][keep]
            got = _query(ctx, 1, (qx, qy, np.where(none, np.float32(-1), qr).astype(np.float32), lo, hi), cap)
            _assert_equal(got, off, idx, cap, "no-window queries")
        ctx.close()


def test_capacity_is_respected_and_the_total_is_true():
    case = _case(*CASES[1])
    ctx = _context(case)
    total = len(case["idx"])
    assert total > 50000
    for cap in (total, total - 1, total // 2, 0):
        _assert_equal(_query(ctx, 1, case["q5"], cap), case["off"], case["idx"], cap, ("cap", cap))
    ctx.close()


def test_batch_entry_lists_are_rows_of_the_batch():
    """three frame slots with 2000, 7 and 0 key points; the queries name their slot in no particular order"""
    case = _case(*CASES[1])
    kx, ky, ko = case["kp"]
    ctx = api.Context(case["camd"], nfeatures=2000, max_batch=3)
    kps = np.zeros(len(kx), api.KP_DTYPE); kps["x"] = kx; kps["y"] = ky; kps["octave"] = ko
    ctx.area_set_keypoints(0, kps); ctx.area_set_keypoints(1, kps[:7]); ctx.area_set_keypoints(2, kps[:0])
    ctx.area_grid(3)
    kp_cap = ctx.geom.kp_cap
    nq = len(case["q5"][0])
    qframe = np.random.RandomState(77).randint(0, 3, nq).astype(np.int32)
    assert (np.diff(qframe) < 0).any() and all((qframe == f).sum() > 1000 for f in range(3))
    off7, idx7 = orc.features_in_area(case["ocam"], kx[:7], ky[:7], ko[:7], *case["q5"])
    per = [(case["off"], case["idx"]), (off7, idx7)]
    lists = [per[f][1][per[f][0][q]:per[f][0][q + 1]] + f * kp_cap if f < 2 else np.zeros(0, np.int32) for q, f in enumerate(qframe)]
    want_off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    want_idx = np.concatenate(lists).astype(np.int32)
    assert len(idx7) > 0 and (np.diff(want_off)[qframe == 0] > TMP).any() and (np.diff(want_off)[qframe == 1] > 0).any()
    cap = len(want_idx)
    _assert_equal(_query(ctx, 0, case["q5"], cap, qframe=qframe), want_off, want_idx, cap, "batch")
    ctx.close()


def test_buffers_are_reused_and_regrown_without_leftovers():
    """one context: 40 000 queries, then 33, then 5000 -- the first-hits and partial-sum buffers keep values of the earlier call"""
    big, small = _case(*CASES[2]), _case(*CASES[1])
    assert big["kp"][0] is small["kp"][0] or np.array_equal(big["kp"][0], small["kp"][0])      # the same frame
    ctx = _context(small)
    q5, off, idx = _prefix(small, 33)
    for what, (q, o, i) in (("5000 first", (small["q5"], small["off"], small["idx"])), ("40000", (big["q5"], big["off"], big["idx"])),
                            ("33", (q5, off, idx)), ("5000", (small["q5"], small["off"], small["idx"]))):
        _assert_equal(_query(ctx, 1, q, len(i)), o, i, len(i), what)
    ctx.close()


def _fuse_window_counts(ocam, kx, ky, ko, sf, pose15, skip, pr, th):
    """ORBMatcher::Fuse: radius th x scale of the predicted level around the projection, every level -- candidates per window, by the
    oracle alone (as _fuse_window_total of test_gpu_parity.py counts them)"""
    fr = orc.is_in_frustum(ocam, pose15, pr["pos"], pr["normal"], pr["min_dist"], pr["max_dist"])
    v = (fr["in_view"] > 0) & (np.asarray(skip) == 0)
    r = (np.float32(th) * sf[fr["level"]]).astype(np.float32)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    m1 = np.full(int(v.sum()), -1, np.int32)
    off, _ = orc.features_in_area(ocam, kx, ky, ko, f32(fr["proj_x"][v]), f32(fr["proj_y"][v]), f32(r[v]), m1, m1, cap=int(v.sum()) * len(kx) + 16)
    return np.diff(off)


def test_store_fuse_with_small_and_large_windows():
    """cms_kfstore_fuse_search / _sets on a dense F = 150 key frame: windows with at most CMS_AREA_TMP candidates (copied first hits) and
    with more (searched again) in ONE call that stays under the first-guess capacity, so the first attempt is the one that returns"""
    F, TH = 150, 5.0
    camd = synth.camera("lafida", F)
    ocam = orc.make_camera(camd)
    ctx = api.Context(camd, nfeatures=2000, max_batch=1)
    store = api.KeyframeStore(ctx, max_keyframes=3, max_features=2048, max_nodes=16)
    kfs, prs, oks, skips = [], [], [], []
    for s in range(2):
        kx, ky, ko = te._keypoints(F, 1900, 301 + 10 * s)
        kd = synth.descriptors(len(kx), 302 + 10 * s)
        pr = synth.local_map_problem(F, kx, ky, ko, kd, seed=305 + 10 * s)
        kf = dict(x=kx, y=ky, octave=ko, angle=np.zeros(len(kx), np.float32), desc=kd, mp=np.full(len(kx), -1, np.int32), R=pr["pose15"][:9], t=pr["pose15"][9:12],
                  Ow=pr["pose15"][12:], node_id=np.zeros(0, np.int32), node_off=np.zeros(1, np.int32), node_feat=np.zeros(0, np.int32), median_depth=1.0,
                  rays=np.zeros((len(kx), 3), np.float32))
        K, _keep = api.make_keyframe(kf)
        store.put(s + 1, K)                                     # slots 1 and 2 (slot 0 stays empty)
        kfs.append(kf); prs.append(pr); oks.append(orc.make_keyframe(ocam, kf))
        skips.append((np.arange(len(pr["pos"])) % (11 + 2 * s) == 0).astype(np.uint8))
    sf = prs[0]["scale_factors"]; inv_s2 = (np.float32(1.0) / (sf * sf)).astype(np.float32)
    jobs, want, cnts = [], [], []
    for slot_i, src in ((0, 0), (1, 1), (0, 1)):                # the last job searches key frame 0 with the map points made for key frame 1
        q = prs[src]
        jobs.append((slot_i + 1, dict(skip=skips[src], pos=q["pos"], normal=q["normal"], min_dist=q["min_dist"], max_dist=q["max_dist"], desc=q["desc"])))
        want.append(orc.fuse_search(ocam, oks[slot_i][0], skips[src], q["pos"], q["normal"], q["min_dist"], q["max_dist"], q["desc"], TH, sf, inv_s2))
        cnts.append(_fuse_window_counts(ocam, kfs[slot_i]["x"], kfs[slot_i]["y"], kfs[slot_i]["octave"], sf, prs[slot_i]["pose15"], skips[src], q, TH))
    nmp = sum(len(j[1]["pos"]) for j in jobs)
    for c in cnts:                                              # both classes in every job, and the whole call under the first guess
        assert ((c > 0) & (c <= TMP)).sum() > 50 and (c > TMP).sum() > 50, ((c <= TMP).sum(), (c > TMP).sum())
    assert sum(int(c.sum()) for c in cnts) < 64 * nmp + 1024
    got = store.fuse_search(jobs, th=TH)
    for j in range(3):
        assert np.array_equal(got[j][0], want[j][0]) and np.array_equal(got[j][1], want[j][1]), (j, int((got[j][0] != want[j][0]).sum()))
    assert sum((w[0] >= 0).sum() for w in want) > 500
    sets = [jobs[0][1], jobs[1][1]]
    sjobs = [(1, 0, skips[0]), (2, 1, skips[1]), (1, 1, skips[1])]
    got_s = store.fuse_search_sets(sets, sjobs, th=TH)
    for j in range(3):
        assert np.array_equal(got_s[j][0], want[j][0]) and np.array_equal(got_s[j][1], want[j][1]), ("sets", j)
    store.close(); ctx.close()


def test_store_fuse_limit_and_reprojection_gate_by_hand():
    """cms_kfstore_fuse_search_sets on a scene small enough to state the answer: what separates Fuse's instantiation of the window scan from
    its two Sim3 siblings -- TH_LOW = 50 (not 100) and the 5.99 chi-square gate on the reprojection error (the siblings have none).
    Identity pose, F = 150 (f = 75, front face at +150): the points project onto dyadic pixels exactly; max_dist = dist3D puts every
    point on level 0 (or 1 at worst: octave 0 passes either way), radius th >= 8 px around the projection.
      point 0 -> (225, 225);       key point 0 there,         Hamming 50           -> key point 0, distance 50
      point 1 -> (243.75, 225);    key point 1 there,         Hamming 51           -> -1, 256
      point 2 -> (206.25, 243.75); key point 2 at (+5, +1),   Hamming 10, e2 = 26  -> -1, 256   (26 / sigma2[0] = 26 > 5.99)"""
    F = 150
    camd = synth.camera("lafida", F)
    ctx = api.Context(camd, nfeatures=2000, max_batch=1)
    store = api.KeyframeStore(ctx, max_keyframes=2, max_features=2048, max_nodes=16)
    pos = np.array([[0.0, 0.0, 2.0], [0.5, 0.0, 2.0], [-0.5, 0.5, 2.0]], np.float32)
    kx = np.array([225.0, 243.75, 206.25 + 5.0], np.float32)
    ky = np.array([225.0, 225.0, 243.75 + 1.0], np.float32)
    bits = lambda k: np.packbits(np.arange(256) < k).astype(np.uint8)
    kd = np.stack([bits(50), bits(51), bits(10)])
    dist = np.sqrt((pos.astype(np.float64) ** 2).sum(1)).astype(np.float32)
    pose15 = np.concatenate([np.eye(3, dtype=np.float32).ravel(), np.zeros(6, np.float32)])
    kf = dict(x=kx, y=ky, octave=np.zeros(3, np.int32), angle=np.zeros(3, np.float32), desc=kd, mp=np.full(3, -1, np.int32), R=pose15[:9], t=pose15[9:12],
              Ow=pose15[12:], node_id=np.zeros(0, np.int32), node_off=np.zeros(1, np.int32), node_feat=np.zeros(0, np.int32), median_depth=1.0,
              rays=np.zeros((3, 3), np.float32))
    K, _keep = api.make_keyframe(kf)
    store.put(1, K)
    mset = dict(pos=pos, normal=(pos / dist[:, None]).astype(np.float32), min_dist=(np.float32(0.5) * dist).astype(np.float32), max_dist=dist,
                desc=np.zeros((3, 32), np.uint8))
    (best_idx, best_dist), = store.fuse_search_sets([mset], [(1, 0, np.zeros(3, np.uint8))], th=8.0)
    print("best_idx", best_idx, "best_dist", best_dist)
    assert best_idx.tolist() == [0, -1, -1]
    assert best_dist.tolist() == [50, 256, 256]
    store.close(); ctx.close()
