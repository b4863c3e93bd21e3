"""ORBMatcher::SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th) (src/ORBMatcher.cpp:796-903) and the search half of
ORBMatcher::Fuse(KeyFrame*, Scw, vpPoints, th, vpReplacePoint) (:1246-1363) on the device: cms_kfstore_search_by_projection_sim3 and
cms_kfstore_fuse_search_sim3 (resident key frames, shared sets of map points, many jobs in one call) against the CPU restatement
tests/npref_sim3_projection.py.  Every comparison is np.array_equal on the index arrays plus equality of the counts and of best_dist.  The cases are
tests/sim3_projection_cases.py's."""
import ctypes as C

import numpy as np
import pytest

import sim3_projection_cases as cases
from cubemapslam_amd import api, build, synth

pytestmark = pytest.mark.gpu
KP = api.KP_DTYPE
F = cases.F


def _kf(kf):
    """a key frame of a case as the dict make_keyframe / put_from_frames take: the STORED pose is the case's decoy (the search reads neither it, nor
    rays, nor the FeatureVector)"""
    n = len(kf["kx"])
    p = np.asarray(kf["pose12"], np.float32)
    return dict(x=kf["kx"], y=kf["ky"], octave=kf["koct"], angle=np.zeros(n, np.float32), desc=kf["kdesc"], rays=np.zeros((n, 3), np.float32),
                mp=np.full(n, -1, np.int32), R=p[:9].reshape(3, 3), t=p[9:], Ow=np.zeros(3, np.float32), median_depth=1.0,
                node_id=np.zeros(0, np.int32), node_off=np.zeros(1, np.int32), node_feat=np.zeros(0, np.int32))


def _put(st, slot, kf):
    K, keep = api.make_keyframe(_kf(kf))
    st.put(slot, K)


def _job(c, slot, set=0, **kw):
    return dict(dict(slot=slot, n=len(c["kf"]["kx"]), Scw=c["Scw"], set=set, skip=c["skip"], taken=c["taken"]), **kw)


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (what, np.flatnonzero(np.asarray(got[0]) != np.asarray(want[0]))[:10], got[1], want[1])


@pytest.fixture(scope="module")
def env():
    cg = api.Context(cases.CAMD, nfeatures=2000, max_batch=1)       # the mapping side's context: the store's stream
    ctx = api.Context(cases.CAMD, nfeatures=2000, max_batch=2)      # the loop-closing thread's
    assert np.array_equal(np.array(cg.geom.scale[:8], np.float32), cases.SF) and cg.geom.nlevels == 8
    st = api.KeyframeStore(cg, max_keyframes=10, max_features=2048, max_nodes=8)
    yield cg, ctx, st
    st.close(); ctx.close(); cg.close()


def _both(st, ctx, c, slot=0, pts=None):
    """(SearchByProjection, Fuse) of a case alone"""
    _put(st, slot, c["kf"])
    pts = c["pts"] if pts is None else pts
    return (st.search_by_projection_sim3(ctx, [pts], [_job(c, slot)], th=c["th"])[0], st.fuse_search_sim3(ctx, [pts], [_job(c, slot)], th=c["th"])[0])


def test_hand_built_cases(env):
    cg, ctx, st = env
    for name, c, match, best, dist in cases.hand_cases():
        dist = [10 if b >= 0 else 256 for b in best] if dist is None else dist
        sbp, fuse = _both(st, ctx, c)
        assert list(sbp[0]) == match and sbp[1] == sum(m >= 0 for m in match), (name, list(sbp[0]), match)
        assert list(fuse[0]) == best and list(fuse[1]) == dist, (name, list(fuse[0]), best, list(fuse[1]), dist)
        _same(sbp, cases.run_sbp(c), name)
        _same(fuse, cases.run_fuse(c), name)


def test_seeded_cases_equal_restatement(env):
    cg, ctx, st = env
    for c in cases.family():
        taken = c["taken"].copy()
        sbp, fuse = _both(st, ctx, c)
        _same(sbp, cases.run_sbp(c), ("SearchByProjection", len(c["skip"])))
        _same(fuse, cases.run_fuse(c), ("Fuse", len(c["skip"])))
        assert np.array_equal(taken, c["taken"])                      # `taken` is not written by the call
        fuse4 = st.fuse_search_sim3(ctx, [c["pts"]], [_job(c, 0)], th=4.0)[0]      # SearchAndFuse's own radius
        _same(fuse4, cases.run_fuse(dict(c, th=4.0)), ("Fuse, th 4", len(c["skip"])))


def test_greedy_rounds_are_reported(env):
    cg, ctx, st = env
    c = cases.family()[2]
    info = {}
    want = cases.run_sbp(c, info)
    _put(st, 0, c["kf"])
    _same(st.search_by_projection_sim3(ctx, [c["pts"]], [_job(c, 0)], th=c["th"])[0], want, "1031 key points")
    assert api.lib().cms_sim3_proj_last_rounds() >= 3 and info["depth"] >= 3


def test_distance_bounds_from_the_getters(env):
    """cms_set_distance_bounds_mode(1) on the calling context: the same case with the getters' values gives the same matches"""
    cg, ctx, st = env
    c = cases.family()[1]
    want = (cases.run_sbp(c, bounds_scaled=1), cases.run_fuse(c, bounds_scaled=1))
    _same(want[0], cases.run_sbp(c), "the restatement's two modes")
    ctx.set_distance_bounds_mode(1)
    try:
        got = _both(st, ctx, c, pts=cases.scaled_pts(c["pts"]))
    finally:
        ctx.set_distance_bounds_mode(0)
    _same(got[0], want[0], "scaled bounds, SearchByProjection")
    _same(got[1], want[1], "scaled bounds, Fuse")


def test_dense_windows_repeat_the_call(env):
    cg, ctx, st = env
    c = cases.dense_case()
    info = {}
    want = cases.run_sbp(c, info)
    assert info["ncand"] > 64 * info["entries"] + 1024               # the first capacity (64 per entry + 1024) is too small: the call runs twice
    sbp, fuse = _both(st, ctx, c)
    _same(sbp, want, "dense, SearchByProjection")
    _same(fuse, cases.run_fuse(c), "dense, Fuse")
    assert want[1] >= 50


def _many(st):
    kfs, sets, jobs = cases.many_jobs()
    for slot, kf in enumerate(kfs):
        _put(st, slot, kf)
    listed = [dict(slot=s, n=len(kfs[s]["kx"]), Scw=S, set=k, skip=skip, taken=taken) for s, S, k, skip, taken in jobs]
    return kfs, sets, jobs, listed


def test_many_jobs_in_one_call_equal_single_calls(env):
    cg, ctx, st = env
    kfs, sets, jobs, listed = _many(st)
    for entry, run in ((st.search_by_projection_sim3, cases.run_sbp), (st.fuse_search_sim3, cases.run_fuse)):
        got = entry(ctx, sets, listed, th=cases.TH)
        assert len(got) == len(listed)
        for g, q, j in zip(got, listed, jobs):
            _same(g, entry(ctx, sets, [q], th=cases.TH)[0], (q["slot"], q["set"], "alone"))
            _same(g, run(cases.job_case(kfs, sets, j)), (q["slot"], q["set"]))
            assert len(g[0]) == len(sets[q["set"]]["pos"])
        again = entry(ctx, sets, listed, th=cases.TH)                 # a repeated call gives identical output
        for g, h in zip(got, again):
            assert g[0].tobytes() == h[0].tobytes() and np.asarray(g[1]).tobytes() == np.asarray(h[1]).tobytes()
        assert entry(ctx, sets, []) == []
    got = st.search_by_projection_sim3(ctx, sets, listed, th=cases.TH)
    assert got[3][1] == 0 and (got[3][0] == -1).all() and len(got[5][0]) == 0 and got[5][1] == 0      # n = 0; an empty set


def test_pinned_and_pageable_result_arrays(env):
    cg, ctx, st = env
    c = cases.family()[1]
    n = len(c["skip"])
    _put(st, 0, c["kf"])
    pa, pb = api.PinnedArray(4 * (n + 2)), api.PinnedArray(4 * (n + 2))
    for a, b in ((np.zeros(n + 2, np.int32), np.zeros(n + 2, np.int32)), (pa.array.view(np.int32), pb.array.view(np.int32))):
        a[:] = -7; b[:] = -7
        want = cases.run_sbp(c)
        got = st.search_by_projection_sim3(ctx, [c["pts"]], [_job(c, 0)], th=c["th"], out=(a, b))[0]
        _same(got, want, "through the caller's arrays")
        assert np.array_equal(a[:n], want[0]) and (a[n:] == -7).all() and b[0] == want[1] and (b[1:] == -7).all()
        a[:] = -7; b[:] = -7
        want = cases.run_fuse(c)
        got = st.fuse_search_sim3(ctx, [c["pts"]], [_job(c, 0)], th=c["th"], out=(a, b))[0]
        _same(got, want, "through the caller's arrays")
        assert np.array_equal(a[:n], want[0]) and np.array_equal(b[:n], want[1]) and (a[n:] == -7).all() and (b[n:] == -7).all()
    pa.close(); pb.close()


def test_error_paths(env):
    cg, ctx, st = env
    c = cases.family()[0]
    n, nk = len(c["skip"]), len(c["kf"]["kx"])
    _put(st, 0, c["kf"])
    free = api.KeyframeStore(cg, max_keyframes=2, max_features=64, max_nodes=8)      # a store whose slots were never filled
    bad_scw = lambda k, v: np.concatenate([c["Scw"].reshape(-1)[:k], [v], c["Scw"].reshape(-1)[k + 1:]]).astype(np.float32)
    for name, entry, run in (("cms_kfstore_search_by_projection_sim3", st.search_by_projection_sim3, cases.run_sbp), ("cms_kfstore_fuse_search_sim3", st.fuse_search_sim3, cases.run_fuse)):
        a = np.full(2 * n + 1, -7, np.int32); b = np.full(2 * n + 1, -7, np.int32)

        def refused(reason, store=None, th=10.0, sets=None, jobs=None, **kw):
            e_ = entry if store is None else getattr(store, entry.__name__)
            with pytest.raises(api.CmsError) as e:
                e_(ctx, [c["pts"]] if sets is None else sets, [dict(_job(c, 0), **kw)] if jobs is None else jobs, th=th, out=(a, b))
            assert "(-1)" in str(e.value) and name + ": " + reason in str(e.value), str(e.value)
            assert (a == -7).all() and (b == -7).all()                # refused before anything was written or enqueued
        refused("empty slot", store=free, n=0)
        refused("slot out of range", slot=10)
        refused("slot out of range", slot=-1)
        refused("n is not the slot's stored key-point count", n=nk - 1)
        refused("set out of range", set=1)
        refused("set out of range", set=-1)
        refused("scw must be finite and nonzero", Scw=np.zeros(12, np.float32))
        refused("Scw must be finite", Scw=bad_scw(5, np.nan))
        refused("Scw must be finite", Scw=bad_scw(3, np.inf))
        refused("th must be finite and >= 0", th=-1.0)
        refused("th must be finite and >= 0", th=float("nan"))
        refused("n is not the slot's stored key-point count", jobs=[_job(c, 0), dict(_job(c, 0), n=nk + 1)])      # a later job: the first one's outputs are untouched too
        got = entry(ctx, [c["pts"]], [_job(c, 0)], th=c["th"], out=(a, b))[0]      # after the errors the next valid call is correct
        _same(got, run(c), "after the refusals")
        assert a[n] == -7
    # set offsets that do not ascend cannot be built through the wrapper: the C entry itself
    L = api.lib()
    L.cms_last_error.restype = C.c_char_p
    soff = np.array([0, n, n - 1], np.int32)
    arr = (api.Sim3ProjJob * 1)()
    arr[0].slot = 0; arr[0].n = nk; arr[0].set = 0; arr[0].Scw[:] = [float(v) for v in c["Scw"].reshape(-1)]
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    pts = c["pts"]
    a = np.full(n, -7, np.int32); b = np.full(n, -7, np.int32)
    L.cms_kfstore_fuse_search_sim3.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 2 + [C.c_float, C.c_void_p, C.c_void_p]
    rc = L.cms_kfstore_fuse_search_sim3(st.h, ctx.h, 2, p(soff), p(pts["pos"]), p(pts["normal"]), p(pts["min_dist"]), p(pts["max_dist"]), p(pts["desc"]), 1, arr, None, 4.0, p(a), p(b))
    assert rc == -1 and b"set offsets must ascend" in L.cms_last_error() and (a == -7).all()
    rc = L.cms_kfstore_fuse_search_sim3(st.h, ctx.h, 1, p(soff), None, p(pts["normal"]), p(pts["min_dist"]), p(pts["max_dist"]), p(pts["desc"]), 1, arr, None, 4.0, p(a), p(b))
    assert rc == -1 and b"null array where entries exist" in L.cms_last_error() and (a == -7).all()
    free.close()


def test_store_beyond_the_claim_table_is_refused(env):
    cg, ctx, st = env
    big = api.KeyframeStore(cg, max_keyframes=1, max_features=4100, max_nodes=8)
    c = cases.family()[0]
    _put(big, 0, c["kf"])
    with pytest.raises(api.CmsError) as e:
        big.search_by_projection_sim3(ctx, [c["pts"]], [_job(c, 0)])
    assert "max_features exceeds the claim table" in str(e.value)
    _same(big.fuse_search_sim3(ctx, [c["pts"]], [_job(c, 0)], th=c["th"])[0], cases.run_fuse(c), "Fuse has no claim table")
    big.close()


def test_context_on_another_device_is_refused(env):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    cg, ctx, st = env
    c = cases.family()[0]
    _put(st, 0, c["kf"])
    other = api.Context(cases.CAMD, nfeatures=500, max_batch=1, device=1)
    for entry in (st.search_by_projection_sim3, st.fuse_search_sim3):
        with pytest.raises(api.CmsError) as e:
            entry(other, [c["pts"]], [_job(c, 0)])
        assert "the context and the store must share the device" in str(e.value)
    other.close()


def test_rendered_pair_on_a_second_stream(env):
    """A frame of the room is extracted on the device and becomes a key frame through put_from_frames (asynchronous, on the frame context's stream); the
    searches follow at once on ANOTHER context's stream and wait for the copies on the device -- the loop-closing thread's configuration.  The points
    are the room's geometry behind the key points of a second frame; Scw is 1.3 times the key frame's true pose."""
    cg, ctx, st = env
    scene = synth.room_scene(0xC0FFEE)
    poses = [synth.room_pose(i, 300) for i in (0, 3)]
    frames = np.stack([synth.render_fisheye(cases.CAMD, scene, R, t) for R, t in poses])
    fctx = api.Context(cases.CAMD, nfeatures=1000, max_batch=2)
    fctx.set_mask(synth.cubemap_valid_mask(cases.CAMD))
    fctx.upload(frames); fctx.process(2, True); fctx.area_grid(2); fctx.sync()
    rng = np.random.default_rng(21)
    (R0, t0), (R1, t1) = poses
    k0, d0 = fctx.fetch(0)
    k1, d1 = fctx.fetch(1)
    n0, n1 = len(k0), len(k1)
    assert 300 < n0 <= 2048 and n1 > 300
    ok, Xw = synth.room_points_behind_pixels(F, R1, t1, k1["x"].astype(np.float64), k1["y"].astype(np.float64))
    O1 = -R1.T @ t1
    dist = np.linalg.norm(Xw @ R0.T + t0, axis=1)                     # seen from the key frame
    mx = (dist * 1.2 ** (k1["octave"] + rng.uniform(-0.8, 0.2, n1))).astype(np.float32)
    nrm = (Xw - O1) / np.maximum(np.linalg.norm(Xw - O1, axis=1), 1e-9)[:, None]
    pts = dict(pos=Xw.astype(np.float32), normal=nrm.astype(np.float32), min_dist=(mx / np.float32(1.2 ** 7)).astype(np.float32), max_dist=mx, desc=np.ascontiguousarray(d1))
    kf = dict(kx=k0["x"].copy(), ky=k0["y"].copy(), koct=k0["octave"].astype(np.int32), kdesc=np.ascontiguousarray(d0), pose12=cases.STORED.copy())
    c = dict(camd=cases.CAMD, sf=cases.SF, kf=kf, Scw=cases.make_scw(1.3, R0, 1.3 * t0), pts=pts, skip=(~ok | (rng.random(n1) < 0.1)).astype(np.uint8),
             taken=(rng.random(n0) < 0.1).astype(np.uint8), th=cases.TH)
    want = cases.run_sbp(c), cases.run_fuse(c)
    assert want[0][1] >= 20, want[0][1]
    st.put_from_frames(fctx, [(7, 0, n0, _kf(kf))])
    _same(st.search_by_projection_sim3(ctx, [pts], [_job(c, 7)], th=c["th"])[0], want[0], "searched at once from another context")
    _same(st.fuse_search_sim3(ctx, [pts], [_job(c, 7)], th=c["th"])[0], want[1], "Fuse")
    _put(st, 9, kf)
    _same(st.search_by_projection_sim3(ctx, [pts], [_job(c, 9)], th=c["th"])[0], want[0], "put_from_frames against put")
    fctx.close()


def test_mirror_equals_the_abi_and_the_restatement():
    """ORBMatcher::SearchByProjection(KeyFrameView, Scw, ...) and ORBMatcher::Fuse(KeyFrameView, Scw, ...) of the host mirror through hm_*: vpMatched and
    vpReplacePoint / the key frame's map points are left as the restatement plus the reference's pointer rules say"""
    build.build(verbose=False)
    api.lib()
    L = C.CDLL(build.HOST_LIB)
    L.hm_last_error.restype = C.c_char_p
    L.hm_extract.argtypes = [C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    L.hm_search_by_projection_sim3.argtypes = [C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 7 + [C.c_int, C.c_void_p]
    L.hm_fuse_sim3.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 7 + [C.c_float, C.c_void_p]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    cam = api.make_camera(cases.CAMD)
    assert L.hm_set_camera(C.byref(cam)) == 0
    W = 3 * F                                                       # the mirror's shared context is sized by the ORBextractor a key frame's features come from
    img = np.ascontiguousarray(synth.texture(W, W, 70)); msk = np.full((W, W), 255, np.uint8)
    k0 = np.zeros(3000, KP); d0 = np.zeros((3000, 32), np.uint8)
    assert L.hm_extract(2000, 1.2, 8, 20, 7, p(img), W, p(msk), W, p(k0), p(d0), 3000) > 0, L.hm_last_error()
    c = cases.family()[1]
    rng = np.random.default_rng(8)
    n, nk = len(c["skip"]), len(c["kf"]["kx"])
    pts = c["pts"]
    kk = np.zeros(nk, KP); kk["x"] = c["kf"]["kx"]; kk["y"] = c["kf"]["ky"]; kk["octave"] = c["kf"]["koct"]
    kdesc = np.ascontiguousarray(c["kf"]["kdesc"])
    Scw = np.ascontiguousarray(c["Scw"], np.float32)
    ids = (1000 + np.arange(n)).astype(np.int64)
    # the case's skipped points: half are bad, the others sit in the key frame already (at key points taken on entry); the other taken key points
    # hold foreign points
    sk = np.flatnonzero(c["skip"]); tk = np.flatnonzero(c["taken"])
    bad = np.zeros(n, np.uint8); bad[sk[::2]] = 1
    inside = sk[1::2]
    assert len(inside) <= len(tk) and len(inside) >= 3
    held = np.full(nk, -1, np.int64)
    held[tk] = 9000 + np.arange(len(tk)); held[tk[:len(inside)]] = ids[inside]
    arrs = [pts["pos"], pts["normal"], pts["min_dist"], pts["max_dist"], np.ascontiguousarray(pts["desc"]), ids, bad]
    # ---- SearchByProjection: vpMatched on entry = held
    matched = held.copy()
    nm = L.hm_search_by_projection_sim3(nk, p(kk), p(kdesc), p(Scw), n, *[p(a) for a in arrs], int(c["th"]), p(matched))
    assert nm >= 0, L.hm_last_error()
    m, want_n = cases.run_sbp(c)
    want = held.copy(); want[m[m >= 0]] = ids[m >= 0]
    assert nm == want_n and want_n >= 50 and np.array_equal(matched, want) and (held[m[m >= 0]] == -1).all()
    # ---- Fuse: the key frame's map points on entry = held, a third of the foreign ones bad (GetMapPoints leaves them out; a hit on one replaces nothing)
    kf_bad = np.zeros(nk, np.uint8); kf_bad[tk[len(inside)::3]] = 1
    kf_mp = held.copy(); replace = np.full(n, -1, np.int64)
    nf = L.hm_fuse_sim3(nk, p(kk), p(kdesc), p(kf_mp), p(kf_bad), p(Scw), n, *[p(a) for a in arrs], float(c["th"]), p(replace))
    assert nf >= 0, L.hm_last_error()
    bi, _ = cases.run_fuse(c)
    want_mp = held.copy(); want_rep = np.full(n, -1, np.int64); want_nf = 0
    for i in np.flatnonzero(bi >= 0):                                 # :1345-1359 in list order
        if want_mp[bi[i]] >= 0:
            if not kf_bad[bi[i]]:
                want_rep[i] = want_mp[bi[i]]
        else:
            want_mp[bi[i]] = ids[i]
        want_nf += 1
    assert nf == want_nf and np.array_equal(kf_mp, want_mp) and np.array_equal(replace, want_rep)
    assert (want_rep >= 0).sum() >= 5 and (want_mp != held).sum() >= 50
