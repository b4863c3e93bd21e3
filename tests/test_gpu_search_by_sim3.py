"""ORBMatcher::SearchBySim3 (src/ORBMatcher.cpp:1365-1586) on the device: cms_kfstore_search_by_sim3 (resident key frames, every accepted hypothesis
of a loop-closing pass in one call) against the CPU restatement tests/npref_sim3_search.py.  Every comparison is np.array_equal on idx2 and equality
of n_found, in both modes of z_as_written.  The cases are tests/sim3_search_cases.py's."""
import ctypes as C

import numpy as np
import pytest

import sim3_search_cases as cases
from cubemapslam_amd import api, build, synth

pytestmark = pytest.mark.gpu
KP = api.KP_DTYPE
F = cases.F
MODES = (False, True)


def _kf(kf, mp):
    """a key frame of a case as the dict make_keyframe / put_from_frames take (the search reads neither rays nor the FeatureVector)"""
    n = len(kf["kx"])
    p = np.asarray(kf["pose12"], np.float32)
    return dict(x=kf["kx"], y=kf["ky"], octave=kf["koct"], angle=np.zeros(n, np.float32), desc=kf["kdesc"], rays=np.zeros((n, 3), np.float32),
                mp=np.where(np.asarray(mp["skip"]) == 0, 1, -1).astype(np.int32), R=p[:9].reshape(3, 3), t=p[9:], Ow=np.zeros(3, np.float32), median_depth=1.0,
                node_id=np.zeros(0, np.int32), node_off=np.zeros(1, np.int32), node_feat=np.zeros(0, np.int32))


def _put(st, slot, kf, mp):
    K, keep = api.make_keyframe(_kf(kf, mp))
    st.put(slot, K)


def _job(c, slot1, slot2, **kw):
    return dict(dict(slot1=slot1, slot2=slot2, s12=c["s12"], R12=c["R12"], t12=c["t12"], mp1=c["mp1"], mp2=c["mp2"]), **kw)


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]) and got[1] == want[1], (what, got[1], want[1], np.flatnonzero(np.asarray(got[0]) != np.asarray(want[0]))[:10])


@pytest.fixture(scope="module")
def env():
    cg = api.Context(cases.CAMD, nfeatures=2000, max_batch=1)       # the mapping side's context: the store's stream
    ctx = api.Context(cases.CAMD, nfeatures=2000, max_batch=2)      # the loop-closing thread's
    assert np.array_equal(np.array(cg.geom.scale[:8], np.float32), cases.SF) and cg.geom.nlevels == 8
    st = api.KeyframeStore(cg, max_keyframes=10, max_features=2048, max_nodes=8)
    yield cg, ctx, st
    st.close(); ctx.close(); cg.close()


def _alone(st, ctx, c, zw, slots=(0, 1)):
    _put(st, slots[0], c["kf1"], c["mp1"])
    if slots[1] != slots[0]:
        _put(st, slots[1], c["kf2"], c["mp2"])
    return st.search_by_sim3(ctx, [_job(c, *slots)], th=c["th"], z_as_written=zw)[0]


@pytest.mark.parametrize("zw", MODES, ids=["corrected", "as_written"])
def test_hand_built_cases(env, zw):
    cg, ctx, st = env
    for name, c, want in cases.hand_cases(zw):
        got = _alone(st, ctx, c, zw)
        assert list(got[0]) == want and got[1] == sum(w >= 0 for w in want), (name, list(got[0]), want)
        _same(got, cases.run(c, zw), name)
        _same(_alone(st, ctx, c, not zw), cases.run(c, not zw), (name, "the other mode"))


@pytest.mark.parametrize("written", MODES, ids=["corrected_family", "as_written_family"])
def test_seeded_cases_equal_restatement(env, written):
    cg, ctx, st = env
    total = 0
    for c in cases.family(written):
        for zw in MODES:
            want = cases.run(c, zw)
            _same(_alone(st, ctx, c, zw), want, (written, len(c["kf1"]["kx"]), zw))
            total += want[1] if zw == written else 0
    assert total >= 50


def test_distance_bounds_from_the_getters(env):
    """cms_set_distance_bounds_mode(1) on the calling context: the same case with the getters' values gives the same matches"""
    cg, ctx, st = env
    c = cases.family(True)[1]
    want = cases.run(c, True, bounds_scaled=1)
    _same(want, cases.run(c, True), "the restatement's two modes")
    sc = lambda m: dict(m, min_dist=(np.float32(0.8) * m["min_dist"]).astype(np.float32), max_dist=(np.float32(1.2) * m["max_dist"]).astype(np.float32))
    ctx.set_distance_bounds_mode(1)
    try:
        got = _alone(st, ctx, dict(c, mp1=sc(c["mp1"]), mp2=sc(c["mp2"])), True)
    finally:
        ctx.set_distance_bounds_mode(0)
    _same(got, want, "scaled bounds")


def test_dense_windows_repeat_the_call(env):
    cg, ctx, st = env
    c = cases.dense_case()
    for zw in MODES:
        info = {}
        want = cases.run(c, zw, info)
        assert info["ncand"] > 64 * info["entries"] + 1024           # the first capacity (64 per entry + 1024) is too small: the call runs twice
        _same(_alone(st, ctx, c, zw), want, ("dense", zw))
    assert cases.run(c, False)[1] >= 50


def test_many_jobs_in_one_call_equal_single_calls(env):
    cg, ctx, st = env
    a, b, w = cases.family(False)[0], cases.family(False)[1], cases.family(True)[2]
    nothing = cases.empty_side_case(a, True)                          # a key frame without key points as key frame 1
    for slot, (kf, mp) in enumerate(((a["kf1"], a["mp1"]), (a["kf2"], a["mp2"]), (b["kf1"], b["mp1"]), (b["kf2"], b["mp2"]), (w["kf1"], w["mp1"]), (w["kf2"], w["mp2"]),
                                     (nothing["kf1"], nothing["mp1"]))):
        _put(st, slot, kf, mp)
    me = cases.self_case(b)
    swapped = dict(b, kf1=b["kf2"], kf2=b["kf1"], mp1=b["mp2"], mp2=b["mp1"])      # the same similarity the other way round: a different problem
    listed = [(a, 0, 1), (b, 2, 3), (nothing, 6, 1), (w, 4, 5), (me, 2, 2), (swapped, 3, 2), (cases.empty_side_case(a, False), 0, 6)]
    for zw in MODES:
        jobs = [_job(c, s1, s2) for c, s1, s2 in listed]
        got = st.search_by_sim3(ctx, jobs, z_as_written=zw)
        assert len(got) == len(listed)
        for g, (c, s1, s2) in zip(got, listed):
            _same(g, st.search_by_sim3(ctx, [_job(c, s1, s2)], z_as_written=zw)[0], (s1, s2, zw, "alone"))
            _same(g, cases.run(c, zw), (s1, s2, zw))
            assert len(g[0]) == len(c["kf1"]["kx"])
        assert got[2][1] == 0 and got[6][1] == 0 and (got[6][0] == -1).all()
        again = st.search_by_sim3(ctx, jobs, z_as_written=zw)             # a repeated call gives identical output
        for g, h in zip(got, again):
            assert g[0].tobytes() == h[0].tobytes() and g[1] == h[1]
    assert st.search_by_sim3(ctx, []) == []


def test_pinned_and_pageable_result_arrays(env):
    cg, ctx, st = env
    c = cases.family(False)[1]
    n1 = len(c["kf1"]["kx"])
    want = cases.run(c, False)
    _put(st, 0, c["kf1"], c["mp1"]); _put(st, 1, c["kf2"], c["mp2"])
    pin_i, pin_n = api.PinnedArray(4 * (n1 + 2)), api.PinnedArray(8)
    for idx2, nf in ((np.full(n1 + 2, -7, np.int32), np.full(2, -7, np.int32)), (pin_i.array.view(np.int32), pin_n.array.view(np.int32))):
        idx2[:] = -7; nf[:] = -7
        got = st.search_by_sim3(ctx, [_job(c, 0, 1)], z_as_written=False, out=(idx2, nf))[0]
        _same(got, want, "through the caller's arrays")
        assert np.array_equal(idx2[:n1], want[0]) and (idx2[n1:] == -7).all() and nf[0] == want[1] and nf[1] == -7
    pin_i.close(); pin_n.close()


def test_error_paths(env):
    cg, ctx, st = env
    c = cases.family(False)[0]
    n1, n2 = len(c["kf1"]["kx"]), len(c["kf2"]["kx"])
    _put(st, 0, c["kf1"], c["mp1"]); _put(st, 1, c["kf2"], c["mp2"])
    want = cases.run(c, False)
    L = api.lib()
    L.cms_last_error.restype = C.c_char_p
    free = api.KeyframeStore(cg, max_keyframes=2, max_features=64, max_nodes=8)      # a store whose slots were never filled
    idx2 = np.full(n1 + 1, -7, np.int32); nf = np.full(1, -7, np.int32)

    def refused(store, reason, th=7.5, n_mp=None, **kw):
        with pytest.raises(api.CmsError) as e:
            store.search_by_sim3(ctx, [dict(_job(c, 0, 1), **kw)], th=th, z_as_written=False, out=(idx2, nf), n_mp=n_mp)
        assert "(-1)" in str(e.value) and "cms_kfstore_search_by_sim3: " + reason in str(e.value), str(e.value)
        assert (idx2 == -7).all() and (nf == -7).all()                # refused before anything was written or enqueued
    refused(free, "empty slot", n1=0, n2=0)
    refused(st, "slot out of range", slot1=10)
    refused(st, "n1 / n2 is not the slot's stored key-point count", n1=n1 - 1)
    refused(st, "n1 / n2 is not the slot's stored key-point count", n2=n2 + 1)
    refused(st, "off2 does not ascend or reaches beyond n_mp", n_mp=n1 + n2 - 1)
    refused(st, "off1 does not ascend or reaches beyond n_mp", off1=-1)
    refused(st, "off2 does not ascend or reaches beyond n_mp", off2=n1 - 1)
    refused(st, "s12 must be finite and nonzero", s12=0.0)
    refused(st, "s12 must be finite and nonzero", s12=float("nan"))
    refused(st, "th must be finite and >= 0", th=-1.0)
    idx2b = np.full(2 * n1 + 1, -7, np.int32); nfb = np.full(2, -7, np.int32)
    with pytest.raises(api.CmsError):                                 # a later job of the call is refused: the first one's outputs are untouched too
        st.search_by_sim3(ctx, [_job(c, 0, 1), dict(_job(c, 0, 1), s12=0.0)], z_as_written=False, out=(idx2b, nfb))
    assert (idx2b == -7).all() and (nfb == -7).all()
    got = st.search_by_sim3(ctx, [_job(c, 0, 1)], z_as_written=False, out=(idx2, nf))[0]      # after the errors the next valid call is correct
    _same(got, want, "after the refusals")
    assert idx2[n1] == -7
    free.close()


def test_context_on_another_device_is_refused(env):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device")
    cg, ctx, st = env
    c = cases.family(False)[0]
    _put(st, 0, c["kf1"], c["mp1"]); _put(st, 1, c["kf2"], c["mp2"])
    other = api.Context(cases.CAMD, nfeatures=500, max_batch=1, device=1)
    with pytest.raises(api.CmsError) as e:
        st.search_by_sim3(other, [_job(c, 0, 1)])
    assert "the context and the store must share the device" in str(e.value)
    other.close()


def test_rendered_pair_on_a_second_stream(env):
    """Two frames of the room are extracted on the device and become key frames through put_from_frames (asynchronous, on the frame context's stream);
    the search follows at once on ANOTHER context's stream and waits for the copies on the device -- the loop-closing thread's configuration.  The map
    points are the room's geometry behind the key points; the similarity is the true relative pose."""
    cg, ctx, st = env
    scene = synth.room_scene(0xC0FFEE)
    poses = [synth.room_pose(i, 300) for i in (0, 3)]
    frames = np.stack([synth.render_fisheye(cases.CAMD, scene, R, t) for R, t in poses])
    fctx = api.Context(cases.CAMD, nfeatures=1000, max_batch=2)
    fctx.set_mask(synth.cubemap_valid_mask(cases.CAMD))
    fctx.upload(frames); fctx.process(2, True); fctx.area_grid(2); fctx.sync()
    rng = np.random.default_rng(21)
    kfs, mps = [], []
    for b, (R, t) in enumerate(poses):
        k, d = fctx.fetch(b)
        n = len(k)
        assert 300 < n <= 2048
        ok, Xw = synth.room_points_behind_pixels(F, R, t, k["x"].astype(np.float64), k["y"].astype(np.float64))
        pose12 = np.concatenate([R.reshape(-1), t]).astype(np.float32)
        dist = np.linalg.norm(Xw @ R.T + t, axis=1)
        mx = (dist * 1.2 ** (k["octave"] + rng.uniform(-0.8, 0.2, n))).astype(np.float32)
        kfs.append(dict(kx=k["x"].copy(), ky=k["y"].copy(), koct=k["octave"].astype(np.int32), kdesc=np.ascontiguousarray(d), pose12=pose12))
        mps.append(dict(skip=(~ok | (rng.random(n) < 0.2)).astype(np.uint8), pos=Xw.astype(np.float32), min_dist=(mx / np.float32(1.2 ** 7)).astype(np.float32), max_dist=mx,
                        desc=np.ascontiguousarray(d)))
    (R1, t1), (R2, t2) = poses
    R12 = R1 @ R2.T
    c = dict(camd=cases.CAMD, sf=cases.SF, kf1=kfs[0], kf2=kfs[1], s12=np.float32(1.0), R12=R12.astype(np.float32), t12=(t1 - R12 @ t2).astype(np.float32), mp1=mps[0], mp2=mps[1],
             th=cases.TH)
    want = {zw: cases.run(c, zw) for zw in MODES}
    assert want[False][1] >= 20, want[False][1]
    st.put_from_frames(fctx, [(7, 0, len(kfs[0]["kx"]), _kf(kfs[0], mps[0])), (8, 1, len(kfs[1]["kx"]), _kf(kfs[1], mps[1]))])
    _same(st.search_by_sim3(ctx, [_job(c, 7, 8)], z_as_written=False)[0], want[False], "searched at once from another context")
    _same(st.search_by_sim3(ctx, [_job(c, 7, 8)], z_as_written=True)[0], want[True], "as written")
    _put(st, 9, kfs[1], mps[1])
    _same(st.search_by_sim3(ctx, [_job(c, 7, 9)], z_as_written=False)[0], want[False], "put_from_frames against put")
    fctx.close()


def test_mirror_equals_the_abi_and_the_restatement():
    build.build(verbose=False)
    api.lib()
    L = C.CDLL(build.HOST_LIB)
    L.hm_last_error.restype = C.c_char_p
    L.hm_extract.argtypes = [C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    side = [C.c_int] + [C.c_void_p] * 9
    L.hm_search_by_sim3.argtypes = side + side + [C.c_float, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    cam = api.make_camera(cases.CAMD)
    assert L.hm_set_camera(C.byref(cam)) == 0
    W = 3 * F                                                       # the mirror's shared context is sized by the ORBextractor a key frame's features come from
    img = np.ascontiguousarray(synth.texture(W, W, 70)); msk = np.full((W, W), 255, np.uint8)
    k0 = np.zeros(3000, KP); d0 = np.zeros((3000, 32), np.uint8)
    assert L.hm_extract(2000, 1.2, 8, 20, 7, p(img), W, p(msk), W, p(k0), p(d0), 3000) > 0, L.hm_last_error()
    c = cases.family(True)[1]
    rng = np.random.default_rng(8)
    n1, n2 = len(c["kf1"]["kx"]), len(c["kf2"]["kx"])
    # ids: a key point whose record is skipped holds no map point, or (a few) a bad one
    ids, bads = [], []
    for base, mp in ((1000, c["mp1"]), (5000, c["mp2"])):
        n = len(mp["skip"])
        bad = ((mp["skip"] != 0) & (rng.random(n) < 0.3)).astype(np.uint8)
        ids.append(np.where((mp["skip"] == 0) | (bad != 0), base + np.arange(n), -1).astype(np.int64)); bads.append(bad)
    # vpMatches12 on entry: twelve pairs SearchByBoW found before; their key points are out on both sides (:1390-1400)
    i1 = rng.choice(np.flatnonzero(c["mp1"]["skip"] == 0), 12, replace=False); i2 = rng.choice(np.flatnonzero(c["mp2"]["skip"] == 0), 12, replace=False)
    matches = np.full(n1, -1, np.int64); matches[i1] = ids[1][i2]
    entry = matches.copy()
    args, keep = [], []
    for kf, mp, idv, bad in ((c["kf1"], c["mp1"], ids[0], bads[0]), (c["kf2"], c["mp2"], ids[1], bads[1])):
        n = len(kf["kx"])
        kk = np.zeros(n, KP); kk["x"] = kf["kx"]; kk["y"] = kf["ky"]; kk["octave"] = kf["koct"]
        Tcw = np.eye(4, dtype=np.float32); Tcw[:3, :3] = kf["pose12"][:9].reshape(3, 3); Tcw[:3, 3] = kf["pose12"][9:]
        arrs = [kk, np.ascontiguousarray(kf["kdesc"]), Tcw, idv, bad, np.ascontiguousarray(mp["pos"]), mp["min_dist"], mp["max_dist"], np.ascontiguousarray(mp["desc"])]
        keep.append(arrs)
        args += [n] + [p(a) for a in arrs]
    R12 = np.ascontiguousarray(c["R12"], np.float32); t12 = np.ascontiguousarray(c["t12"], np.float32)
    nm = L.hm_search_by_sim3(*args, float(c["s12"]), p(R12), p(t12), float(c["th"]), 1, p(matches))
    assert nm >= 0, L.hm_last_error()
    s1 = c["mp1"]["skip"].copy(); s1[i1] = 1
    s2 = c["mp2"]["skip"].copy(); s2[i2] = 1
    want_idx, want_n = cases.run(dict(c, mp1=dict(c["mp1"], skip=s1), mp2=dict(c["mp2"], skip=s2)), True)
    want = entry.copy()
    want[want_idx >= 0] = ids[1][want_idx[want_idx >= 0]]
    assert nm == want_n and want_n >= 40 and np.array_equal(matches, want)
    assert (want[want_idx >= 0] >= 5000).all() and (entry[want_idx >= 0] == -1).all()
