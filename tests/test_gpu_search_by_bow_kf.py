"""ORBMatcher::SearchByBoW(KeyFrame*, KeyFrame*, ...) (src/ORBMatcher.cpp:541-674) on the device: cms_kfstore_search_by_bow_keyframes (resident key
frames, all candidates of a loop-closing pass in one launch) against the CPU restatement tests/npref_bow_kf.py, bit for bit -- both sides are integer
apart from one float32 multiply and the float32 angle arithmetic, which the restatement does in float32 too.  The cases are tests/bow_kf_cases.py's."""
import ctypes as C

import numpy as np
import pytest

import bow_kf_cases as cases
import npref_bow_kf
import vocab_cases as vc
from cubemapslam_amd import api, build, synth

pytestmark = pytest.mark.gpu
KP = api.KP_DTYPE
F = 550
EMPTY_FV = dict(node_id=np.zeros(0, np.int32), node_off=np.zeros(1, np.int32), node_feat=np.zeros(0, np.int32))


def _kf(side):
    """a side of a case as the dict make_keyframe / put_from_frame take (the search reads neither rays nor pose)"""
    n = len(side["mp"])
    kf = dict(x=np.full(n, 100.0, np.float32), y=np.full(n, 100.0, np.float32), octave=np.zeros(n, np.int32), rays=np.zeros((n, 3), np.float32),
              R=np.eye(3, dtype=np.float32), t=np.zeros(3, np.float32), Ow=np.zeros(3, np.float32), median_depth=1.0)
    kf.update(side)
    return kf


def _put(st, slot, side):
    K, keep = api.make_keyframe(_kf(side))
    st.put(slot, K)


@pytest.fixture(scope="module")
def env():
    camd = synth.camera("lafida", F)
    cg = api.Context(camd, nfeatures=2000, max_batch=1)             # the mapping side's context: the store's stream
    ctx = api.Context(camd, nfeatures=2000, max_batch=2)            # the loop-closing thread's
    st = api.KeyframeStore(cg, max_keyframes=8, max_features=4096, max_nodes=2048)
    yield camd, cg, ctx, st
    st.close(); ctx.close(); cg.close()


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]) and got[1] == want[1], (what, got[1], want[1], np.flatnonzero(np.asarray(got[0]) != np.asarray(want[0]))[:10])


def test_hand_built_cases_through_the_device(env):
    camd, cg, ctx, st = env
    for c in cases.HAND:
        _put(st, 0, c["kf1"]); _put(st, 1, c["kf2"])
        got = st.search_by_bow_keyframes(ctx, [(0, len(c["kf1"]["mp"]), 1, len(c["kf2"]["mp"]), c["bad1"], c["bad2"])], nnratio=c["nnratio"], check_orientation=c["ori"])[0]
        _same(got, cases.restate(c), c["name"])
        assert list(got[0]) == c["idx2"] and got[1] == c["n"], c["name"]


@pytest.mark.parametrize("kind", ["coarse", "fine", "many"])
def test_seeded_cases_equal_restatement(env, kind):
    camd, cg, ctx, st = env
    kf1, kf2, bad1, bad2 = cases.seeded_pair(kind)
    _put(st, 2, kf1); _put(st, 3, kf2)
    for k, nnratio, ori in cases.SEEDED:
        if k != kind:
            continue
        want = cases.seeded_reference(kind, nnratio, ori)
        assert want[1] >= 50
        got = st.search_by_bow_keyframes(ctx, [(2, len(kf1["mp"]), 3, len(kf2["mp"]), bad1, bad2)], nnratio=nnratio, check_orientation=ori)[0]
        _same(got, want, (kind, nnratio, ori))


@pytest.fixture(scope="module")
def rendered():
    camd = synth.camera("lafida", F)
    scene = synth.room_scene(0xC0FFEE)
    poses = [synth.room_pose(i, 300) for i in (0, 3)]
    frames = np.stack([synth.render_fisheye(camd, scene, R, t) for R, t in poses])
    fctx = api.Context(camd, nfeatures=2000, max_batch=2)
    fctx.set_mask(synth.cubemap_valid_mask(camd))
    fctx.upload(frames); fctx.process(2, True); fctx.area_grid(2); fctx.sync()
    out = [fctx.fetch(b) for b in range(2)]
    yield fctx, out
    fctx.close()


def _want(s1, s2, bad1, bad2, nnratio, ori):
    n1, n2 = len(s1["mp"]), len(s2["mp"])
    return npref_bow_kf.search_by_bow_kf(s1["angle"], s1["desc"], s1["mp"] >= 0, bad1, s1, s2["angle"], s2["desc"], s2["mp"] >= 0, bad2, s2, nnratio, ori,
                                         npref_bow_kf.feat_node_of(s1, n1), npref_bow_kf.feat_node_of(s2, n2))


def test_slots_filled_from_frames_and_by_compute_bow(env, rendered):
    """slots filled by put, by put_from_frame (asynchronous, on the frame context's stream: the search follows at once from ANOTHER context and waits
    for the copy on the device) and by put_from_frame + KeyFrame::ComputeBoW on the device all take part"""
    camd, cg, ctx, st = env
    fctx, fr = rendered
    assert all(len(k) > 800 for k, _ in fr)
    rng = np.random.default_rng(11)
    sides, bads = [], []
    for k, d in fr:
        n = len(k)
        mp = np.where(rng.random(n) < 0.6, np.arange(n), -1).astype(np.int32)
        sides.append(dict(x=k["x"], y=k["y"], octave=k["octave"], angle=k["angle"], desc=d, mp=mp, **cases._fv_of(d, "fine")))
        bads.append((rng.random(n) < 0.1).astype(np.uint8))
    n1, n2 = len(sides[0]["mp"]), len(sides[1]["mp"])
    want = _want(sides[0], sides[1], bads[0], bads[1], 0.75, True)
    assert want[1] >= 50, want[1]
    _put(st, 0, sides[0]); _put(st, 1, sides[1])
    _same(st.search_by_bow_keyframes(ctx, [(0, n1, 1, n2, bads[0], bads[1])])[0], want, "put")
    st.put_from_frames(fctx, [(4, 0, n1, _kf(sides[0])), (5, 1, n2, _kf(sides[1]))])
    _same(st.search_by_bow_keyframes(ctx, [(4, n1, 5, n2, bads[0], bads[1])])[0], want, "put_from_frames, searched at once from another context")
    _same(st.search_by_bow_keyframes(ctx, [(0, n1, 5, n2, bads[0], bads[1])])[0], want, "put against put_from_frames")
    # KeyFrame::ComputeBoW on the device: the FeatureVector the search reads is the one the store computed
    dv = api.Vocabulary.from_dict(vc.case_tree("k10_L3"))
    for b in range(2):
        st.put_from_frame(6 + b, fctx, b, len(sides[b]["mp"]), _kf(dict(sides[b], **EMPTY_FV)))
    st.compute_bow(dv, [6, 7], 1)
    dev_sides = []
    for b in range(2):
        fvd = st.fetch_bow(6 + b, feature_vector=True)
        assert len(fvd["node_id"]) > 10
        dev_sides.append(dict(sides[b], node_id=fvd["node_id"], node_off=fvd["node_off"], node_feat=fvd["node_feat"]))
    want_dev = _want(dev_sides[0], dev_sides[1], bads[0], bads[1], 0.75, True)
    assert want_dev[1] >= 20, want_dev[1]
    _same(st.search_by_bow_keyframes(ctx, [(6, n1, 7, n2, bads[0], bads[1])])[0], want_dev, "put_from_frame + compute_bow")
    dv.close()


def test_batched_jobs_equal_single_calls(env):
    camd, cg, ctx, st = env
    a1, a2, abad1, abad2 = cases.seeded_pair("fine")
    b1, b2, bbad1, bbad2 = cases.seeded_pair("coarse")
    nonodes = dict(a1, **EMPTY_FV)
    for slot, side in enumerate((a1, a2, b1, b2, nonodes)):
        _put(st, slot, side)
    n = [len(s["mp"]) for s in (a1, a2, b1, b2, nonodes)]
    jobs = [(0, n[0], 1, n[1], abad1, abad2), (1, n[1], 0, n[0], None, None), (2, n[2], 3, n[3], bbad1, None), (3, n[3], 2, n[2], None, bbad1),
            (0, n[0], 4, n[4], None, None),            # key frame 2 without nodes
            (4, n[4], 1, n[1], None, None),            # key frame 1 without nodes
            (1, n[1], 1, n[1], None, abad2),           # slot1 == slot2: every feature with a map point finds itself at distance 0
            (0, n[0], 1, n[1], None, None)]
    sides = (a1, a2, b1, b2, nonodes)
    got = st.search_by_bow_keyframes(ctx, jobs)
    assert len(got) == 8
    for job, g in zip(jobs, got):
        _same(st.search_by_bow_keyframes(ctx, [job])[0], g, job[:4])
        _same(g, _want(sides[job[0]], sides[job[2]], job[4], job[5], 0.75, True), job[:4])
        assert len(g[0]) == job[1]
    assert got[4][1] == 0 and got[5][1] == 0 and (got[4][0] == -1).all() and (got[5][0] == -1).all()
    assert got[0][1] >= 50 and got[2][1] >= 50 and got[6][1] >= 50
    again = st.search_by_bow_keyframes(ctx, jobs)
    for g, h in zip(got, again):
        assert g[0].tobytes() == h[0].tobytes() and g[1] == h[1]


def test_error_paths_leave_the_outputs_untouched(env):
    camd, cg, ctx, st = env
    kf1, kf2, bad1, bad2 = cases.seeded_pair("fine")
    _put(st, 2, kf1); _put(st, 3, kf2)
    n1, n2 = len(kf1["mp"]), len(kf2["mp"])
    L = api.lib()
    L.cms_kfstore_search_by_bow_keyframes.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_void_p]
    L.cms_last_error.restype = C.c_char_p
    free = api.KeyframeStore(cg, max_keyframes=2, max_features=64, max_nodes=8)      # a store whose slots were never filled

    def call(store, src, jobs):
        arr = (api.BowKfJob * len(jobs))()
        for q, (s1, c1, s2, c2) in zip(arr, jobs):
            q.slot1 = s1; q.n1 = c1; q.slot2 = s2; q.n2 = c2; q.skip1 = None; q.skip2 = None
        idx2 = np.full(sum(max(j[1], 0) for j in jobs) + 1, -7, np.int32); nm = np.full(len(jobs), -7, np.int32)
        rc = L.cms_kfstore_search_by_bow_keyframes(store, src, len(jobs), arr, 0.75, 1, idx2.ctypes.data_as(C.c_void_p), nm.ctypes.data_as(C.c_void_p))
        return rc, idx2, nm

    good = (2, n1, 3, n2)
    bad_calls = [(st.h, ctx.h, [(-1, n1, 3, n2)]), (st.h, ctx.h, [(2, n1, 8, n2)]),          # a slot out of range, on either side
                 (st.h, ctx.h, [(2, n1 - 1, 3, n2)]), (st.h, ctx.h, [(2, n1, 3, n2 + 1)]),     # n1 / n2 that is not the slot's stored count
                 (st.h, ctx.h, [good, (2, n1, 3, 0)]),                                         # ... in a later job of the call
                 (free.h, ctx.h, [(0, 0, 1, 0)]),                                              # a slot not filled
                 (st.h, None, [good]), (None, ctx.h, [good])]                                  # no context / no store
    for store, src, jobs in bad_calls:
        rc, idx2, nm = call(store, src, jobs)
        assert rc == -1 and (idx2 == -7).all() and (nm == -7).all(), jobs
        assert b"cms_kfstore_search_by_bow_keyframes" in L.cms_last_error()
    import torch
    if torch.cuda.device_count() > 1:                                                          # a context on another device than the store's
        other = api.Context(camd, nfeatures=500, max_batch=1, device=1)
        rc, idx2, nm = call(st.h, other.h, [good])
        assert rc == -1 and (idx2 == -7).all() and (nm == -7).all()
        other.close()
    rc, idx2, nm = call(st.h, ctx.h, [])                                                       # an empty call: CMS_OK, nothing written
    assert rc == 0 and (idx2 == -7).all()
    rc, idx2, nm = call(st.h, ctx.h, [good])                                                   # after the errors the next valid call is correct
    want = _want(kf1, kf2, None, None, 0.75, True)
    assert rc == 0 and nm[0] == want[1] and np.array_equal(idx2[:n1], want[0]) and idx2[n1] == -7
    free.close()


def test_mirror_search_by_bow_keyframes_equals_restatement():
    build.build(verbose=False)
    api.lib()
    L = C.CDLL(build.HOST_LIB)
    L.hm_last_error.restype = C.c_char_p
    L.hm_extract.argtypes = [C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    side_args = [C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 3
    L.hm_search_by_bow_keyframes.argtypes = side_args + side_args + [C.c_float, C.c_int, C.c_void_p]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    Fm = 150
    cam = api.make_camera(synth.camera("lafida", Fm))
    assert L.hm_set_camera(C.byref(cam)) == 0
    W = 3 * Fm                                                      # the mirror's shared context is sized by the ORBextractor a key frame's features come from
    img = np.ascontiguousarray(synth.texture(W, W, 70)); msk = np.full((W, W), 255, np.uint8)
    k0 = np.zeros(1500, KP); d0 = np.zeros((1500, 32), np.uint8)
    assert L.hm_extract(1000, 1.2, 8, 20, 7, p(img), W, p(msk), W, p(k0), p(d0), 1500) > 0, L.hm_last_error()
    kf1, kf2, bad1, bad2 = cases.seeded_pair("coarse")
    args, keep = [], []
    for s, bad in ((kf1, bad1), (kf2, bad2)):
        n = len(s["mp"])
        kk = np.zeros(n, KP); kk["x"] = s["x"]; kk["y"] = s["y"]; kk["octave"] = s["octave"]; kk["angle"] = s["angle"]
        arrs = [kk, np.ascontiguousarray(s["desc"]), s["mp"].astype(np.int64), bad, s["node_id"], s["node_off"], s["node_feat"]]
        keep.append(arrs)
        args += [n, p(arrs[0]), p(arrs[1]), p(arrs[2]), p(arrs[3]), len(arrs[4]), p(arrs[4]), p(arrs[5]), p(arrs[6])]
    out = np.full(len(kf1["mp"]), -7, np.int64)
    nm = L.hm_search_by_bow_keyframes(*args, 0.75, 1, p(out))
    assert nm >= 0, L.hm_last_error()
    want_idx, want_n = cases.seeded_reference("coarse", 0.75, True)
    want = np.where(want_idx >= 0, kf2["mp"].astype(np.int64)[np.maximum(want_idx, 0)], -1)
    assert nm == want_n and want_n >= 50 and np.array_equal(out, want)
    assert (want[want_idx >= 0] >= 0).all()                         # a match always carries a map point of key frame 2
