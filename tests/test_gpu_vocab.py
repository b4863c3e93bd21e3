"""ComputeBoW on the device (cms_vocab_*, cms_frames_compute_bow / fetch_bow, cms_kfstore_compute_bow / fetch_bow / search_by_bow_frames) against the host
build of the same core (csrc/cms_vocab_core.h through libcubemapslam_host.so) on the same inputs.  Every output must be bit-equal: words, values as raw
float64 bits, node ids, offsets, feature lists -- both sides are integer or IEEE-rounded.  The shapes are tests/vocab_cases.py's: the smallest at which
each mechanism can go wrong."""
import numpy as np
import pytest

import npref_vocab as ref
import vocab_cases as vc
import vocab_hostlib as hl
from cubemapslam_amd import api, synth

pytestmark = pytest.mark.gpu
KP = api.KP_DTYPE
F = 150


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(synth.camera("lafida", F), nfeatures=2500, max_batch=8)
    assert c.geom.kp_cap >= 2000
    yield c
    c.close()


_vocabs = {}


def _pair(name):
    """(device vocabulary, host vocabulary) of a case, made once"""
    if name not in _vocabs:
        t = vc.case_tree(name)
        _vocabs[name] = (api.Vocabulary.from_dict(t), hl.HostVocabulary(t))
    return _vocabs[name]


@pytest.fixture(scope="module", autouse=True)
def _close_vocabs():
    yield
    for dv, hv in _vocabs.values():
        dv.close(); hv.close()
    _vocabs.clear()


def _place(ctx, b, desc):
    """n descriptors (and as many key points) into row b of the context, as if the batch had extracted them"""
    n = len(desc)
    k = np.zeros(max(n, 1), KP)
    k["x"] = 10 + (np.arange(max(n, 1)) % 400); k["y"] = 10 + (np.arange(max(n, 1)) // 400)
    ctx.area_set_keypoints(b, k[:n])
    if n:
        ctx.area_set_descriptors(b, desc)


def _same(want, got, what):
    d = ref.first_difference(want, got)
    assert d is None, (what, d)


@pytest.mark.parametrize("name", sorted(vc.CASES))
def test_device_equals_host_core(ctx, name):
    dv, hv = _pair(name)
    _, ns, levelsups = vc.CASES[name]
    for n in ns:
        d = vc.case_descriptors(name, n)
        for lu in levelsups:
            want = hv.transform(d, lu)
            _same(want, dv.transform(ctx, d, lu), (name, n, lu, "cms_vocab_transform"))
            _place(ctx, 1, d)
            ctx.compute_bow(dv, [1], [n], lu)
            _same(want, ctx.fetch_bow(1), (name, n, lu, "cms_frames_compute_bow"))


def test_vocab_info(ctx):
    dv, _ = _pair("k17_L2")
    t = vc.case_tree("k17_L2")
    i = dv.info()
    assert (i["k"], i["L"], i["scoring"], i["weighting"], i["nodes"], i["words"], i["device"]) == (17, 2, 0, 0, len(t["parent"]), int(t["is_leaf"].sum()), 0)


def test_all_words_stopped(ctx):
    dv, hv = _pair("all_stopped")
    d = vc.case_descriptors("k10_L3", 257)
    got = dv.transform(ctx, d, 1)
    _same(hv.transform(d, 1), got, "all stopped")
    assert len(got["word_id"]) == 0 and len(got["node_id"]) == 0 and list(got["node_off"]) == [0] and len(got["node_feat"]) == 0


def test_repeated_descriptor(ctx):
    d = vc.repeated_descriptor()
    t = vc.case_tree("k10_L3")
    for scoring in (vc.L1_NORM, vc.DOT_PRODUCT):
        tt = vc.with_weights(t, scoring=scoring)
        dv, hv = api.Vocabulary.from_dict(tt), hl.HostVocabulary(tt)
        got = dv.transform(ctx, d, 1)
        _same(hv.transform(d, 1), got, ("repeated", scoring))
        assert len(got["word_id"]) == 1 and list(got["node_feat"]) == list(range(300))
        dv.close()


def test_full_size_tree(ctx):
    """ORBvoc.txt's shape (k = 10, L = 6, 1.1 M nodes): index width and layout"""
    dv, hv = _pair("full_size")
    d = vc.case_descriptors("full_size", 300)
    got = dv.transform(ctx, d, 4)
    _same(hv.transform(d, 4), got, "full size")
    assert got["word_id"].max() > 500000


def test_batch_equals_single_rows(ctx):
    dv, hv = _pair("k10_L3")
    ns = [0, 1, 63, 64, 65, 257, 2000, 700]
    descs = [vc.descriptors(50 + b, vc.case_tree("k10_L3"), n) for b, n in enumerate(ns)]
    for b, d in enumerate(descs):
        _place(ctx, b, d)
    ctx.compute_bow(dv, list(range(8)), ns, 1)
    batch = [ctx.fetch_bow(b) for b in range(8)]
    for b in (7, 3, 0, 5, 1, 6, 2, 4):      # one row per call, in another order
        ctx.compute_bow(dv, [b], [ns[b]], 1)
        single = ctx.fetch_bow(b)
        _same(single, batch[b], ("batch vs single", b))
        _same(hv.transform(descs[b], 1), batch[b], ("batch vs host", b))


@pytest.fixture(scope="module")
def extracted():
    """four overlapping views through the real frame path: key points, descriptors, rays and the frame grid are on the device"""
    camd = synth.camera("lafida", F)
    B = 4
    c = api.Context(camd, nfeatures=800, max_batch=B)
    c.set_mask(synth.cubemap_valid_mask(camd, erode=5, band=30))
    base = synth.texture(camd["Ih"], camd["Iw"], 3)
    c.upload(np.stack([np.roll(base, 2 * b, axis=1) for b in range(B)])); c.process(B, True); c.area_grid(B); c.sync()
    fr = [c.fetch(b) for b in range(B)]
    assert all(len(k) > 100 for k, _ in fr)
    yield camd, c, fr
    c.close()


def _kf(k, d, fv, seed):
    rng = np.random.default_rng(seed)
    n = len(k)
    mp = np.where(rng.random(n) < 0.6, np.arange(n), -1).astype(np.int32)
    t = np.array([0.05 * seed, 0.0, 0.0], np.float32)
    return dict(mp=mp, R=np.eye(3, dtype=np.float32), t=t, Ow=-t, median_depth=2.0, **fv)


EMPTY_FV = dict(node_id=np.zeros(0, np.int32), node_off=np.zeros(1, np.int32), node_feat=np.zeros(0, np.int32))


def test_resident_path(extracted):
    camd, c, fr = extracted
    dv, hv = _pair("k10_L3")
    cg = api.Context(camd, nfeatures=800, max_batch=1)      # the mapping side's context
    B = len(fr)
    st = api.KeyframeStore(cg, max_keyframes=2 * B, max_features=1024, max_nodes=256)
    host = [hv.transform(d, 1) for _, d in fr]
    assert all(len(h["node_id"]) > 10 for h in host)
    fvs = [dict(node_id=h["node_id"], node_off=h["node_off"], node_feat=h["node_feat"]) for h in host]
    # slots 0..B-1: put with the host core's FeatureVector; slots B..2B-1: put without one, then KeyFrame::ComputeBoW on the device
    st.put_from_frames(c, [(b, b, len(fr[b][0]), _kf(fr[b][0], fr[b][1], fvs[b], b)) for b in range(B)])
    st.put_from_frames(c, [(B + b, b, len(fr[b][0]), _kf(fr[b][0], fr[b][1], EMPTY_FV, b)) for b in range(B)])
    st.compute_bow(dv, [B + b for b in range(B)], 1)
    for b in range(B):
        a, g = st.debug_fetch(b), st.debug_fetch(B + b)
        assert sorted(a) == sorted(g)
        for key in a:
            if key == "header":      # the record's offsets name the slot: f0, node0, noff0, nfeat0 differ by construction
                assert np.array_equal(np.delete(a[key], [0, 2, 4, 5]), np.delete(g[key], [0, 2, 4, 5])), (b, key)
            else:
                assert np.asarray(a[key]).tobytes() == np.asarray(g[key]).tobytes(), (b, key)
        wid, wval = st.fetch_bow(B + b)
        assert np.array_equal(wid, host[b]["word_id"]) and np.array_equal(wval.view(np.uint64), host[b]["word_val"].view(np.uint64))
    # Frame::ComputeBoW for all rows, then SearchByBoW with the resident FeatureVector against the same search given the fetched one
    ns = [len(k) for k, _ in fr]
    c.compute_bow(dv, list(range(B)), ns, 1)
    rng = np.random.default_rng(2)
    jobs, jobs_host = [], []
    for b in range(B):
        slot = B + (b + 1) % B
        skip = (rng.random(ns[(b + 1) % B]) < 0.1).astype(np.uint8)
        got_fv = c.fetch_bow(b)
        _same(host[b], got_fv, ("frame row", b))
        jobs.append((slot, b, ns[b], skip)); jobs_host.append((slot, b, ns[b], got_fv, skip))
    res = st.search_by_bow_frames(c, jobs)
    res_host = st.search_by_bow(c, jobs_host)
    assert sum(r[1] for r in res_host) > 20
    for r, w in zip(res, res_host):
        assert np.array_equal(r[0], w[0]) and r[1] == w[1]
    # CreateNewMapPoints on the two sets of slots: identical records
    rec_a = st.create_new_map_points([(0, [1, 2, 3])])
    rec_g = st.create_new_map_points([(B, [B + 1, B + 2, B + 3])])
    for x, y in zip(rec_a[0], rec_g[0]):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
    st.close(); cg.close()


def test_error_paths(extracted, ctx):
    camd, c, fr = extracted
    dv, hv = _pair("k10_L3")
    cg = api.Context(camd, nfeatures=800, max_batch=1)
    # max_nodes overflow leaves the slot unchanged (levelsup 0: one node per word, far more than 8)
    st = api.KeyframeStore(cg, max_keyframes=2, max_features=1024, max_nodes=8)
    k, d = fr[0]
    h = hv.transform(d, 3)      # the root alone: fits
    st.put_from_frames(c, [(0, 0, len(k), _kf(k, d, dict(node_id=h["node_id"], node_off=h["node_off"], node_feat=h["node_feat"]), 1))])
    before = st.debug_fetch(0)
    with pytest.raises(api.CmsError) as e:
        st.compute_bow(dv, [0], 0)
    assert "(-4)" in str(e.value)
    after = st.debug_fetch(0)
    assert all(np.asarray(before[key]).tobytes() == np.asarray(after[key]).tobytes() for key in before)
    with pytest.raises(api.CmsError):
        st.fetch_bow(0)                       # no BowVector was committed
    st.compute_bow(dv, [0], 3)                # ... and the call that fits goes through
    assert np.array_equal(st.fetch_bow(0)[0], h["word_id"])
    with pytest.raises(api.CmsError):
        st.compute_bow(dv, [1], 1)            # empty slot
    # a row without a BoW: a new batch takes the rows' results away, and computing row 0 gives row 3 none
    c.compute_bow(dv, [0, 3], [len(k), len(fr[3][0])], 1)
    c.fetch_bow(3)
    c.process(len(fr), True); c.area_grid(len(fr)); c.sync()
    for b in (0, 3):
        with pytest.raises(api.CmsError):
            c.fetch_bow(b)
    c.compute_bow(dv, [0], [len(k)], 1)
    c.fetch_bow(0)
    with pytest.raises(api.CmsError):
        c.fetch_bow(3)
    with pytest.raises(api.CmsError):
        st.search_by_bow_frames(c, [(0, 3, len(fr[3][0]), None)])
    with pytest.raises(api.CmsError):
        st.search_by_bow_frames(c, [(0, 0, len(k) - 1, None)])      # computed for another key-point count
    assert st.search_by_bow_frames(c, [(0, 0, len(k), None)])[0][1] >= 0
    # n > 16383, n beyond the row, a row named twice, a negative levelsup
    for rows, ns, lu in (([0], [16384], 1), ([0], [c.geom.kp_cap + 1], 1), ([0, 0], [5, 5], 1), ([0], [5], -1), ([len(fr)], [5], 1)):
        with pytest.raises(api.CmsError):
            c.compute_bow(dv, rows, ns, lu)
    with pytest.raises(api.CmsError):
        dv.transform(ctx, np.zeros((16384, 32), np.uint8), 1)
    # a malformed tree is refused before anything reaches the device
    t = vc.case_tree("k3_L2")
    bad = vc.with_weights(t, parent=np.where(np.arange(len(t["parent"])) == 2, 5, t["parent"]).astype(np.int32))
    with pytest.raises(api.CmsError) as e:
        api.Vocabulary.from_dict(bad)
    assert "parent" in str(e.value)
    st.close(); cg.close()


def test_vocabulary_on_another_device_is_rejected(ctx):
    if api.lib().cms_device_count() < 2:
        pytest.skip("needs two visible devices: a vocabulary can only be created on a device that exists")
    d = vc.case_descriptors("k10_L3", 65)
    other = api.Vocabulary.from_dict(vc.case_tree("k10_L3"), device=1)
    with pytest.raises(api.CmsError) as e:
        other.transform(ctx, d, 1)
    assert "another device" in str(e.value)
    _place(ctx, 0, d)
    with pytest.raises(api.CmsError):
        ctx.compute_bow(other, [0], [65], 1)
    other.close()


def test_refilled_slot_has_no_bowvector(extracted):
    """a slot's BowVector belongs to the key frame it was computed from: every put into the slot takes it away"""
    camd, c, fr = extracted
    dv, hv = _pair("k10_L3")
    cg = api.Context(camd, nfeatures=800, max_batch=1)
    st = api.KeyframeStore(cg, max_keyframes=2, max_features=1024, max_nodes=256)
    (k0, d0), (k1, d1) = fr[0], fr[1]
    st.put_from_frames(c, [(0, 0, len(k0), _kf(k0, d0, EMPTY_FV, 0))])
    st.compute_bow(dv, [0], 1)
    h0 = hv.transform(d0, 1)
    _same(h0, st.fetch_bow(0, feature_vector=True), "slot 0, first key frame")
    # another key frame into the same slot, from a frame row ...
    st.put_from_frames(c, [(0, 1, len(k1), _kf(k1, d1, EMPTY_FV, 1))])
    with pytest.raises(api.CmsError) as e:
        st.fetch_bow(0)
    assert "no BowVector" in str(e.value)
    st.compute_bow(dv, [0], 1)
    _same(hv.transform(d1, 1), st.fetch_bow(0, feature_vector=True), "slot 0, second key frame")
    # ... through the single-frame entry ...
    st.put_from_frame(0, c, 0, len(k0), _kf(k0, d0, EMPTY_FV, 0))
    with pytest.raises(api.CmsError):
        st.fetch_bow(0)
    st.compute_bow(dv, [0], 1)
    _same(h0, st.fetch_bow(0, feature_vector=True), "slot 0, first key frame again")
    # ... and from the host
    kf = dict(x=k1["x"], y=k1["y"], octave=k1["octave"], angle=k1["angle"], desc=d1, rays=np.zeros((len(k1), 3), np.float32), **_kf(k1, d1, EMPTY_FV, 1))
    K, keep = api.make_keyframe(kf)
    st.put(0, K)
    with pytest.raises(api.CmsError):
        st.fetch_bow(0)
    st.compute_bow(dv, [0], 1)
    _same(hv.transform(d1, 1), st.fetch_bow(0, feature_vector=True), "slot 0, key frame from the host")
    st.close(); cg.close()


def test_mirror_device_engine_equals_host_core():
    """ORBVocabulary::transform of the mirror with its default engine (the shared context's device) against engine HOST_CORE"""
    import ctypes as C
    H = hl.H()
    cam = api.make_camera(synth.camera("lafida", F))
    assert H.hm_set_camera(C.byref(cam)) == 0, H.hm_last_error()
    for name in ("k10_L3", "k17_L2", "tf_dot"):
        hv = hl.HostVocabulary(vc.case_tree(name))
        for n in (0, 65, 2000):
            d = vc.case_descriptors(name, n) if n in vc.CASES[name][1] else vc.descriptors(7, vc.case_tree(name), n)
            _same(hv.transform(d, 1, engine=hl.HOST_CORE), hv.transform(d, 1, engine=hl.DEVICE), (name, n, "mirror DEVICE"))
        hv.close()
