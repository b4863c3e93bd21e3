"""KeyFrameDatabase on the device (cms_kfstore_set_bow, cms_kfdb_add / erase / clear / set_covisibles / detect, cms_kfstore_bow_score) against the host
build of csrc/cms_kfdb_core.h (hm_kfdb_*), which tests/test_kfdb_cpu.py holds against a literal restatement of the reference.  Every comparison is
exact: candidate lists as lists, common-word counts as ints, scores as float32 / float64 bits.  The cases are tests/kfdb_cases.py's: a store of 160
slots with max_features 256, BowVectors set from the host so that no vocabulary stands in the way -- except in the query-form test, which runs
cms_frames_compute_bow once."""
import ctypes as C

import numpy as np
import pytest

import kfdb_cases as kc
import kfdb_hostlib as hl
import vocab_cases as vc
import vocab_hostlib
from cubemapslam_amd import api, synth

pytestmark = pytest.mark.gpu

KP = api.KP_DTYPE
F = 150


DeviceBackend = hl.DeviceBackend


class HostBackend:
    def __init__(self):
        self.db = hl.HostDatabase(kc.K, kc.MAXF)
        self.detect = self.db.detect

    def __getattr__(self, op):
        def call(*a):
            assert getattr(self.db, op)(*a) == 0, op
        return call


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(synth.camera("lafida", F), nfeatures=1000, max_batch=2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev(ctx):
    cg = api.Context(synth.camera("lafida", F), nfeatures=500, max_batch=1)      # the mapping side's context: the store's stream is not the frame thread's
    st = api.KeyframeStore(cg, max_keyframes=kc.K, max_features=kc.MAXF, max_nodes=8)
    b = DeviceBackend(st, ctx)
    for s in range(kc.K):
        b.refill(s)
    yield b
    st.close(); cg.close()


_host = {}


def host_expected(name):
    """the host core's results of a case, computed once"""
    if name not in _host:
        h = HostBackend()
        _host[name] = kc.run(kc.case_ops(name), h)
        h.db.close()
    return _host[name]


@pytest.mark.parametrize("name", kc.NAMES)
def test_device_equals_host_core(dev, name):
    want = host_expected(name)
    dev.reset()
    got = kc.run(kc.case_ops(name), dev)
    assert kc.first_difference(want, got) is None, kc.first_difference(want, got)
    assert kc.first_difference(kc.expected(name), got) is None      # ... and so the restatement of the reference


def test_stale_score_one_call_equals_two_calls(dev):
    res = {}
    for name in ("stale_one_call", "stale_two_calls", "stale_readd"):
        dev.reset()
        res[name] = kc.run(kc.case_ops(name), dev)
    one, two, readd = res["stale_one_call"][0][1], res["stale_two_calls"][1][0], res["stale_readd"][1][0]
    assert one[0] == two[0] == [0] and np.array_equal(one[1], two[1]) and np.array_equal(one[2], two[2])
    assert readd[0] == [1]      # what a zeroed score gives


def test_query_forms(dev, ctx):
    """a frame row's resident BowVector (cms_frames_compute_bow), the same vector in a store slot and as explicit words give the same answer"""
    tree = vc.case_tree("k10_L3")
    voc = api.Vocabulary.from_dict(tree)
    hv = vocab_hostlib.HostVocabulary(tree)
    dev.reset()
    host = HostBackend()
    slots = list(range(10, 40))
    for s in slots:
        bow = hv.transform(vc.descriptors(100 + s, tree, 150), 1)
        dev.set_bow(s, bow["word_id"], bow["word_val"]); host.set_bow(s, bow["word_id"], bow["word_val"])
    d = vc.descriptors(7, tree, 200)
    k = np.zeros(len(d), KP)
    k["x"] = 10 + np.arange(len(d)) % 400; k["y"] = 10 + np.arange(len(d)) // 400
    ctx.area_set_keypoints(1, k); ctx.area_set_descriptors(1, d)
    ctx.compute_bow(voc, [1], [len(d)], 1)
    q = ctx.fetch_bow(1)
    assert len(q["word_id"]) > 50
    dev.set_bow(5, q["word_id"], q["word_val"]); host.set_bow(5, q["word_id"], q["word_val"])
    for b in (dev, host):
        b.add(slots, [0] * len(slots))
        for i, s in enumerate(slots):
            b.covis(s, kc.pad10(slots[(i + j) % len(slots)] for j in (1, 2, 5)))
    forms = {"row": ("row", 1), "slot": ("slot", 5), "words": kc.words(q["word_id"], q["word_val"])}
    want = host.detect([kc.job(kc.RELOC, forms["words"]), kc.job(kc.LOOP, forms["words"], min_score=0.01, connected=[12, 13])])
    assert len(want[0][0]) > 0 and want[0][1].max() > 5
    for name, form in forms.items():
        got = dev.detect([kc.job(kc.RELOC, form), kc.job(kc.LOOP, form, min_score=0.01, connected=[12, 13])])
        assert kc.first_difference([want], [got]) is None, (name, kc.first_difference([want], [got]))
    # a row without a computed BoW is refused
    with pytest.raises(api.CmsError) as e:
        dev.detect([kc.job(kc.RELOC, ("row", 0))])
    assert "no BoW computed" in str(e.value)
    host.db.close(); voc.close(); hv.close()


def test_bow_score(dev):
    rng = np.random.default_rng(3)
    dev.reset()
    host = HostBackend()
    voc = vocab_hostlib.HostVocabulary(vc.case_tree("k10_L3"))
    bows = [kc.random_bow(rng, n, 300) for n in (1, 63, 64, 65, 200, 130)]
    bows.append((bows[0][0] + 5000, bows[0][1]))      # no word in common with any other
    bows.append((np.zeros(0, np.int32), np.zeros(0)))
    for s, (ids, v) in enumerate(bows):
        dev.set_bow(s, ids, v); host.set_bow(s, ids, v)
    a, b = np.meshgrid(np.arange(len(bows)), np.arange(len(bows)))
    a, b = a.ravel(), b.ravel()
    got = dev.st.bow_score(a, b)
    assert np.array_equal(got.view(np.uint64), host.db.bow_score(a, b).view(np.uint64))
    mirror = np.array([voc.score(bows[i], bows[j]) for i, j in zip(a, b)])
    assert np.array_equal(got.view(np.uint64), mirror.view(np.uint64))
    assert got[(a == 6) & (b == 4)][0] == 0.0 and got[(a == 4) & (b == 4)][0] > 0.99
    dev.refill(100)
    with pytest.raises(api.CmsError):
        dev.st.bow_score([100], [0])
    host.db.close(); voc.close()


def test_error_paths(dev):
    st = dev.st
    dev.reset()
    ids, v = np.arange(4, dtype=np.int32), np.full(4, 0.25)
    dev.refill(0); dev.refill(1)
    with pytest.raises(api.CmsError) as e:
        st.db_add([0], [0])
    assert "no BowVector" in str(e.value)
    for bad in ([3, 2, 5], [2, 2, 4], [-1, 2, 4]):
        with pytest.raises(api.CmsError) as e:
            st.set_bow(0, bad, [0.1, 0.2, 0.7])
        assert "ascending" in str(e.value)
    with pytest.raises(api.CmsError):
        st.set_bow(0, np.arange(kc.MAXF + 1), np.ones(kc.MAXF + 1))
    with pytest.raises(api.CmsError):
        st.db_add([0], [0])      # the refused calls left the slot without a BowVector
    st.set_bow(0, ids, v); st.set_bow(1, ids, v)
    with pytest.raises(api.CmsError):
        st.db_add([1, 0, 1], [0, 0, 0])
    st.db_add([0, 1], [0, 0])
    with pytest.raises(api.CmsError) as e:
        st.db_add([0], [0])
    assert "already" in str(e.value)
    with pytest.raises(api.CmsError):
        st.set_bow(0, ids, v)      # in the database
    j = [kc.job(kc.RELOC, kc.words(ids, v))]
    assert dev.detect(j)[0][0] == [0, 1]
    with pytest.raises(api.CmsError) as e:
        st.detect_candidates(dev.ctx, j, cand_cap=1)
    assert "cand_cap" in str(e.value) and st.last_n_cand[0] == 2      # n_cand is delivered with the overflow
    with pytest.raises(api.CmsError):
        dev.detect([kc.job(kc.RELOC, kc.words([4, 3], [0.5, 0.5]))])
    dev.refill(2)
    with pytest.raises(api.CmsError):
        dev.detect([kc.job(kc.LOOP, ("slot", 2))])      # no BowVector in the query slot
    dev.refill(0)                                       # a refilled slot has left the database
    assert dev.detect(j)[0][0] == [1]
    st.db_erase([0, 5])                                 # not in it: left alone
    assert dev.detect(j)[0][0] == [1]
    assert dev.detect([]) == []


def test_store_on_another_device_is_rejected(dev):
    if api.lib().cms_device_count() < 2:
        pytest.skip("needs two visible devices: a frame context can only be created on a device that exists")
    other = api.Context(synth.camera("lafida", F), nfeatures=500, max_batch=1, device=1)
    with pytest.raises(api.CmsError) as e:
        dev.st.detect_candidates(other, [kc.job(kc.RELOC, kc.words([1], [1.0]))])
    assert "share the device" in str(e.value)
    other.close()


def test_handle_reuse_stage_grows(dev):
    """a small call, then a larger one on the same store (more entries, more jobs, longer queries), then the small one again"""
    small, large = "one_entry", "random_9"
    for name in (small, large, small, "stride_130"):
        dev.reset()
        got = kc.run(kc.case_ops(name), dev)
        assert kc.first_difference(host_expected(name), got) is None, (name, kc.first_difference(host_expected(name), got))


def test_mirror_device_engine_equals_host_core():
    """ORB_SLAM2::KeyFrameDatabase of the mirror: its device engine (a store on the shared context) against its host engine, one relocalisation and
    one loop query"""
    H = vocab_hostlib.H()
    cam = api.make_camera(synth.camera("lafida", F))
    assert H.hm_set_camera(C.byref(cam)) == 0, H.hm_last_error()
    tree = vc.case_tree("k10_L3")
    hv = vocab_hostlib.HostVocabulary(tree)
    n_kf = 24
    descs = [vc.descriptors(300 + i, tree, 120) for i in range(n_kf)]
    q = vc.descriptors(305, tree, 120).copy()
    q[:40] = vc.descriptors(999, tree, 40)
    covis = np.array([kc.pad10((i + j) % n_kf for j in (1, 3)) for i in range(n_kf)], np.int32)
    out = {}
    for engine in (vocab_hostlib.HOST_CORE, vocab_hostlib.DEVICE):
        out[engine] = hl.mirror_detect(hv, engine, descs, covis, q, loop_query=4, min_score=0.02, connected=[5, 6])
    assert out[vocab_hostlib.HOST_CORE] == out[vocab_hostlib.DEVICE]
    assert len(out[vocab_hostlib.DEVICE][0]) > 0 and len(out[vocab_hostlib.DEVICE][1]) > 0
    hv.close()
