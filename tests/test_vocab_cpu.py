"""ComputeBoW without a GPU: the host build of csrc/cms_vocab_core.h (the definition of record the device entries are held to) against the literal
numpy restatement tests/npref_vocab.py on every case of tests/vocab_cases.py -- equal exactly, ids as integers and values as float64 bits --, the text
format (save -> load -> save, trailing newline, malformed files), the mirror's ORBVocabulary (ComputeBoW's guards, score), and the loader and the core
as a stand-alone program under AddressSanitizer + UBSan."""
import os
import subprocess

import numpy as np
import pytest

import npref_vocab as ref
import vocab_cases as vc
import vocab_hostlib as hl

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _host(name):
    return hl.HostVocabulary(vc.case_tree(name))


@pytest.mark.parametrize("name", sorted(vc.CASES))
def test_host_core_equals_restatement(name):
    tr = ref.Tree(vc.case_tree(name))
    hv = _host(name)
    _, ns, levelsups = vc.CASES[name]
    for n in ns:
        d = vc.case_descriptors(name, n)
        for lu in levelsups:
            want = ref.transform(tr, d, lu)
            got = hv.transform(d, lu)
            assert ref.first_difference(want, got) is None, (name, n, lu, ref.first_difference(want, got))
            assert n < 64 or name == "all_stopped" or len(want["word_id"]) > 0


def test_descent_feature_by_feature():
    name = "unbalanced"
    t = vc.case_tree(name)
    tr = ref.Tree(t)
    hv = _host(name)
    d = vc.case_descriptors(name, 257)
    for lu in (0, 1, 2, 3, 4):
        word, nid, w = hv.descend(d, lu)
        want = [ref.descend(tr, f, lu) for f in d]
        assert [int(x) for x in word] == [a for a, _, _ in want] and [int(x) for x in nid] == [c for _, _, c in want]
        assert np.array_equal(w.view(np.uint64), np.array([b for _, b, _ in want], np.float64).view(np.uint64))
    # some descents end on a level-1 leaf (above the nid level of levelsup 1) and report that leaf, some go on to level 3
    word, nid, _ = hv.descend(d, 1)
    level1_leaves = set(int(i) for i in np.flatnonzero((t["parent"] == 0) & (t["is_leaf"] != 0)) if i > 0)
    assert 0 < sum(int(x) in level1_leaves for x in nid) < len(nid)
    # L - levelsup <= 0: the root
    assert set(int(x) for x in hv.descend(d, 3)[1]) == {0} and set(int(x) for x in hv.descend(d, 4)[1]) == {0}


def test_tie_goes_to_the_first_child():
    t = vc.case_tree("ties")
    d = vc.case_descriptors("ties", 257)
    word, _, _ = _host("ties").descend(d, 1)
    # the last child of every family repeats the first one's descriptor: no descent may ever pick a last child
    n = len(t["parent"])
    last_child = {}
    for i in range(1, n):
        last_child[int(t["parent"][i])] = i      # ascending ids: the last one seen is the last child
    last_leaves = [i for i in last_child.values() if t["is_leaf"][i]]
    assert last_leaves
    wid = vc.word_ids(t)
    assert not set(int(w) for w in word) & set(int(wid[i]) for i in last_leaves)
    # ... although descriptors were drawn AT such leaves
    lv_desc = {bytes(t["desc"][i]) for i in last_leaves}
    assert any(bytes(f) in lv_desc for f in d)


def test_zero_weight_words_enter_neither_vector():
    t = vc.case_tree("k10_L3")
    hv = _host("k10_L3")
    d = vc.case_descriptors("k10_L3", 2000)
    word, _, w = hv.descend(d, 1)
    r = hv.transform(d, 1)
    stopped = w <= 0
    assert stopped.any() and (w < 0).any() and (w == 0).any()
    assert sorted(set(int(x) for x in word[~stopped])) == [int(x) for x in r["word_id"]]
    assert sorted(int(x) for x in r["node_feat"]) == [int(i) for i in np.flatnonzero(~stopped)]
    # ... and when every word is stopped both vectors are empty
    tr = ref.Tree(vc.case_tree("all_stopped"))
    got = _host("all_stopped").transform(d[:257], 1)
    assert ref.first_difference(ref.transform(tr, d[:257], 1), got) is None
    assert len(got["word_id"]) == 0 and len(got["node_id"]) == 0 and list(got["node_off"]) == [0]


def test_repeated_descriptor():
    d = vc.repeated_descriptor()
    for name, weighting in (("k10_L3", vc.TF_IDF),):
        t = vc.case_tree(name)
        for scoring in (vc.L1_NORM, vc.DOT_PRODUCT):
            tt = vc.with_weights(t, scoring=scoring, weighting=weighting)
            hv = hl.HostVocabulary(tt)
            got = hv.transform(d, 1)
            assert ref.first_difference(ref.transform(ref.Tree(tt), d, 1), got) is None
            assert len(got["word_id"]) == 1 and len(got["node_id"]) == 1 and list(got["node_feat"]) == list(range(300))
            if scoring == vc.DOT_PRODUCT:
                # w added to itself 299 times, then divided by v.size() = 1: not 300 * w
                w = float(hv.descend(d[:1], 1)[2][0])
                acc = w
                for _ in range(299):
                    acc += w
                assert got["word_val"][0] == acc


def test_full_size_tree():
    """ORBvoc.txt's shape: 1.1 M nodes, ids beyond 2^20"""
    t = vc.case_tree("full_size")
    assert len(t["parent"]) == 1111111
    d = vc.case_descriptors("full_size", 300)
    got = hl.HostVocabulary(t).transform(d, 4)
    assert ref.first_difference(ref.transform(ref.Tree(t), d, 4), got) is None
    assert got["word_id"].max() > 500000 and len(got["node_id"]) > 50


# ---- text format
def test_text_save_load_save(tmp_path):
    t = vc.case_tree("unbalanced")
    a, b = tmp_path / "a.txt", tmp_path / "b.txt"
    hl.HostVocabulary(t).save(a)
    ta = a.read_bytes()
    assert ta == vc.text(t).encode()      # the reference's bytes: "k L  s w", "parent leaf d0 .. d31  weight" with 6 significant digits
    hv = hl.HostVocabulary(path=a)
    hv.save(b)
    assert b.read_bytes() == ta
    u = hv.tree()
    assert u["k"] == t["k"] and u["L"] == t["L"] and np.array_equal(u["parent"], t["parent"]) and np.array_equal(u["is_leaf"], t["is_leaf"])
    assert np.array_equal(u["desc"], t["desc"]) and np.array_equal(u["weight"][1:], np.array([float("%g" % w) for w in t["weight"][1:]]))
    assert u["words"] == int(t["is_leaf"].sum())


def test_text_trailing_newline(tmp_path):
    t = vc.case_tree("k3_L2")
    txt = vc.text(t)
    trees = []
    for i, s in enumerate((txt, txt[:-1], txt + "\n", txt + "\n\n")):
        f = tmp_path / ("v%d.txt" % i)
        f.write_text(s)
        trees.append(hl.HostVocabulary(path=f).tree())
    for u in trees[1:]:
        assert all(np.array_equal(u[key], trees[0][key]) for key in ("parent", "is_leaf", "desc", "weight")) and u["words"] == trees[0]["words"]


D32 = " " + " ".join(str(i) for i in range(32)) + "  "
MALFORMED = {
    "k out of range": "21 3  0 0\n0 1" + D32 + "1\n",
    "L out of range": "2 11  0 0\n0 1" + D32 + "1\n",
    "scoring out of range": "2 3  6 0\n0 1" + D32 + "1\n",
    "weighting out of range": "2 3  0 4\n0 1" + D32 + "1\n",
    "inner node without children": "2 2  0 0\n0 0" + D32 + "1\n0 1" + D32 + "1\n",
    "leaf with children": "2 2  0 0\n0 1" + D32 + "1\n1 1" + D32 + "1\n",
    "parent id not smaller": "2 2  0 0\n1 1" + D32 + "1\n",
    "more than k children": "2 2  0 0\n" + ("0 1" + D32 + "1\n") * 3,
}


@pytest.mark.parametrize("what", sorted(MALFORMED))
def test_text_malformed_is_refused(what, tmp_path):
    f = tmp_path / "bad.txt"
    f.write_text(MALFORMED[what])
    with pytest.raises(hl.VocabError) as e:
        hl.HostVocabulary(path=f)
    assert "vocabulary" in str(e.value)
    # the well-formed neighbour loads
    f.write_text("2 2  0 0\n0 1" + D32 + "1\n0 1" + D32 + "0.5\n")
    assert hl.HostVocabulary(path=f).tree()["words"] == 2


# ---- mirror class
def test_mirror_transform_equals_core():
    for name in ("k10_L3", "tf_dot", "tf_idf_l2"):
        hv = _host(name)
        d = vc.case_descriptors(name, 257)
        assert ref.first_difference(ref.transform(ref.Tree(vc.case_tree(name)), d, 4), hv.transform(d, 4, engine=hl.HOST_CORE)) is None


def test_compute_bow_guards():
    hv = _host("k10_L3")
    d = vc.case_descriptors("k10_L3", 257)
    want = hv.transform(d, 4)
    nw, nn = len(want["word_id"]), len(want["node_id"])
    # Frame::ComputeBoW: only when mBowVec is empty
    assert hv.compute_bow_guard(False, d, pre_bow=False, pre_fv=False) == (True, nw, nn)
    assert hv.compute_bow_guard(False, d, pre_bow=False, pre_fv=True) == (True, nw, nn)
    assert hv.compute_bow_guard(False, d, pre_bow=True, pre_fv=False) == (False, 1, 0)
    # KeyFrame::ComputeBoW: when mBowVec or mFeatVec is empty
    assert hv.compute_bow_guard(True, d, pre_bow=False, pre_fv=False) == (True, nw, nn)
    assert hv.compute_bow_guard(True, d, pre_bow=True, pre_fv=False) == (True, nw, nn)
    assert hv.compute_bow_guard(True, d, pre_bow=False, pre_fv=True) == (True, nw, nn)
    assert hv.compute_bow_guard(True, d, pre_bow=True, pre_fv=True) == (False, 1, 1)


def test_score_l1():
    hv = _host("k10_L3")
    a = (np.array([1, 4, 9], np.int32), np.array([0.5, 0.25, 0.25]))
    b = (np.array([2, 4, 9, 11], np.int32), np.array([0.25, 0.25, 0.125, 0.375]))
    # by hand: common words 4 and 9: (|0.25 - 0.25| - 0.25 - 0.25) + (|0.25 - 0.125| - 0.25 - 0.125) = -0.5 - 0.25 = -0.75 -> 0.375
    assert hv.score(a, b) == 0.375 and hv.score(b, a) == 0.375
    assert hv.score(a, a) == 1.0
    assert hv.score(a, (np.array([0, 2, 3], np.int32), np.array([0.5, 0.25, 0.25]))) == 0.0
    assert hv.score(a, (np.zeros(0, np.int32), np.zeros(0))) == 0.0
    d1, d2 = vc.case_descriptors("k10_L3", 257), vc.case_descriptors("k10_L3", 2000)
    v1, v2 = hv.transform(d1, 4), hv.transform(d2, 4)
    p1, p2 = (v1["word_id"], v1["word_val"]), (v2["word_id"], v2["word_val"])
    assert hv.score(p1, p2) == ref.score_l1(p1, p2) and 0.0 < hv.score(p1, p2) < 1.0
    assert abs(hv.score(p1, p1) - 1.0) < 1e-12
    with pytest.raises(hl.VocabError):
        _host("tf_idf_l2").score(a, b)


# ---- the loader and the core under the sanitizers, as a program of their own
def test_vocab_core_emulation_sanitized(tmp_path):
    exe = str(tmp_path / "vocab_core_emu")
    host = os.path.join(ROOT, "cubemapslam_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"), "-I", host, os.path.join(HERE, "emu", "vocab_core_emu.cpp"),
                           os.path.join(host, "io_formats.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "vocab_core_emu: ok" in r.stdout and "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]
