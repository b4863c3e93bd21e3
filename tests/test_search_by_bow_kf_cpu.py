"""ORBMatcher::SearchByBoW(KeyFrame*, KeyFrame*, ...) (src/ORBMatcher.cpp:541-674): the CPU restatement (tests/npref_bow_kf.py) against known answers
built by hand, the floor of matches on the seeded cases the GPU test compares, and the libraries' exports and ABI layout.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bow_kf_cases as cases
import npref_bow
from cubemapslam_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_NAME = {c["name"]: c for c in cases.HAND}


@pytest.mark.parametrize("c", cases.HAND, ids=[c["name"] for c in cases.HAND])
def test_hand_built_answers(c):
    idx2, n = cases.restate(c)
    assert list(idx2) == c["idx2"] and n == c["n"]


def test_feat_node_rule_only_changes_malformed_vectors():
    for c in cases.HAND:
        plain = cases.restate(c, feat_node=False)
        if c["name"].startswith("listed_twice") and c["name"] != "listed_twice_in_a_node_2":
            continue
        assert list(plain[0]) == c["idx2"] and plain[1] == c["n"], c["name"]
    # the reference as it stands on the malformed ones: a second listing matches again and counts again
    idx2, n = cases.restate(BY_NAME["listed_twice_across_nodes"], feat_node=False)
    assert list(idx2) == [1, 2, -1] and n == 3
    idx2, n = cases.restate(BY_NAME["listed_twice_in_a_node_1"], feat_node=False)
    assert list(idx2) == [1] and n == 2
    for kind in ("coarse", "many"):
        c = cases.seeded(kind, 0.75, True)
        plain, want = cases.restate(c, feat_node=False), cases.seeded_reference(kind, 0.75, True)
        assert np.array_equal(plain[0], want[0]) and plain[1] == want[1]


def _other_overload(c):
    """the (KeyFrame, Frame) overload's restatement on the same pair, key frame 2 as the frame: idx2 per key-frame-1 feature"""
    k1, k2 = c["kf1"], c["kf2"]
    kf_idx, n = npref_bow.search_by_bow(k1["angle"], k1["desc"], k1["mp"] >= 0, c["bad1"], k1, k2["angle"], k2["desc"], k2, len(k2["mp"]), c["nnratio"], c["ori"])
    idx2 = np.full(len(k1["mp"]), -1, np.int32)
    for i2, i1 in enumerate(kf_idx):
        if i1 >= 0:
            idx2[i1] = i2
    return list(idx2), n


def test_the_two_overloads_disagree():
    assert _other_overload(BY_NAME["dist_50_rejected"]) == ([0], 1)                 # <= TH_LOW there, < TH_LOW here
    assert _other_overload(BY_NAME["nearest_without_map_point"]) == ([0], 1)        # no filter on the frame side there
    assert _other_overload(BY_NAME["nearest_bad"]) == ([0], 1)
    assert _other_overload(BY_NAME["dist_49_accepted"]) == ([0], 1)                 # ... and agree where neither difference bears


@pytest.mark.parametrize("kind,nnratio,ori", cases.SEEDED)
def test_seeded_cases_have_matches(kind, nnratio, ori):
    idx2, n = cases.seeded_reference(kind, nnratio, ori)
    assert n >= 50 and n == int((idx2 >= 0).sum())


def test_seeded_cases_reach_the_paths_they_are_for():
    sizes = lambda k: np.diff(k["node_off"])
    _, k2, _, _ = cases.seeded_pair("coarse")
    assert sizes(k2).min() > 64                                     # the lane stride over key frame 2's features of a node wraps
    k1, k2, _, _ = cases.seeded_pair("fine")
    assert 64 < len(k1["node_id"]) <= 1024
    k1, k2, b1, b2 = cases.seeded_pair("many")
    assert 1024 < len(k1["node_id"]) <= 2048 and 1024 < len(k2["node_id"]) <= 2048      # the kernel's outer node loop runs twice
    for k, b in ((k1, b1), (k2, b2)):
        assert len(k["mp"]) <= 4096
        assert 0.3 < (k["mp"] < 0).mean() < 0.5 and 0.05 < b.mean() < 0.15
    # the orientation check removes something
    assert cases.seeded_reference("coarse", 0.75, True)[1] < cases.seeded_reference("coarse", 0.75, False)[1]


def test_libraries_export_the_keyframe_search():
    assert hasattr(api.lib(), "cms_kfstore_search_by_bow_keyframes")
    H = C.CDLL(os.path.join(ROOT, "cubemapslam_amd", "lib", "libcubemapslam_host.so"))
    assert hasattr(H, "hm_search_by_bow_keyframes")


def test_bow_kf_job_layout_matches_header(tmp_path):
    """api.BowKfJob against cms_bow_kf_job as the C compiler lays it out from include/cubemapslam_hip.h (sizeof / offsetof of a probe program)"""
    fields = ("slot1", "n1", "slot2", "n2", "skip1", "skip2")
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cubemapslam_hip.h"\nint main(void) {\n  printf("%zu", sizeof(cms_bow_kf_job));\n' +
                   "".join('  printf(" %%zu", offsetof(cms_bow_kf_job, %s));\n' % f for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(api.BowKfJob)
    assert got[1:] == [getattr(api.BowKfJob, f).offset for f in fields]
