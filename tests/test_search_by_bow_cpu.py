"""ORBMatcher::SearchByBoW(KeyFrame*, Frame&, ...) (src/ORBMatcher.cpp:409-539): known answers for the CPU restatement (tests/npref_bow.py), built by
hand, and the library's exports and ABI layout.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np

import npref_bow
from cubemapslam_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def desc_at(dist, seed=0):
    """a descriptor at Hamming distance `dist` from the all-zero one (the first `dist` bits set, rotated by seed)"""
    bits = np.zeros(256, np.uint8)
    bits[(np.arange(dist) + seed) % 256] = 1
    return np.packbits(bits)


def case(kf_rows, f_rows, kf_fv, f_fv, kf_angle=None, f_angle=None, has_mp=None, bad=None, nnratio=0.7, ori=False):
    """kf_rows / f_rows: distance of each feature's descriptor from zero (key-frame descriptors are all zero-distance references: each key-frame
    feature is the zero descriptor, so a frame feature's distance to any key-frame feature is its row value)"""
    kd = np.zeros((len(kf_rows), 32), np.uint8)
    fd = np.stack([desc_at(d, 7 * i) for i, d in enumerate(f_rows)]) if len(f_rows) else np.zeros((0, 32), np.uint8)
    ka = np.zeros(len(kf_rows), np.float32) if kf_angle is None else np.asarray(kf_angle, np.float32)
    fa = np.zeros(len(f_rows), np.float32) if f_angle is None else np.asarray(f_angle, np.float32)
    mp = np.ones(len(kf_rows), bool) if has_mp is None else np.asarray(has_mp, bool)
    return npref_bow.search_by_bow(ka, kd, mp, bad, kf_fv, fa, fd, f_fv, len(f_rows), nnratio, ori)


def fv(nodes):
    """{node id: [features]} -> CSR"""
    ids = sorted(nodes)
    off = np.concatenate([[0], np.cumsum([len(nodes[i]) for i in ids])]).astype(np.int32)
    feat = np.array([f for i in ids for f in nodes[i]], np.int32)
    return np.array(ids, np.int32), off, feat


def test_tie_at_best_gives_no_match():
    m, n = case([0], [20, 20], fv({5: [0]}), fv({5: [0, 1]}))
    assert n == 0 and list(m) == [-1, -1]
    m, n = case([0], [20, 30], fv({5: [0]}), fv({5: [0, 1]}))      # 20 < 0.7 * 30
    assert n == 1 and list(m) == [0, -1]


def test_taken_frame_feature_is_skipped_in_the_node_only():
    # node 5: key-frame features 0 and 1 both prefer frame feature 0 (10); the second gets frame feature 1 (30, alone: 30 < 0.7 * 256)
    m, n = case([0, 0, 0], [10, 30, 10], fv({5: [0, 1], 9: [2]}), fv({5: [0, 1], 9: [2]}))
    assert n == 3 and list(m) == [0, 1, 2]
    # (without the skip the second key-frame feature would take frame feature 0 again and the result would be [1, -1, 2]); node 9's frame feature 2,
    # as close as frame feature 0, is matched all the same: a taken feature of node 5 does not reach into node 9


def test_th_low_boundary():
    m, n = case([0], [50], fv({1: [0]}), fv({1: [0]}))
    assert n == 1 and list(m) == [0]
    m, n = case([0], [51], fv({1: [0]}), fv({1: [0]}))
    assert n == 0 and list(m) == [-1]


def test_ratio_boundary_is_strict_in_float():
    assert np.float32(0.7) * np.float32(50) == np.float32(35.0)
    m, n = case([0], [35, 50], fv({1: [0]}), fv({1: [0, 1]}), nnratio=0.7)
    assert n == 0
    m, n = case([0], [34, 50], fv({1: [0]}), fv({1: [0, 1]}), nnratio=0.7)
    assert n == 1 and list(m) == [0, -1]


def test_rotation_bin_30_wraps_to_0():
    # rot = 359.9 -> 359.9 / 12 = 29.99 -> round 30 -> bin 0; with bin 0 the largest bin it survives the filter together with a rot = 0 match
    m, n = case([0, 0, 0], [10, 10, 10], fv({1: [0], 2: [1], 3: [2]}), fv({1: [0], 2: [1], 3: [2]}), kf_angle=[359.9, 0.0, 100.0],
                f_angle=[0.0, 0.0, 0.0], ori=True)
    # bins: 0, 0, 8 -> max1 = bin 0 (2), max2 = bin 8 (1) >= 0.1 * 2: all kept
    assert n == 3 and list(m) == [0, 1, 2]


def test_three_maxima_drops_small_bins():
    # 11 matches in bin 0, one in bin 10: 1 < 0.1 * 11 -> bin 10 dropped
    k = 12
    nodes = {i: [i] for i in range(k)}
    ang = [0.0] * 11 + [120.0]
    m, n = case([0] * k, [10] * k, fv(nodes), fv(nodes), kf_angle=ang, f_angle=[0.0] * k, ori=True)
    assert n == 11 and m[11] == -1 and (m[:11] >= 0).all()
    # 10 in bin 0 and 1 in bin 10: 1 < 0.1 * 10 is false -> kept; a third bin of 1 is kept too
    ang = [0.0] * 10 + [120.0, 240.0]
    m, n = case([0] * k, [10] * k, fv(nodes), fv(nodes), kf_angle=ang, f_angle=[0.0] * k, ori=True)
    assert n == 12
    # four bins: the fourth never survives
    ang = [0.0] * 9 + [120.0, 240.0, 300.0]
    m, n = case([0] * k, [10] * k, fv(nodes), fv(nodes), kf_angle=ang, f_angle=[0.0] * k, ori=True)
    assert n == 11 and m[11] == -1
    assert npref_bow.compute_three_maxima([11, 1] + [0] * 28) == (0, -1, -1)
    assert npref_bow.compute_three_maxima([10, 1, 0, 0] + [0] * 26) == (0, 1, -1)


def test_node_on_one_side_only_contributes_nothing():
    m, n = case([0, 0], [10, 10], fv({1: [0], 4: [1]}), fv({2: [0], 4: [1]}))
    assert n == 1 and list(m) == [-1, 1]
    m, n = case([0], [10], fv({3: [0]}), fv({}))
    assert n == 0


def test_orientation_off_filters_nothing():
    k = 12
    nodes = {i: [i] for i in range(k)}
    ang = [0.0] * 11 + [120.0]
    m, n = case([0] * k, [10] * k, fv(nodes), fv(nodes), kf_angle=ang, f_angle=[0.0] * k, ori=False)
    assert n == 12 and (m >= 0).all()


def test_bad_map_points_are_skipped():
    m, n = case([0, 0], [10, 30], fv({5: [0, 1]}), fv({5: [0, 1]}), bad=np.array([1, 0], np.uint8))
    assert n == 1 and list(m) == [1, -1]


def test_library_exports_search_by_bow():
    L = C.CDLL(os.path.join(ROOT, "cubemapslam_amd", "lib", "libcubemapslam_hip.so"))
    assert hasattr(L, "cms_search_by_bow") and hasattr(L, "cms_kfstore_search_by_bow")
    H = C.CDLL(os.path.join(ROOT, "cubemapslam_amd", "lib", "libcubemapslam_host.so"))
    assert hasattr(H, "hm_search_by_bow")


def test_bow_job_layout_matches_header(tmp_path):
    """api.BowJob against cms_bow_job as the C compiler lays it out from include/cubemapslam_hip.h (sizeof / offsetof of a probe program)"""
    fields = ("slot", "b", "n", "nnodes", "node_id", "node_off", "node_feat", "kf_skip")
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cubemapslam_hip.h"\nint main(void) {\n  printf("%zu", sizeof(cms_bow_job));\n' +
                   "".join('  printf(" %%zu", offsetof(cms_bow_job, %s));\n' % f for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(api.BowJob)
    assert got[1:] == [getattr(api.BowJob, f).offset for f in fields]
