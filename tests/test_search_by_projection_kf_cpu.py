"""ORBMatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) (src/ORBMatcher.cpp:253-378): the CPU restatement
(tests/npref_reloc.py) against answers worked out by hand and, stage by stage, against the oracle; what the synthetic inputs of the GPU tests
exercise; the library's exports and the ABI layout of the job record.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import npref_reloc
import orc
import reloc_cases
from cubemapslam_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = reloc_cases.hand_cases()


@pytest.mark.parametrize("name,case,match,n,kp_mp", HAND, ids=[h[0] for h in HAND])
def test_hand_built_known_answers(name, case, match, n, kp_mp):
    m, nm, km = reloc_cases.run(case)
    assert list(m) == match and nm == n and list(km) == kp_mp, (name, list(m), nm, list(km))


def test_hand_built_cases_cover_the_list():
    names = " | ".join(h[0] for h in HAND)
    for word in ("ORBdist is accepted", "+ 1 is not", "tie", "taken by the entry before", "on entry", "levels", "cosFovTh", "lower bound", "upper bound", "minority",
                 "check off", "bin 30"):
        assert word in names, word
    info = {}
    reloc_cases.run([h for h in HAND if h[0] == "zc below cosFovTh"][0][1], info)
    assert list(info["proj"]["drop"]) == [npref_reloc.DROP_FOV, npref_reloc.DROP_NONE]
    for nm in ("dist3D below the lower bound", "dist3D above the upper bound"):
        reloc_cases.run([h for h in HAND if h[0] == nm][0][1], info)
        assert list(info["proj"]["drop"]) == [npref_reloc.DROP_DIST]
    reloc_cases.run([h for h in HAND if h[0] == "levels L-1 .. L+1"][0][1], info)
    assert list(info["proj"]["level"]) == [4] * 4


def test_rot_bin_and_three_maxima():
    assert npref_reloc.rot_bin(359.9, 0.0) == 0 and npref_reloc.rot_bin(354.0, 0.0) == 0 and npref_reloc.rot_bin(353.9, 0.0) == 29
    assert npref_reloc.rot_bin(10.0, 20.0) == 29 and npref_reloc.rot_bin(6.0, 0.0) == 1 and npref_reloc.rot_bin(5.9, 0.0) == 0      # round half away from zero
    assert npref_reloc.compute_three_maxima([11, 1] + [0] * 28) == (0, -1, -1)
    assert npref_reloc.compute_three_maxima([10, 1, 0, 0] + [0] * 26) == (0, 1, -1)
    assert npref_reloc.compute_three_maxima([2, 0, 2, 0, 2, 0, 2] + [0] * 23) == (0, 2, 4)


def test_descriptor_distance_table_equals_oracle():
    rng = np.random.default_rng(1)
    d = rng.integers(0, 256, (64, 32), dtype=np.uint8)
    for i in range(0, 64, 2):
        assert int(npref_reloc._POP[np.bitwise_xor(d[i], d[i + 1])].sum()) == orc.descriptor_distance(d[i], d[i + 1])


def test_scale_factors_are_the_extractors():
    sf = npref_reloc.scale_factors(1.2, 8)
    assert sf[1] == np.float32(1.2) and sf[3] == np.float32(np.float32(np.float32(1.2) * np.float32(1.2)) * np.float32(1.2))


@pytest.fixture(scope="module")
def kf_input():
    return reloc_cases.keyframe_input(seed=31)


def test_projection_stage_equals_oracle(kf_input):
    """(b): for every listed point that passes the cosFovTh test, u, v and the predicted level equal Frame::isInFrustum's of the oracle on the same pose
    (viewing-cosine limit below any cosine; it shares projection, bounds and PredictScale) -- bit for bit, over a few thousand random points"""
    inp, kf, kf_feat = kf_input
    F = inp["camd"]["face"]
    cam = orc.make_camera(inp["camd"])
    rng = np.random.default_rng(77)
    X = rng.normal(0, 1, (3000, 3)); X *= (rng.uniform(0.5, 9.0, 3000) / np.linalg.norm(X, axis=1))[:, None]
    pos = np.concatenate([inp["pos"], X.astype(np.float32)])
    total = 0
    poses = [inp["pose12"], reloc_cases.perturbed(inp["pose12"], rng), reloc_cases.perturbed(inp["pose12"], rng, 30.0, 50.0)]
    for pose12 in poses:
        Ow = npref_reloc.camera_centre(pose12)
        dist = np.linalg.norm(pos.astype(np.float64) - Ow.astype(np.float64), axis=1)
        mn, mx = reloc_cases.distance_members(dist, rng.uniform(-1.0, 9.0, len(pos)), rng, outside=0.15)
        pr = npref_reloc.project(F, npref_reloc.cos_fov_th(inp["camd"]), pose12, pos, mn, mx, 1.2, 8)
        pose15 = np.concatenate([pose12, Ow]).astype(np.float32)
        nrm = np.zeros_like(pos); nrm[:, 2] = 1
        fr = orc.is_in_frustum(cam, pose15, pos, nrm, mn, mx, viewing_cos_limit=-2.0, scale_factor=1.2, nlevels=8)
        ok = pr["drop"] != npref_reloc.DROP_FOV
        live = pr["drop"][ok] == 0
        assert np.array_equal(fr["in_view"][ok] != 0, live)
        sel = np.flatnonzero(ok)[live]
        assert np.array_equal(fr["proj_x"][sel].view(np.uint32), pr["u"][sel].view(np.uint32))
        assert np.array_equal(fr["proj_y"][sel].view(np.uint32), pr["v"][sel].view(np.uint32))
        assert np.array_equal(fr["level"][sel], pr["level"][sel])
        assert set(np.unique(pr["level"][sel])) == set(range(8)) and (pr["drop"] == npref_reloc.DROP_DIST).sum() > 100
        total += len(sel)
    assert total > 2000, total


def test_camera_centre_is_the_frame_members():
    """Ow as :259 derives it: the double-accumulated -Rcw.t()*tcw; for an exactly representable pose it is the exact value"""
    p = np.array([0, -1, 0, 1, 0, 0, 0, 0, 1, 0.5, -2.0, 4.0], np.float32)
    assert np.array_equal(npref_reloc.camera_centre(p), np.array([2.0, 0.5, -4.0], np.float32))


def test_synthetic_input_exercises_what_it_is_for(kf_input):
    inp, kf, kf_feat = kf_input
    assert np.all(np.diff(kf_feat) > 0)
    info = {}
    m, n, km = reloc_cases.run(inp, info)
    drop = info["proj"]["drop"]
    assert n >= 100, n
    assert info["first_choice_taken"] >= 1
    assert info["removed"] >= 1
    for reason in (npref_reloc.DROP_FOV, npref_reloc.DROP_FACE, npref_reloc.DROP_DIST):
        assert (drop == reason).sum() >= 1, reason
    assert info["unfolded"] >= 1
    assert n == (m >= 0).sum() and np.array_equal(np.flatnonzero(km >= 0), np.sort(m[m >= 0]))
    assert np.array_equal(km[m[m >= 0]], np.flatnonzero(m >= 0))
    # the second search of Relocalization on the same input still finds something
    c2, _ = reloc_cases.variant(inp, kf_feat, 3, th=3.0, orb=64)
    assert reloc_cases.run(c2)[1] >= 20


def test_edge_and_cluster_inputs(kf_input):
    e = reloc_cases.edge_input()
    info = {}
    m, n, km = reloc_cases.run(e, info)
    assert 150 <= len(e["pos"]) <= 260 and n >= 40 and info["unfolded"] >= 20, (len(e["pos"]), n, info["unfolded"])
    c = reloc_cases.cluster_input()
    assert len(c["pos"]) == 8
    pr = npref_reloc.project(c["camd"]["face"], npref_reloc.cos_fov_th(c["camd"]), c["pose12"], c["pos"], c["min_dist"], c["max_dist"])
    lv = pr["level"]
    assert (pr["drop"] == 0).all()
    off, idx = npref_reloc._windows(orc.make_camera(c["camd"]), c["kx"], c["ky"], c["koct"], pr["u"], pr["v"], (np.float32(10) * c["sf"][lv]).astype(np.float32), lv - 1, lv + 1)
    assert off[-1] > 64 * 8 + 1024, off[-1]                           # beyond the first capacity
    assert reloc_cases.run(c)[1] >= 4


def test_library_exports_the_keyframe_projection_search():
    L = C.CDLL(os.path.join(ROOT, "cubemapslam_amd", "lib", "libcubemapslam_hip.so"))
    assert hasattr(L, "cms_search_by_projection_keyframe") and hasattr(L, "cms_kfstore_search_by_projection")
    H = C.CDLL(os.path.join(ROOT, "cubemapslam_amd", "lib", "libcubemapslam_host.so"))
    assert hasattr(H, "hm_search_by_projection_keyframe")


def test_kfproj_job_layout_matches_header(tmp_path):
    """api.KfProjJob against cms_kfproj_job as the C compiler lays it out from include/cubemapslam_hip.h (sizeof / offsetof of a probe program)"""
    fields = ("slot", "b", "n", "pose12", "nmp", "kf_feat", "pos", "min_dist", "max_dist", "mp_desc", "kp_mp", "match")
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cubemapslam_hip.h"\nint main(void) {\n  printf("%zu", sizeof(cms_kfproj_job));\n' +
                   "".join('  printf(" %%zu", offsetof(cms_kfproj_job, %s));\n' % f for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(api.KfProjJob)
    assert got[1:] == [getattr(api.KfProjJob, f).offset for f in fields]
