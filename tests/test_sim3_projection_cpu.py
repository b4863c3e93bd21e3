"""ORBMatcher::SearchByProjection(KeyFrame*, Scw, ...) (src/ORBMatcher.cpp:796-903) and the search half of ORBMatcher::Fuse(KeyFrame*, Scw, ...)
(:1246-1363) without a GPU: the hand-built answers and the conditions on the shared cases (tests/sim3_projection_cases.py), the host build of
csrc/cms_sim3_proj_core.h against the restatement tests/npref_sim3_projection.py bit for bit, the job check of the two entries, and the record's
layout."""
import ctypes as C
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import npref_sim3_projection as ref
import sim3_projection_cases as cases
import sim3_projection_hostlib as host
from cubemapslam_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- conditions on the inputs
def test_hand_built_answers():
    hc = cases.hand_cases()
    assert len(hc) >= 35
    for name, c, match, best, dist in hc:
        dist = [10 if b >= 0 else 256 for b in best] if dist is None else dist      # (key points and points of the plain cases are 10 bits apart)
        gm, gn = cases.run_sbp(c)
        gb, gd = cases.run_fuse(c)
        assert list(gm) == match and gn == sum(m >= 0 for m in match), (name, list(gm), match)
        assert list(gb) == best and list(gd) == dist, (name, list(gb), best, list(gd), dist)


def test_hand_cases_do_not_read_the_stored_pose():
    """every hand-built key frame carries a stored pose under which its first point would not be seen where its key point waits"""
    for name, c, match, _, _ in cases.hand_cases():
        if not any(m >= 0 for m in match):
            continue
        stored = np.concatenate([c["kf"]["pose12"][:9].reshape(3, 3), c["kf"]["pose12"][9:].reshape(3, 1)], 1)
        assert cases.run_sbp(dict(c, Scw=stored))[1] == 0, name


def test_seeded_cases_reach_what_they_are_for():
    drops = Counter()
    depth = []
    for c in cases.family() + [cases.dense_case()]:
        nk, n = len(c["kf"]["kx"]), len(c["skip"])
        assert all(v % 8 and v % 32 and v % 64 for v in (nk, n))
        info = {}
        m, nm = cases.run_sbp(c, info)
        assert nm == int((m >= 0).sum())
        taken_now = m[m >= 0]
        assert len(set(taken_now.tolist())) == len(taken_now) and not c["taken"][taken_now].any()      # no key point twice, none that was taken on entry
        drops.update(info["drop"].tolist())
        depth.append(info["depth"])
        if nk >= 257:
            assert nm >= 50
            loose, _ = cases.run_sbp(c, sequential=False)
            assert int((loose != m).sum()) >= 10                          # sequencing matters: the twins
        b, d = cases.run_fuse(c)
        assert ((b >= 0) == (d <= 50)).all() and (d[b < 0] == 256).all()
    assert all(drops[k] >= 20 for k in (ref.KEEP, ref.BEHIND, ref.IMAGE, ref.DIST, ref.ANGLE, -1)), drops
    assert max(depth) >= 3                                                # a parallel resolution needs at least three rounds somewhere
    info = {}
    cases.run_sbp(cases.dense_case(), info)
    assert info["ncand"] > 64 * info["entries"] + 1024                    # the first attempt's capacity is too small


def test_many_jobs_case():
    kfs, sets, jobs = cases.many_jobs()
    assert len(jobs) == 7 and sum(len(s["pos"]) > 0 for s in sets) == 2
    assert any(a[0] == b[0] and not np.array_equal(a[1], b[1]) for a in jobs for b in jobs)      # one slot under two Scw
    assert any(len(kfs[j[0]]["kx"]) == 0 for j in jobs) and any(len(sets[j[2]]["pos"]) == 0 for j in jobs)
    assert sum(cases.run_sbp(cases.job_case(kfs, sets, j))[1] > 0 for j in jobs) >= 3


def test_distance_bounds_modes_agree():
    for c in cases.family()[:2] + [cases.hand_cases()[0][1]]:
        a, b = cases.run_sbp(c), cases.run_sbp(c, bounds_scaled=1)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]
        a, b = cases.run_fuse(c), cases.run_fuse(c, bounds_scaled=1)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------------------------- the host build of the core
EDGE_S = [1.0, 0.7, 1.4, 3.0, 1e-3, 1e3, np.float32(1) / np.float32(3)]


def _edge_scws():
    rng = np.random.default_rng(3)
    out = [c["Scw"] for c in cases.family() + [cases.dense_case()]] + [c["Scw"] for _, c, _, _, _ in cases.hand_cases()]
    out += [cases.make_scw(s, cases.synth._rot(rng.normal(0, 1, 3), rng.uniform(0, 3.0)), rng.uniform(-5, 5, 3)) for s in EDGE_S for _ in range(4)]
    out += [cases.make_scw(2.0, np.diag([1.0, 1.0, -1.0]), (0.5, -0.25, 1.0)),                    # a negative determinant
            cases.make_scw(1.0, np.eye(3), [0.0, -0.0, 1.0])]
    return out


def test_decompose_bit_equal():
    for S in _edge_scws():
        want, got = ref.decompose(S), host.decompose(S)
        for k in ("scw", "Rcw", "tcw", "Ow"):
            assert np.array_equal(bits(want[k]), bits(got[k])), (k, S)


def _same_projection(a, b, what):
    assert np.array_equal(a["drop"], b["drop"]), (what, np.flatnonzero(a["drop"] != b["drop"])[:8])
    assert np.array_equal(a["level"], b["level"]), (what, np.flatnonzero(a["level"] != b["level"])[:8])
    for k in ("u", "v", "dist", "radius"):
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k, np.flatnonzero(bits(a[k]) != bits(b[k]))[:8])


def test_project_bit_equal_on_all_cases():
    seen = set()
    every = [("seeded", c) for c in cases.family() + [cases.dense_case()]] + [(name, c) for name, c, _, _, _ in cases.hand_cases()]
    for name, c in every:
        if len(c["skip"]) == 0:
            continue
        for mode in (0, 1):
            pts = cases.scaled_pts(c["pts"]) if mode else c["pts"]
            for th in (c["th"], 4.0):
                a = ref.project(cases.F, c["Scw"], pts["pos"], pts["normal"], pts["min_dist"], pts["max_dist"], th, c["sf"], mode)
                b = host.project(cases.F, c["Scw"], pts["pos"], pts["normal"], pts["min_dist"], pts["max_dist"], th, c["sf"], mode)
                _same_projection(a, b, (name, mode, th))
                seen |= set(a["drop"].tolist())
    assert seen == {ref.KEEP, ref.BEHIND, ref.IMAGE, ref.DIST, ref.ANGLE}


def test_project_bit_equal_on_edge_values():
    """rays on the seams and corners of the faces, the camera centre, zero depth, a NaN, under the edge similarities"""
    v = [0.0, -0.0, 1.0, -1.0, 5.0, -5.0, np.nextafter(np.float32(5), np.float32(6)), np.nextafter(np.float32(5), np.float32(4)), 1e-30, 1e30]
    pts = np.array([(x, y, z) for x in v for y in v for z in v] + [(np.nan, 1.0, 1.0), (1.0, 1.0, np.inf)], np.float32)
    n = len(pts)
    nrm = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (n, 1))
    mn = np.full(n, 0.1, np.float32); mx = np.full(n, 4.0, np.float32)
    for S in [cases.IDENT_S] + _edge_scws()[-30:]:
        with np.errstate(all="ignore"):
            a = ref.project(cases.F, S, pts, nrm, mn, mx, 10.0, cases.SF)
        b = host.project(cases.F, S, pts, nrm, mn, mx, 10.0, cases.SF)
        assert np.array_equal(a["drop"], b["drop"]) and np.array_equal(a["level"], b["level"])
        for k in ("u", "v", "radius"):
            assert np.array_equal(bits(a[k]), bits(b[k])), k
        ok = np.isfinite(a["dist"])
        assert np.array_equal(bits(a["dist"][ok]), bits(b["dist"][ok])) and np.array_equal(np.isnan(a["dist"]), np.isnan(b["dist"]))


# ---------------------------------------------------------------------------------------------------------------- the job check
def _job(**kw):
    j = dict(slot=0, n=10, Scw=cases.make_scw(1.25, np.eye(3), (0.1, 0.2, 0.3)), set=0)
    j.update(kw)
    return j


USED, SLOT_N, SET_OFF = [1, 1, 0, 1], [10, 12, 5, 0], [0, 7, 7, 20]


def _scw_with(k, value, s=1.25):
    S = cases.make_scw(s, np.eye(3), (0.1, 0.2, 0.3)).copy()
    S.reshape(-1)[k] = value
    return S


def test_job_check_accepts():
    assert host.job_check([_job()], USED, SLOT_N, SET_OFF) == (0, "")
    assert host.job_check([], USED, SLOT_N, SET_OFF) == (0, "")
    assert host.job_check([_job(), _job(slot=1, n=12, set=2), _job(set=2)], USED, SLOT_N, SET_OFF) == (0, "")      # jobs share sets and slots
    assert host.job_check([_job(set=1)], USED, SLOT_N, SET_OFF) == (0, "")                                        # an empty set
    assert host.job_check([_job(slot=3, n=0)], USED, SLOT_N, SET_OFF) == (0, "")                                  # a key frame without key points
    assert host.job_check([_job(Scw=cases.make_scw(-0.5, np.eye(3), (0, 0, 0)))], USED, SLOT_N, SET_OFF, th=0.0) == (0, "")


@pytest.mark.parametrize("jobs,kw,reason", [
    ([_job(slot=-1)], {}, "slot out of range"),
    ([_job(slot=4)], {}, "slot out of range"),
    ([_job(slot=2, n=5)], {}, "empty slot"),
    ([_job(n=9)], {}, "n is not the slot's stored key-point count"),
    ([_job(n=-1)], {}, "n is not the slot's stored key-point count"),
    ([_job(set=-1)], {}, "set out of range"),
    ([_job(set=3)], {}, "set out of range"),
    ([_job()], dict(set_off=[0, 7, 6, 20]), "set offsets must ascend"),
    ([_job()], dict(set_off=[1, 7, 7, 20]), "set offsets must start at 0"),
    ([_job(Scw=np.zeros((3, 4), np.float32))], {}, "scw must be finite and nonzero"),
    ([_job(Scw=_scw_with(1, 3e38, s=3e38))], {}, "scw must be finite and nonzero"),                                     # every entry finite, the norm of row 0 not
    ([_job(Scw=_scw_with(1, np.nan))], {}, "Scw must be finite"),
    ([_job(Scw=_scw_with(7, np.inf))], {}, "Scw must be finite"),
    ([_job(Scw=_scw_with(11, -np.inf))], {}, "Scw must be finite"),
    ([_job(), _job(slot=1, n=11)], {}, "n is not the slot's stored key-point count"),                             # a later job
    ([_job()], dict(th=-1.0), "th must be finite and >= 0"),
    ([_job()], dict(th=np.nan), "th must be finite and >= 0"),
    ([_job()], dict(th=np.inf), "th must be finite and >= 0"),
    ([_job()], dict(nlevels=17), "more than 16 pyramid levels"),
    ([_job()], dict(same_device=False), "the context and the store must share the device"),
])
def test_job_check_refuses(jobs, kw, reason):
    kw = dict(kw)
    set_off = kw.pop("set_off", SET_OFF)
    assert host.job_check(jobs, USED, SLOT_N, set_off, **kw) == (-1, reason)


# ---------------------------------------------------------------------------------------------------------------- exports and layout
def test_libraries_export_the_entries():
    for name in ("cms_kfstore_search_by_projection_sim3", "cms_kfstore_fuse_search_sim3", "cms_sim3_proj_last_rounds"):
        assert hasattr(api.lib(), name), name
    for name in ("hm_sim3p_decompose", "hm_sim3p_project", "hm_sim3p_job_check", "hm_search_by_projection_sim3", "hm_fuse_sim3"):
        assert hasattr(host.H(), name), name
    assert hasattr(api.KeyframeStore, "search_by_projection_sim3") and hasattr(api.KeyframeStore, "fuse_search_sim3")


def test_job_layout_matches_header(tmp_path):
    """api.Sim3ProjJob and the host helper's Job against cms_sim3_proj_job as the C compiler lays it out from include/cubemapslam_hip.h"""
    fields = ("slot", "n", "Scw", "set")
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cubemapslam_hip.h"\nint main(void) {\n  printf("%zu", sizeof(cms_sim3_proj_job));\n' +
                   "".join('  printf(" %%zu", offsetof(cms_sim3_proj_job, %s));\n' % f for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    for S in (api.Sim3ProjJob, host.Job):
        assert got[0] == C.sizeof(S) and got[1:] == [getattr(S, f).offset for f in fields]
    assert host.H().hm_sim3p_job_size() == got[0]
