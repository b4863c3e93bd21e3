"""ORBMatcher::SearchBySim3 (src/ORBMatcher.cpp:1365-1586) without a GPU: the conditions on the shared cases (tests/sim3_search_cases.py), the host
build of csrc/cms_sim3_search_core.h against the restatement tests/npref_sim3_search.py bit for bit, the job check of cms_kfstore_search_by_sim3,
and the record's layout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import npref_sim3_search as ref
import sim3_search_cases as cases
import sim3_search_hostlib as host
from cubemapslam_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- conditions on the inputs
@pytest.mark.parametrize("zw", [False, True], ids=["corrected", "as_written"])
def test_hand_built_answers(zw):
    assert cases.hand_sites_apart()
    hc = cases.hand_cases(zw)
    assert len(hc) >= 35
    for name, c, want in hc:
        idx2, n = cases.run(c, zw)
        assert list(idx2) == want and n == sum(w >= 0 for w in want), (name, list(idx2), want)


def test_only_z_as_written_decides_one_hand_case():
    for (name, c, a), (_, _, b) in zip(cases.hand_cases(False), cases.hand_cases(True)):
        assert (a != b) == (name == "only z_as_written decides"), name


@pytest.mark.parametrize("written", [False, True], ids=["corrected", "as_written"])
def test_seeded_families_have_matches(written):
    fam = cases.family(written)
    own = [cases.run(c, written) for c in fam]
    other = [cases.run(c, not written) for c in fam]
    assert sum(n for _, n in own) >= 50 and all(n >= 50 for (_, n), c in zip(own, fam) if len(c["kf1"]["kx"]) >= 257)
    for (i, n) in own + other:
        assert n == int((i >= 0).sum())
    # direction 1 -> 2 does not read key frame 1's key points, but the agreement does: each family matches in its own mode and loses nearly all in the other
    assert all(not np.array_equal(a[0], b[0]) for a, b in zip(own, other))
    assert sum(n for _, n in other) * 5 < sum(n for _, n in own)


def test_seeded_cases_reach_what_they_are_for():
    for written in (False, True):
        for c in cases.family(written):
            n1, n2 = len(c["kf1"]["kx"]), len(c["kf2"]["kx"])
            assert all(n % 8 and n % 32 and n % 64 for n in (n1, n2, n1 + n2)) and n2 == n1 + 5
            if n1 >= 257:
                assert all(0.1 < (mp["skip"] != 0).mean() < 0.4 for mp in (c["mp1"], c["mp2"]))      # a third are distractors, half of those without a point
    c = cases.dense_case()
    for zw in (False, True):
        info = {}
        _, n = cases.run(c, zw, info)
        assert info["ncand"] > 64 * info["entries"] + 1024                # the first attempt's capacity is too small in either mode
        assert (n >= 50) == (not zw)
    s = cases.self_case(cases.family(False)[1])
    assert cases.run(s, False)[1] >= 50
    e = cases.family(False)[0]
    assert cases.run(cases.empty_side_case(e, True))[1] == 0 and cases.run(cases.empty_side_case(e, False))[1] == 0


def test_distance_bounds_modes_agree_on_the_seeded_cases():
    c = cases.family(True)[1]
    a, b = cases.run(c, True), cases.run(c, True, bounds_scaled=1)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]


# ---------------------------------------------------------------------------------------------------------------- the host build of the core
EDGE_S12 = [1.0, 0.7, 1.4, 3.0, 1e-3, 1e3, -2.0, np.float32(1) / np.float32(3)]


def test_compose_bit_equal():
    rng = np.random.default_rng(3)
    sims = [(c["s12"], c["R12"], c["t12"]) for w in (False, True) for c in cases.family(w)]
    sims += [(s, cases.synth._rot(rng.normal(0, 1, 3), rng.uniform(0, 3.0)), rng.uniform(-5, 5, 3)) for s in EDGE_S12 for _ in range(4)]
    sims += [(2.0, np.eye(3), np.zeros(3)), (1.0, np.eye(3), [0.0, -0.0, 1.0])]
    for s12, R12, t12 in sims:
        want, got = ref.compose(s12, R12, t12), host.compose(s12, R12, t12)
        for k in ("sR12", "t12", "sR21", "t21"):
            assert np.array_equal(bits(want[k]), bits(got[k])), (k, s12)


def _both_projections(c, second, zw, bounds_scaled=0):
    m = ref.compose(c["s12"], c["R12"], c["t12"])
    kf, mp = (c["kf2"], c["mp2"]) if second else (c["kf1"], c["mp1"])
    sR, t = (m["sR12"], m["t12"]) if second else (m["sR21"], m["t21"])
    mn, mx = mp["min_dist"], mp["max_dist"]
    if bounds_scaled:
        mn = (np.float32(0.8) * mn).astype(np.float32); mx = (np.float32(1.2) * mx).astype(np.float32)
    pos = np.nan_to_num(mp["pos"], nan=3.0)
    a = ref.project(cases.F, kf["pose12"], sR, t, pos, mn, mx, second_as_depth=second and zw, bounds_scaled=bounds_scaled)
    b = host.project(cases.F, kf["pose12"], sR, t, pos, mn, mx, second_as_depth=second and zw, bounds_scaled=bounds_scaled)
    return a, b


def _same_projection(a, b, what):
    assert np.array_equal(a["drop"], b["drop"]), (what, np.flatnonzero(a["drop"] != b["drop"])[:8])
    for k in ("u", "v", "dist", "raw_max"):
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k, np.flatnonzero(bits(a[k]) != bits(b[k]))[:8])


def test_project_bit_equal_on_seeded_points():
    seen = set()
    for written in (False, True):
        for c in cases.family(written) + ([cases.dense_case()] if not written else []):
            for second in (False, True):
                for zw in (False, True):
                    for mode in (0, 1):
                        a, b = _both_projections(c, second, zw, mode)
                        _same_projection(a, b, (written, second, zw, mode))
                        seen |= set(a["drop"].tolist())
    assert seen == {ref.KEEP, ref.BEHIND, ref.IMAGE, ref.DIST}


def test_project_bit_equal_on_edge_values():
    for zw in (False, True):
        for name, c, _ in cases.hand_cases(zw):
            for second in (False, True):
                if len((c["mp2"] if second else c["mp1"])["skip"]) == 0:
                    continue
                _same_projection(*_both_projections(c, second, zw), what=(name, second, zw))
    # rays on the seams and corners of the faces, the camera centre, zero depth, a NaN
    v = [0.0, -0.0, 1.0, -1.0, 5.0, -5.0, np.nextafter(np.float32(5), np.float32(6)), np.nextafter(np.float32(5), np.float32(4)), 1e-30, 1e30]
    pts = np.array([(x, y, z) for x in v for y in v for z in v] + [(np.nan, 1.0, 1.0), (1.0, 1.0, np.inf)], np.float32)
    n = len(pts)
    mn = np.full(n, 0.1, np.float32); mx = np.full(n, 4.0, np.float32)
    ident = cases.IDENT
    for second_as_depth in (False, True):
        with np.errstate(all="ignore"):
            a = ref.project(cases.F, ident, np.eye(3, dtype=np.float32), np.zeros(3, np.float32), pts, mn, mx, second_as_depth=second_as_depth)
        b = host.project(cases.F, ident, np.eye(3, dtype=np.float32), np.zeros(3, np.float32), pts, mn, mx, second_as_depth=second_as_depth)
        assert np.array_equal(a["drop"], b["drop"])
        for k in ("u", "v"):
            assert np.array_equal(bits(a[k]), bits(b[k])), k
        ok = np.isfinite(a["dist"])
        assert np.array_equal(bits(a["dist"][ok]), bits(b["dist"][ok])) and np.array_equal(np.isnan(a["dist"]), np.isnan(b["dist"]))


# ---------------------------------------------------------------------------------------------------------------- the job check
def _job(**kw):
    j = dict(slot1=0, n1=10, slot2=1, n2=12, s12=1.25, R12=np.eye(3), t12=np.zeros(3), off1=0, off2=10)
    j.update(kw)
    return j


USED, SLOT_N = [1, 1, 0, 1], [10, 12, 5, 0]


def test_job_check_accepts():
    assert host.job_check([_job()], USED, SLOT_N, 22) == (0, "")
    assert host.job_check([], USED, SLOT_N, 0) == (0, "")
    assert host.job_check([_job(), _job(off1=22, off2=32)], USED, SLOT_N, 44) == (0, "")
    assert host.job_check([_job(off1=3, off2=20)], USED, SLOT_N, 40) == (0, "")                         # gaps between the records are allowed
    assert host.job_check([_job(slot2=0, n2=10)], USED, SLOT_N, 20) == (0, "")                          # slot1 == slot2
    assert host.job_check([_job(slot1=3, n1=0, off2=0)], USED, SLOT_N, 12) == (0, "")                   # a key frame without key points
    assert host.job_check([_job(s12=-0.5)], USED, SLOT_N, 22, th=0.0) == (0, "")


@pytest.mark.parametrize("jobs,kw,reason", [
    ([_job(slot1=-1)], {}, "slot out of range"),
    ([_job(slot2=4)], {}, "slot out of range"),
    ([_job(slot1=2, n1=5)], {}, "empty slot"),
    ([_job(n1=9)], {}, "n1 / n2 is not the slot's stored key-point count"),
    ([_job(n2=13)], {}, "n1 / n2 is not the slot's stored key-point count"),
    ([_job(s12=0.0)], {}, "s12 must be finite and nonzero"),
    ([_job(s12=np.inf)], {}, "s12 must be finite and nonzero"),
    ([_job(s12=np.nan)], {}, "s12 must be finite and nonzero"),
    ([_job(off1=-1)], {}, "off1 does not ascend or reaches beyond n_mp"),
    ([_job(off1=13, off2=23)], {}, "off1 does not ascend or reaches beyond n_mp"),
    ([_job(off1=12, off2=22)], {}, "off2 does not ascend or reaches beyond n_mp"),
    ([_job(off2=9)], {}, "off2 does not ascend or reaches beyond n_mp"),
    ([_job(off2=11)], {}, "off2 does not ascend or reaches beyond n_mp"),
    ([_job(off1=2 ** 31 - 5, off2=2 ** 31 - 1)], {}, "off1 does not ascend or reaches beyond n_mp"),
    ([_job(), _job(off1=21, off2=31)], dict(n_mp=60), "off1 does not ascend or reaches beyond n_mp"),      # the second job starts inside the first
    ([_job()], dict(th=-1.0), "th must be finite and >= 0"),
    ([_job()], dict(th=np.nan), "th must be finite and >= 0"),
    ([_job()], dict(th=np.inf), "th must be finite and >= 0"),
    ([_job()], dict(nlevels=17), "more than 16 pyramid levels"),
    ([_job()], dict(same_device=False), "the context and the store must share the device"),
    ([_job()], dict(n_mp=-1), "n_mp is negative"),
])
def test_job_check_refuses(jobs, kw, reason):
    kw = dict(kw)
    n_mp = kw.pop("n_mp", 22)
    assert host.job_check(jobs, USED, SLOT_N, n_mp, **kw) == (-1, reason)


# ---------------------------------------------------------------------------------------------------------------- exports and layout
def test_libraries_export_the_search():
    assert hasattr(api.lib(), "cms_kfstore_search_by_sim3")
    for name in ("hm_sim3s_compose", "hm_sim3s_project", "hm_sim3s_job_check", "hm_search_by_sim3"):
        assert hasattr(host.H(), name), name


def test_job_layout_matches_header(tmp_path):
    """api.Sim3SearchJob and the host helper's Job against cms_sim3_search_job as the C compiler lays it out from include/cubemapslam_hip.h"""
    fields = ("slot1", "n1", "slot2", "n2", "s12", "R12", "t12", "off1", "off2")
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cubemapslam_hip.h"\nint main(void) {\n  printf("%zu", sizeof(cms_sim3_search_job));\n' +
                   "".join('  printf(" %%zu", offsetof(cms_sim3_search_job, %s));\n' % f for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    for S in (api.Sim3SearchJob, host.Job):
        assert got[0] == C.sizeof(S) and got[1:] == [getattr(S, f).offset for f in fields]
