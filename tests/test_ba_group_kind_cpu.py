"""Which windows cms_ba_optimize_many puts into one group, and which kernel sums a window's Schur slices how
(cubemapslam_amd/csrc/cms_ba_group_kind.h).  The header's promise "same bits alone or in any group" for deterministic windows rests on this:
everything that selects a kernel whose rounding differs must be decided from the window alone and be part of the group key.  The header has no HIP
in it; tests/emu/ba_group_kind_emu.cpp evaluates it for the windows this test lists.  Built twice -- plain and AddressSanitizer + UBSan -- and
each build run as a child process (the sanitizer runtimes are linked into the program)."""
import itertools
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cubemapslam_amd", "csrc")
SRC = os.path.join(HERE, "emu", "ba_group_kind_emu.cpp")

BUILDS = {
    "plain": [],
    "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"],
}


def _define(fname, name):
    """the integer value of `#define name <arithmetic>` in a source file of the library"""
    txt = open(os.path.join(CSRC, fname)).read()
    m = re.search(r"^#define\s+%s\s+\(?([0-9*+\- ]+)\)?" % name, txt, re.M)
    assert m, (fname, name)
    return int(eval(m.group(1), {"__builtins__": {}}))


STRIDE = _define("cms_ba_fused.hip", "BA_S3_STRIDE")
CEILING = _define("cms_api_ba.hip", "BA_LDS_CEILING")
REDUCE_MAX = 24      # CMS_BA_SOLVE_REDUCE_MAX's default (ba_knobs, cms_api_ba.hip)
KEYS = ("device", "fast_plan", "edge_list", "deterministic", "det_points", "has_runs", "se_waves", "det_ranges", "np", "solve3_ok", "slices")


@pytest.fixture(scope="module", params=sorted(BUILDS))
def emu(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ba_group_kind") / ("ba_group_kind_emu_" + request.param))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + BUILDS[request.param] + [SRC, "-o", exe])

    def run(windows, stride=STRIDE, ceiling=CEILING, reduce_max=REDUCE_MAX):
        """windows: dicts with the fields of KEYS (solve3_ok defaults to np <= 25, the three-lane solve's limit) ->
        [(kind, solve_presum, solve_sums_slices, solve3_lds, presum_lds)]"""
        text = "".join(" ".join(str(int(w.get(k, w["np"] <= 25))) for k in KEYS) + "\n" for w in windows)
        r = subprocess.run([exe, str(stride), str(ceiling), str(reduce_max)], input=text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True,
                           timeout=120)
        assert r.returncode == 0 and "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]
        lines = r.stdout.split("\n")
        assert lines[len(windows)] == "ba_group_kind_emu: ok %d windows" % len(windows), lines[-3:]
        return [tuple(int(v) for v in ln.split()) for ln in lines[:len(windows)]]
    return run


def _win(np_, **kw):
    """a deterministic window of the fused chain: eight wavefronts, no runs, 16 workgroups; more slices than the solve kernel sums itself"""
    w = dict(device=0, fast_plan=0, edge_list=1, deterministic=1, det_points=0, has_runs=0, se_waves=8, det_ranges=16, np=np_, slices=REDUCE_MAX + 1)
    w.update(kw)
    return w


def _presum_bytes(np_, stride):
    """LDS of kb_ba_trial_solve3rp's launch for np free key frames, from the layout comment in ba_trial_solve3_body (cms_ba_fused.hip), in doubles:
    L panels [np (np - 1) / 2][stride] | diagonal factors [np][36] | W double buffer [2][np][stride] | diag staging [36] | y [6 np] | 1/D [6 np] | bp [6 np]
    | the slices' sums [np (np + 1) / 2][42]; the host adds eight spare doubles"""
    panels = stride * (np_ * (np_ - 1) // 2)
    diag = 36 * np_
    wbuf = 2 * stride * np_
    vectors = 3 * 6 * np_
    sums = 42 * (np_ * (np_ + 1) // 2)
    return 8 * (panels + diag + wbuf + 36 + vectors + 8 + sums)


def test_the_constants_are_the_ones_the_figures_below_were_worked_out_for():
    assert STRIDE == 38 and CEILING == 160 * 1024 - 512 == 163328
    txt = open(os.path.join(CSRC, "cms_api_ba.hip")).read()
    assert re.search(r'getenv\("CMS_BA_SOLVE_REDUCE_MAX"\); q\.solve_reduce_max = v \? atoi\(v\) : %d;' % REDUCE_MAX, txt)


def test_presum_threshold_follows_the_lds_formula(emu):
    """np = 1 .. 25 free key frames, the dense pair count: presum iff the launch's LDS fits -- true up to 20 (149 472 bytes), false from 21 (163 648)
    under the current ceiling; a window the three-lane solve does not take never presums"""
    out = emu([_win(n) for n in range(1, 26)])
    for n, (_, presum, _, lds3, need) in zip(range(1, 26), out):
        assert need == _presum_bytes(n, STRIDE) and lds3 == need - 8 * 42 * (n * (n + 1) // 2), n
        assert presum == (_presum_bytes(n, STRIDE) <= CEILING), n
        assert presum == (n <= 20), n
    assert out[19][3:] == (78912, 149472) and out[20][3:] == (86032, 163648)
    # the line moves with the ceiling and the stride, not with a constant of its own
    for stride, ceiling in ((38, 64 * 1024), (38, 149472), (38, 149471), (38, 163648), (40, CEILING), (36, 10 ** 6)):
        for n, (_, presum, _, _, need) in zip(range(1, 26), emu([_win(n) for n in range(1, 26)], stride, ceiling)):
            assert need == _presum_bytes(n, stride) and presum == (need <= ceiling), (stride, ceiling, n)
    assert [o[1] for o in emu([dict(_win(10), solve3_ok=0), dict(_win(30), solve3_ok=0)])] == [0, 0]


def test_deterministic_windows_of_one_kind_have_their_slices_summed_alike(emu):
    """every pair of deterministic windows (np1, np2) in 1 .. 25, with and without runs, 16 and 64 workgroups, every wavefront count, slice counts on both
    sides of solve_reduce_max: equal kind => equal presum decision and equal "the solve kernel sums the slices" decision (20 and 21 free key frames
    share the wavefront count 8, carry no runs and may share the workgroup count: only the presum term of the key keeps them apart; a window of 18
    chunks and one of 140, both cut into up to 64 workgroups, differ in nothing but their slice counts)"""
    wins = [_win(n, has_runs=r, det_ranges=g, se_waves=sw, slices=s) for n in range(1, 26) for r in (0, 1) for g in (16, 64) for sw in (2, 4, 6, 8)
            for s in (2, 16, 24, 25, 64) if s <= g]
    out = emu(wins)
    by_kind = {}
    for w, (kind, presum, sums, _, _) in zip(wins, out):
        assert presum == (w["np"] <= 20) and sums == (w["slices"] <= REDUCE_MAX)
        by_kind.setdefault(kind, set()).add((presum, sums))
    for kind, decisions in by_kind.items():
        assert len(decisions) == 1, (kind, decisions)
    k20, k21 = emu([_win(20), _win(21)])
    assert k20[0] != k21[0] and (k20[1], k21[1]) == (1, 0)
    k18, k64 = emu([_win(11, det_ranges=64, slices=18), _win(11, det_ranges=64, slices=64)])
    assert k18[0] != k64[0] and (k18[2], k64[2]) == (1, 0)
    # ... and the terms separate nothing else: windows on one side of a line that agree in the rest share a kind
    assert len({o[0] for o in emu([_win(n) for n in range(1, 21)])}) == 1 and len({o[0] for o in emu([_win(n) for n in range(21, 26)])}) == 1
    assert len({o[0] for o in emu([_win(7, det_ranges=64, slices=s) for s in range(2, 25)])}) == 1
    assert len({o[0] for o in emu([_win(7, det_ranges=64, slices=s) for s in range(25, 65)])}) == 1


# the key's value for windows without either of the two terms (21 free key frames, 25 slices), as cms_ba_optimize_many computed it before they
# existed: device * 8 + 4 fast_plan + 2 edge_list + deterministic, and for deterministic windows
# + 1024 * (1 + det_points + 2 has_runs + 4 min(max(se_waves, 0), 15) + 64 det_ranges)
KEY_TABLE = [
    (dict(deterministic=0), 2),
    (dict(deterministic=0, device=1, fast_plan=1), 14),
    (dict(deterministic=0, edge_list=0), 0),
    (dict(), 1082371),
    (dict(has_runs=1), 1084419),
    (dict(det_points=1), 1083395),
    (dict(se_waves=6), 1074179),
    (dict(det_ranges=64), 4228099),
    (dict(fast_plan=1), 1082375),
    (dict(device=2), 1082387),
    (dict(det_ranges=128, has_runs=1), 8424451),
    (dict(se_waves=20), 1082371 + 1024 * 4 * 7),      # clamped to 15
    (dict(se_waves=-1), 1082371 - 1024 * 4 * 8),      # clamped to 0
]


def test_the_key_separates_what_it_separated_before(emu):
    out = emu([_win(21, **kw) for kw, _ in KEY_TABLE])
    assert [o[0] for o in out] == [want for _, want in KEY_TABLE]
    # the two new terms: one bit each above everything else, for deterministic windows only (slices: of the fused chain only)
    for (kw, want), (k, presum, sums, _, _) in zip(KEY_TABLE, emu([_win(20, **kw) for kw, _ in KEY_TABLE])):
        assert presum == 1 and sums == 0 and k == want + ((1 << 24) if kw.get("deterministic", 1) else 0), kw
    for (kw, want), (k, presum, sums, _, _) in zip(KEY_TABLE, emu([_win(21, slices=REDUCE_MAX, **kw) for kw, _ in KEY_TABLE])):
        fused_det = kw.get("deterministic", 1) and not kw.get("det_points", 0)
        assert presum == 0 and sums == fused_det and k == want + ((1 << 25) if fused_det else 0), kw
    # every combination: two windows share a kind iff they agree in device, planner, edge list and mode, and -- deterministic ones -- in path, runs,
    # wavefront count (0 .. 15), workgroup count, presum decision and who sums the slices
    fields = dict(device=(0, 1, 3), fast_plan=(0, 1), edge_list=(0, 1), deterministic=(0, 1), det_points=(0, 1), has_runs=(0, 1), se_waves=(-1, 0, 2, 6, 8, 15, 20),
                  det_ranges=(2, 16, 64, 128), np=(20, 21), slices=(24, 25))
    wins = [dict(zip(fields, v)) for v in itertools.product(*fields.values())]

    def want(w):
        t = (w["device"], w["fast_plan"], w["edge_list"], w["deterministic"])
        if w["deterministic"]:
            t += (w["det_points"], w["has_runs"], min(max(w["se_waves"], 0), 15), w["det_ranges"], w["np"] <= 20,
                  w["slices"] <= REDUCE_MAX and not w["det_points"] and bool(w["edge_list"]))
        return t
    kinds = {}
    for w, o in zip(wins, emu(wins)):
        kinds.setdefault(o[0], set()).add(want(w))
    assert all(len(v) == 1 for v in kinds.values()), [v for v in kinds.values() if len(v) > 1][:3]
    assert len(kinds) == len({want(w) for w in wins})
