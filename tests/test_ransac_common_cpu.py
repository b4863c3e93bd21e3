"""What the PnP, Sim3 and two-view solvers share, without a GPU: cms_ransac_core.h and cms_ransac_job_check.h compiled on their own by g++
(tests/emu/ransac_common_emu.cpp) -- the draw resolver against the literal swap-and-pop, the hypothesis counts of a call and what the PnP and the
Sim3 job check make of them, the byte <-> bit form of a mask, and the iteration count of SetRansacParameters.  The same cases then go through the
stand-alone program under the host sanitizers."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import init_cases as ic
import pnp_cases as pc
import sim3_cases as sc
from cubemapslam_amd import api
from hostlib import p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "ransac_common_emu.cpp")
GPP = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "cubemapslam_amd", "csrc"), "-I", os.path.join(ROOT, "include")]
INT_MIN = -2 ** 31
SWAP_AND_POP = {3: sc.swap_and_pop, 4: pc.swap_and_pop, 8: ic.swap_and_pop}


@pytest.fixture(scope="module")
def E(tmp_path_factory):
    so = tmp_path_factory.mktemp("ransac_emu") / "ransac_common_emu.so"
    subprocess.check_call(GPP + ["-O2", "-fPIC", "-shared", EMU, "-o", str(so)])
    E = C.CDLL(str(so))
    E.emu_resolve_draws.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    E.emu_hypotheses.argtypes = [C.c_int] * 5 + [C.c_void_p] * 2
    E.emu_hypotheses.restype = None
    E.emu_pnp_check_job.argtypes = [C.c_void_p, C.c_void_p]
    E.emu_sim3_check_job.argtypes = [C.c_void_p] * 3
    E.emu_iterations.argtypes = [C.c_double, C.c_float]
    E.emu_mask_pack.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    E.emu_mask_pack.restype = None
    E.emu_mask_unpack.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    E.emu_mask_unpack.restype = None
    return E


# ---------------------------------------------------------------------------------------------------------------- the cases

def draw_rows():
    """(K, N, row): 60 random rows per N and the extreme ones"""
    rng = np.random.default_rng(21)
    rows = []
    for K in (3, 4, 8):
        for N in (K, K + 1, K + 2, 9, 64):
            for _ in range(60):
                rows.append((K, N, [int(rng.integers(0, N - k)) for k in range(K)]))
            rows.append((K, N, [0] * K))                                                  # always the first: from k = 1 on a position written before
            rows.append((K, N, [N - 1 - k for k in range(K)]))                            # always the current last
            rows.append((K, N, [(N - 1 - k) if k % 2 == 0 else 0 for k in range(K)]))     # the last, then the first, ...
            rows.append((K, N, [0 if k % 2 == 0 else (N - 1 - k) for k in range(K)]))     # the first (written before), then the last, ...
            rows.append((K, N, [min(1, N - 1 - k) for k in range(K)]))                    # position 1 again and again, until it is the last
    return rows


def hypothesis_rows():
    """(N, min_inliers, max_its, iterations, n_iterations), (H_max, H_min): left = max_its - iterations negative, zero, below, at and above n_iterations"""
    rows = []
    for left, n_it in ((-3, 5), (-3, 0), (0, 5), (0, 0), (2, 5), (5, 5), (9, 5), (9, 0), (1, 1 << 20), (1 << 20, 1)):
        rows.append(((30, 10, 10 + left, 10, n_it), (max(left, n_it, 0), max(min(left, n_it), 0))))
    rows.append(((9, 10, 40, 10, 5), (0, 0)))                                             # N < min_inliers: the solvers return before the loop
    rows.append(((10, 10, 40, 10, 5), (30, 5)))                                           # N == min_inliers: they do not
    return rows


def mask_rows():
    rng = np.random.default_rng(22)
    rows = []
    for N in (0, 1, 63, 64, 65, 128, 129):
        rows.append(np.zeros(N, np.uint8))
        rows.append(np.ones(N, np.uint8))
        rows.append((rng.uniform(size=N) < 0.5).astype(np.uint8) * rng.integers(1, 256, N).astype(np.uint8))      # any non-zero byte is an inlier
    return rows


def literal_iterations(probability, epsilon):
    """ceil(log(1 - p) / log(1 - eps^3)) in double on the float epsilon; INT_MIN for NaN and for what no int holds (x86's cvttsd2si)"""
    with np.errstate(all="ignore"):
        v = np.ceil(np.log(np.float64(1) - np.float64(probability)) / np.log(np.float64(1) - np.float64(np.float32(epsilon)) ** 3))
    return int(v) if np.isfinite(v) and -2147483648.0 <= v < 2147483648.0 else INT_MIN


def iteration_rows():
    """(probability, epsilon, pinned value or None)"""
    f32 = np.float32
    rows = [(0.99, 0.5, 35),                               # test_pnp_cpu: (20, 0.99, 10, 300, 4, 0.5); test_sim3_cpu: (40, 0.99, 20, 300)
            (0.5, 0.5, 6),                                 # test_sim3_cpu: (40, 0.5, 20, 300)
            (0.99, f32(10) / f32(15), 14),                 # test_pnp_cpu: (15, 0.99, 10, 300, 4, 0.5)
            (0.99, 0.1, 4603),                             # test_pnp_cpu: (200, 0.99, 10, 300, 4, 0.1), cut to 300 by the entry
            (0.99, f32(4) / f32(3), INT_MIN),              # test_pnp_cpu: N = 3 < minSet, the log of a negative number
            (0.99, f32(20) / f32(19), INT_MIN),            # test_sim3_cpu: (19, 0.99, 20, 300)
            (0.99, f32(np.inf), INT_MIN),                  # test_sim3_cpu: N = 0
            (0.99, f32(np.nan), INT_MIN),                  # test_sim3_cpu: N = 0 and minInliers = 0
            (0.99, 1.0, 0),                                # log(0) = -inf below: -0.0, the entries then say max(1, .)
            (1.0, 0.5, INT_MIN),                           # log(0) = -inf above: +inf
            (1.0, 1.0, INT_MIN)]                           # -inf / -inf
    for N, mi in ((100, 20), (25, 20), (21, 20), (7, 6), (300, 6), (50, 45), (60, 20)):      # the table of test_sim3_cpu.test_ransac_parameters
        rows.append((0.99, f32(mi) / f32(N), None))
    return rows


# ---------------------------------------------------------------------------------------------------------------- the shared library

def test_resolver_is_the_literal_swap_and_pop(E):
    rows = draw_rows()
    assert len(rows) == 3 * 5 * 65
    for K, N, row in rows:
        idx = np.full(K + 2, -7, np.int32)
        assert E.emu_resolve_draws(K, N, p(np.array(row, np.int32)), p(idx)) == 0
        assert list(idx[:K]) == SWAP_AND_POP[K](N, row), (K, N, row)
        assert (idx[K:] == -7).all()
        assert len(set(idx[:K])) == K and idx[:K].min() >= 0 and idx[:K].max() < N


def hypotheses(E, row):
    H = (C.c_int * 2)(-1, -1)
    E.emu_hypotheses(*row, C.byref(H, 0), C.byref(H, 4))
    return H[0], H[1]


def test_hypothesis_counts(E):
    for row, want in hypothesis_rows():
        assert hypotheses(E, row) == want, row


def test_pnp_runs_h_max_and_sim3_brings_h_max_and_runs_h_min(E):
    ppr = pc.problem(3, N=30, outliers=0.2)
    spr = sc.problem(3, N=30, outliers=0.2)
    for (N_, mi, max_its, its, n_it), (H_max, H_min) in hypothesis_rows():
        if max(max_its, n_it) > 64:
            continue                                       # (the draws of 2^20 iterations: the arithmetic is pinned above)
        carried = dict(min_inliers=mi + 30 - N_, max_its=max_its, iterations=its)      # 30 correspondences: N < min_inliers by a higher bar
        ps = api.pnp_job_state(dict(ppr, **carried), n_it, pc.draws(4, 30, H_max))
        H = C.c_int(-1)
        assert E.emu_pnp_check_job(api.pnp_jobs([ps]), C.byref(H)) == 0 and H.value == H_max
        ss = api.sim3_job_state(dict(spr, **carried), n_it, sc.draws(4, 30, H_max))
        Hd, Hr = C.c_int(-1), C.c_int(-1)
        assert E.emu_sim3_check_job(api.sim3_jobs([ss]), C.byref(Hd), C.byref(Hr)) == 0 and (Hd.value, Hr.value) == (H_max, H_min)
        if H_max > 0:                                      # one row of draws short of H_max: both refuse, also where Sim3 would run fewer
            ps = api.pnp_job_state(dict(ppr, **carried), n_it, pc.draws(4, 30, H_max - 1))
            assert E.emu_pnp_check_job(api.pnp_jobs([ps]), C.byref(H)) == -1
            ss = api.sim3_job_state(dict(spr, **carried), n_it, sc.draws(4, 30, H_max - 1))
            assert E.emu_sim3_check_job(api.sim3_jobs([ss]), C.byref(Hd), C.byref(Hr)) == -1


def test_draw_range_and_best_mask_rules(E):
    E.emu_check_draws.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    E.emu_check_best_mask.argtypes = [C.c_void_p, C.c_int, C.c_int]
    for K in (3, 4, 8):
        N = 12
        good = np.array([[N - 1 - k for k in range(K)], [0] * K], np.int32)
        assert E.emu_check_draws(p(good), good.size, 2, K, N) == 0
        assert E.emu_check_draws(p(good), good.size - 1, 2, K, N) == -1                    # fewer than K * H
        assert E.emu_check_draws(None, good.size, 2, K, N) == -1
        assert E.emu_check_draws(None, 0, 0, K, N) == 0                                    # no hypothesis, no draws
        for k in range(K):
            bad = good.copy(); bad[1, k] = N - k
            assert E.emu_check_draws(p(bad), bad.size, 2, K, N) == -1, (K, k)
            assert E.emu_check_draws(p(bad), bad.size, 1, K, N) == 0                       # the row is beyond H
            bad = good.copy(); bad[0, k] = -1
            assert E.emu_check_draws(p(bad), bad.size, 2, K, N) == -1
    m = np.array([0, 3, 0, 255, 1], np.uint8)
    assert E.emu_check_best_mask(p(m), 5, 3) == 0 and E.emu_check_best_mask(p(m), 5, 2) == -1 and E.emu_check_best_mask(p(m), 3, 1) == 0
    assert E.emu_check_best_mask(None, 0, 0) == 0 and E.emu_check_best_mask(None, 0, 1) == -1


def pack(E, m):
    words = np.zeros((len(m) + 63) // 64 + 1, np.uint64)
    words[-1] = 0x7777777777777777
    E.emu_mask_pack(p(m) if len(m) else None, len(m), p(words))
    assert words[-1] == 0x7777777777777777
    return words[:-1]


def test_mask_round_trip(E):
    for m in mask_rows():
        N = len(m)
        words = pack(E, m)
        for i in range(64 * len(words)):
            assert int(words[i >> 6] >> np.uint64(i & 63)) & 1 == (1 if i < N and m[i] else 0), (N, i)
        back = np.full(N + 16, 7, np.uint8)
        E.emu_mask_unpack(p(words) if N else None, N, p(back))
        assert np.array_equal(back[:N], (m != 0).astype(np.uint8)) and (back[N:] == 7).all()
    # packing ORs: a second mask into the same words adds its bits
    a = np.zeros(65, np.uint8); a[[0, 64]] = 1
    b = np.zeros(65, np.uint8); b[[1, 63]] = 1
    words = pack(E, a)
    E.emu_mask_pack(p(b), 65, p(words))
    assert [int(w) for w in words] == [(1 << 63) | 3, 1]


def test_iteration_count(E):
    for prob, eps, pinned in iteration_rows():
        got = E.emu_iterations(prob, float(eps))
        assert got == literal_iterations(prob, eps), (prob, eps)
        if pinned is not None:
            assert got == pinned, (prob, eps)
    # the two entries are this count between 1 and maxIterations
    assert api.ransac_parameters(20, 0.99, 10, 300, 4, 0.5)[1] == E.emu_iterations(0.99, 0.5) == api.sim3_ransac_parameters(40, 0.99, 20, 300)
    assert api.ransac_parameters(200, 0.99, 10, 5000, 4, 0.1)[1] == E.emu_iterations(0.99, float(np.float32(0.1)))
    assert math.ceil(math.log(0.01) / math.log(1 - float(np.float32(0.1)) ** 3)) == 4603


# ---------------------------------------------------------------------------------------------------------------- the stand-alone program

def test_stand_alone_program_under_the_host_sanitizers(tmp_path, E):
    """-DRANSAC_EMU_MAIN: a program with its own main, built with -fsanitize=address,undefined and run on the cases above; every buffer of it has
    exactly the size the helper may touch.  Nothing of it is loaded into this process."""
    exe = tmp_path / "ransac_common_emu"
    subprocess.check_call(GPP + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                                 "-DRANSAC_EMU_MAIN", EMU, "-o", str(exe)])
    blob, want = [], []
    for K, N, row in draw_rows():
        blob.append(struct.pack("<iii%di" % K, 0, K, N, *row))
        want.append("r " + " ".join(str(v) for v in SWAP_AND_POP[K](N, row)))
    for row, (H_max, H_min) in hypothesis_rows():
        blob.append(struct.pack("<i5i", 1, *row))
        want.append("h %d %d" % (H_max, H_min))
    for m in mask_rows():
        blob.append(struct.pack("<ii", 2, len(m)) + m.tobytes())
        want.append(" ".join(["m %d %d" % (len(m), int((m != 0).sum()))] + ["%x" % int(w) for w in pack(E, m)]))
    for prob, eps, _ in iteration_rows():
        blob.append(struct.pack("<idf", 3, prob, float(eps)))
        want.append("i %d" % literal_iterations(prob, eps))
    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<i", len(blob)) + b"".join(blob))
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "ERROR" not in r.stderr, r.stderr[-2000:]
    assert r.stdout.splitlines() == want
