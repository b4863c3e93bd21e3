"""The window query's second launch derives CSR offsets per tile of queries: the partial sums in front of the tile (one per search
workgroup), a scan of the tile's counts handed from wavefront to wavefront, and a guard against the candidate array's capacity.  That
arithmetic lives in cubemapslam_amd/csrc/cms_area_offsets.h; tests/emu/area_offsets_emu.cpp replays it on the host, thread by thread,
and here it must equal np.cumsum of the oracle's candidate counts."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import orc
import test_area_emu as te
from cubemapslam_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GUARD = 64


@functools.lru_cache(maxsize=None)
def _emu():
    so = os.path.join(HERE, "emu", "libarea_offsets_emu.so")
    src = os.path.join(HERE, "emu", "area_offsets_emu.cpp")
    hdr = os.path.join(ROOT, "cubemapslam_amd", "csrc", "cms_area_offsets.h")
    if not os.path.exists(so) or max(os.path.getmtime(src), os.path.getmtime(hdr)) > os.path.getmtime(so):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", src, "-o", so])
    L = C.CDLL(so)
    L.area_offsets_emu.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.area_offsets_consts.argtypes = [C.c_void_p]
    return L


def _consts():
    c = np.zeros(5, np.int32)
    _emu().area_offsets_consts(c.ctypes.data_as(C.c_void_p))
    return dict(wg_q=int(c[0]), tile=int(c[1]), threads=int(c[2]), per_thread=int(c[3]), tile_parts=int(c[4]))


@functools.lru_cache(maxsize=None)
def _oracle_counts():
    """candidates per window of 40 000 queries on a dense F = 150 frame, by the oracle (0 ... a few hundred per window)"""
    F = 150
    cam = orc.make_camera(synth.camera("lafida", F))
    kx, ky, ko = te._keypoints(F, 2000, 22)
    qx, qy, qr, lo, hi, _ = te._queries(F, 40000, 52)
    off, _ = orc.features_in_area(cam, kx, ky, ko, qx, qy, qr, lo, hi, cap=2 * 10**6)
    cnt = np.diff(off).astype(np.int32)
    assert (cnt == 0).any() and (cnt > 64).any()
    return cnt


def _replay(cnt, cap):
    nq = len(cnt)
    cnt = np.ascontiguousarray(cnt, np.int32)
    off = np.full(nq + 1, -777, np.int32)
    written = np.zeros(max(cap, 0) + GUARD, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    tot = _emu().area_offsets_emu(nq, p(cnt), p(off), cap, p(written), len(written))
    return tot, off, written


def _sizes():
    tile = _consts()["tile"]
    return [1, 31, 32, 33, tile - 1, tile, tile + 1, 2 * tile + 1, 40000]


def test_layout_constants_fit_together():
    c = _consts()
    assert c["tile"] == c["threads"] * c["per_thread"] and c["threads"] <= 256 and c["threads"] % 64 == 0
    assert c["tile"] % c["wg_q"] == 0 and c["tile_parts"] == c["tile"] // c["wg_q"]      # a tile starts on a search-workgroup boundary
    assert c["tile_parts"] % 4 == 0                                                        # the partial sums in front are read four at a time
    assert 40000 > 32 * c["tile"]                                                          # the largest size spans more than 32 tiles


@pytest.mark.parametrize("which", range(9))
def test_offsets_equal_cumsum_of_oracle_counts(which):
    nq = _sizes()[which]
    cnt = _oracle_counts()[:nq]
    want = np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)])
    total = int(want[-1])
    tot, off, written = _replay(cnt, cap=total)
    assert tot == total, (nq, tot, total)
    assert np.array_equal(off, want), nq
    assert (written[:total] == 1).all() and (written[total:] == 0).all()      # every list position stored exactly once


@pytest.mark.parametrize("which", range(9))
def test_capacity_guard(which):
    nq = _sizes()[which]
    cnt = _oracle_counts()[:nq]
    want = np.concatenate([[0], np.cumsum(cnt, dtype=np.int64)])
    total = int(want[-1])
    for cap in sorted({0, total // 2, max(total - 1, 0)}):
        tot, off, written = _replay(cnt, cap=cap)
        assert tot == total and np.array_equal(off, want), (nq, cap)          # offsets and total do not depend on the capacity
        n = min(cap, total)
        assert (written[:n] == 1).all() and (written[n:] == 0).all(), (nq, cap)
