"""k_project_keyframe's arithmetic without a GPU: the kernel and the __device__ helpers it shares with k_in_frustum are taken from
cubemapslam_amd/csrc/cms_track_kernels.hip as they stand (the text between its host-emulation markers), compiled for the host (tests/emu/project_keyframe_emu_*.h supply the intrinsics and a driver
that runs the threads one after the other) and compared bit for bit with tests/npref_reloc.py: windows, levels, gathered angles, both distance-bounds
modes, resident and stand-alone angle sources."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import npref_reloc
import reloc_cases
from cubemapslam_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
p = lambda a: a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    s = open(os.path.join(ROOT, "cubemapslam_amd", "csrc", "cms_track_kernels.hip")).read()

    def cut(name):
        a, b = "// [host-emulation begin: %s]" % name, "// [host-emulation end: %s]" % name
        assert s.count(a) == 1 and s.count(b) == 1, name
        return s[s.index(a):s.index(b)]
    parts = [cut("bounds helpers"), cut("k_project_keyframe")]
    emu = os.path.join(ROOT, "tests", "emu")
    d = tmp_path_factory.mktemp("emu")
    src = d / "project_keyframe_emu.cpp"
    src.write_text(open(os.path.join(emu, "project_keyframe_emu_head.h")).read() + "\n".join(parts) + open(os.path.join(emu, "project_keyframe_emu_tail.h")).read())
    so = d / "project_keyframe_emu.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "cubemapslam_amd", "csrc"), str(src), "-o", str(so)])
    lib = C.CDLL(str(so))
    lib.emu_project.argtypes = [C.c_int] + [C.c_void_p] * 10 + [C.c_float] * 3 + [C.c_int] * 3 + [C.c_void_p] * 9
    return lib


def check(L, c, mode, resident):
    n=len(c['pos']); F=c['camd']['face']
    cf=npref_reloc.cos_fov_th(c['camd']); ls=npref_reloc.logf(np.float32(1.2))
    mn,mx=(c['min_dist'],c['max_dist']) if mode==0 else ((np.float32(0.8)*c['min_dist']).astype(np.float32),(np.float32(1.2)*c['max_dist']).astype(np.float32))
    ptjob=np.ones(n,np.int32); pose=np.concatenate([np.zeros(12,np.float32),c['pose12']]).astype(np.float32)
    jf=np.array([9,3],np.int32)
    if resident:
        nk=3*n; feat=np.sort(np.random.default_rng(1).choice(nk,n,replace=False)).astype(np.int32)
        kp=np.zeros(nk+50,api.KP_DTYPE); kp['angle'][50+feat]=c['kf_angle']; jk=np.array([-1,50],np.int32); ang_in=np.zeros(n,np.float32)
    else:
        kp=np.zeros(1,api.KP_DTYPE); feat=np.zeros(n,np.int32); jk=np.array([0,-1],np.int32); ang_in=c['kf_angle']
    o=dict(qf=np.zeros(n,np.int32),qx=np.zeros(n,np.float32),qy=np.zeros(n,np.float32),qr=np.zeros(n,np.float32),qmin=np.zeros(n,np.int32),qmax=np.zeros(n,np.int32),ang=np.zeros(n,np.float32),lvl=np.zeros(n,np.int32))
    pos=np.ascontiguousarray(c['pos'],np.float32)
    L.emu_project(n,p(ptjob),p(pose),p(jf),p(jk),p(kp),p(feat),p(ang_in),p(pos),p(mn),p(mx),c['th'],float(cf),float(ls),8,F,mode,p(c['sf']),
                  p(o['qf']),p(o['qx']),p(o['qy']),p(o['qr']),p(o['qmin']),p(o['qmax']),p(o['ang']),p(o['lvl']))
    pr=npref_reloc.project(F,cf,c['pose12'],c['pos'],c['min_dist'],c['max_dist'],1.2,8)
    live=pr['drop']==0
    assert np.array_equal(o['qr']>=0, live), (mode, (o['qr']>=0).sum(), live.sum())
    assert np.array_equal(o['lvl'][live], pr['level'][live]) and (o['lvl'][~live]==-1).all()
    assert np.array_equal(o['qx'][live].view(np.uint32), pr['u'][live].view(np.uint32)) and np.array_equal(o['qy'][live].view(np.uint32), pr['v'][live].view(np.uint32))
    want_r=(np.float32(c['th'])*c['sf'][pr['level'][live]]).astype(np.float32)
    assert np.array_equal(o['qr'][live], want_r)
    assert np.array_equal(o['qmin'],o['lvl']-1) and np.array_equal(o['qmax'],o['lvl']+1)
    assert np.array_equal(o['ang'], c['kf_angle']) and (o['qf']==3).all()
    return live.sum()


def test_emulated_kernel_equals_restatement(L):
    inp, kf, feat = reloc_cases.keyframe_input(seed=31)
    big, _, _ = reloc_cases.keyframe_input(seed=32, n_pts=4400, with_mp=0.75)
    rng = np.random.default_rng(5)
    total = 0
    for c in (inp, dict(inp, pose12=reloc_cases.perturbed(inp["pose12"], rng)), big, reloc_cases.edge_input(), reloc_cases.cluster_input(), dict(inp, th=3.0)):
        for mode in (0, 1):
            for resident in (False, True):
                total += check(L, c, mode, resident)
    assert total > 5000, total


def test_emulated_kernel_on_the_hand_built_cases(L):
    for name, case, m, n, k in reloc_cases.hand_cases():
        for mode in (0, 1):
            check(L, case, mode, False)
