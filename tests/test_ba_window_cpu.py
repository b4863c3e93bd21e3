"""The host build of the local-BA-window core (csrc/cms_ba_window_core.h, hm_ba_window_*) against tests/npref_ba_window.py, the restatement of
Optimizer.cpp:194-357 with objects and marks, exactly: integers and doubles with array_equal (widening is exact, and the quaternion and in-face
arithmetic is the same IEEE operation sequence in numpy)."""
import numpy as np
import pytest

import ba_window_cases as bc
import ba_window_hostlib as bh
import covis_hostlib
import npref_ba_window


def want(c, jobs=None):
    return npref_ba_window.windows(c, bc.F, bh.cos_fov(), bc.INV_SIGMA2, jobs)


@pytest.mark.parametrize("name", bc.NAMES)
def test_host_core_equals_the_restatement(name):
    c = bc.case(name)
    rc, got = bh.host_windows(c)
    assert rc == 0
    w = want(c)
    assert bc.difference(w, got) is None, bc.difference(w, got)
    for j, g in enumerate(got):
        K, nl, P, E = (int(v) for v in g["counts"])
        assert nl == len(c["jobs"][j][0]) and (g["e_pose"] < K).all() and (g["e_point"] < P).all()
        assert np.array_equal(g["e_point"], np.sort(g["e_point"]))


def test_the_cases_hold_what_they_are_for():
    t = bh.host_windows(bc.case("tiny"))[1][0]
    assert t["counts"].tolist()[:3] == [1, 1, 5]
    f = bh.host_windows(bc.case("fixed_order"))[1][0]
    assert f["kf_member"].tolist() == bc.FIXED_ORDER_KF and f["kf_member"].tolist()[2:] != sorted(f["kf_member"].tolist()[2:])
    assert f["point_id"].tolist() == [10, 11, 12, 13, 14, 15]
    fm = bh.host_windows(bc.case("first_member"))[1]
    assert [w["fixed"].tolist() for w in fm] == [[0, 1, 1, 1, 1, 1, 1], [0, 0, 1, 1, 1, 1, 1], [0, 0, 1, 1, 1, 1, 1], [0, 0, 1, 1, 1, 1, 1]]
    fl = bh.host_windows(bc.case("filters"))[1]
    assert fl[1]["counts"].tolist() == [1, 1, 0, 0]
    p20 = fl[0]["point_id"].tolist().index(20)
    assert p20 not in fl[0]["e_point"].tolist() and len(set(fl[0]["e_point"].tolist())) == len(fl[0]["point_id"]) - 1
    n_obs = sum(int((m["mp"] == i).sum()) for i in fl[0]["point_id"] for m in bc.case("filters")["members"])
    assert n_obs - int(fl[0]["counts"][3]) == 4      # two by the ray test, two by the unknown face
    wv = bh.host_windows(bc.case("waves"))[1][0]
    assert wv["counts"][2] > 1024 and wv["counts"][3] > 1024 and wv["counts"][0] > 25
    assert set(wv["e_face"].tolist()) == {0, 1, 2, 3, 4}
    mm = bh.host_windows(bc.case("many_members"))[1][0]
    assert mm["counts"][0] > 40 and (mm["kf_member"][40:] > 1024).any()
    for name in ("waves", "many_members"):
        c = bc.case(name)
        assert max(int(m["mp"].max()) for m in c["members"]) == c["max_points"] - 1
    # every branch of the quaternion: the trace positive, and each diagonal element the largest
    q = np.concatenate([w["poses"][:, 3:] for w in (wv, mm)])
    assert all((np.abs(q).argmax(axis=1) == k).any() for k in range(4))


@pytest.mark.parametrize("name", bc.NAMES)
def test_point_ids_are_the_local_points_of_the_same_list(name):
    c = bc.case(name)
    hb = covis_hostlib.HostBackend(c["K"], c["maxf"])
    for s, m in zip(c["slots"], c["members"]):
        hb.put(s, m["mp"], m["oct"])
    hb.build(c["slots"])
    lists = [j[0] for j in c["jobs"]]
    rc, n_out, ids = hb.local_points(lists, c["caps"][1])
    hb.close()
    got = bh.host_windows(c)[1]
    assert rc == 0 and [g["point_id"].tolist() for g in got] == [list(i) for i in ids] and [int(g["counts"][2]) for g in got] == [int(n) for n in n_out]


def test_refusals_write_nothing():
    c = bc.case("fixed_order")
    hw = bh.HostWindows(c)
    from cubemapslam_amd import api
    for jobs, caps, word in (([([], -1)], c["caps"], "local"), ([([2, 8], -1)], c["caps"], "no member"), ([([2, -1], -1)], c["caps"], "no member"),
                             ([([2, 5, 2], -1)], c["caps"], "twice"), ([([2, 5], 8)], c["caps"], "first_member"), ([([2, 5], -2)], c["caps"], "first_member"),
                             ([([2, 5], -1)], (0, 8, 32), "cap"), ([([2, 5], -1)], (8, 0, 32), "cap"), ([([2, 5], -1)], (8, 8, 0), "cap")):
        o = api.ba_window_arrays(len(jobs), *[max(v, 1) for v in caps], fill=0xAB)
        with pytest.raises(bh.Refused, match=word):
            hw.run(jobs, caps, out=o)
        assert all((o[k].view(np.uint8) == 0xAB).all() for k in ("counts",) + api.BA_WINDOW_ARRAYS)
    hw.close()
    # a local point whose row holds no position: the job is named
    keep = c["pos_ids"] != 14
    hw = bh.HostWindows(c, pos_ids=c["pos_ids"][keep], pos=c["pos"][keep])
    o = api.ba_window_arrays(2, *c["caps"], fill=0xAB)
    with pytest.raises(bh.Refused, match="job 1"):
        hw.run([([7], -1), ([2, 5], -1)], c["caps"], out=o)
    assert all((o[k].view(np.uint8) == 0xAB).all() for k in ("counts",) + api.BA_WINDOW_ARRAYS)
    hw.close()


@pytest.mark.parametrize("which", (0, 1, 2))
def test_overflow_delivers_counts_and_stays_inside_the_caps(which):
    from cubemapslam_amd import api
    c = bc.case("filters")
    full = bh.host_windows(c)[1]
    caps = list(c["caps"])
    caps[which] = [int(full[0]["counts"][0]) - 1, int(full[0]["counts"][2]) - 1, int(full[0]["counts"][3]) - 1][which]
    hw = bh.HostWindows(c)
    o = api.ba_window_arrays(len(c["jobs"]) + 1, *caps, fill=0xAB)      # one row more than jobs: the guard behind the last job
    rc, got, _ = hw.run(c["jobs"], caps, out=o)
    hw.close()
    assert rc == -4 and [g["counts"].tolist() for g in got] == [f["counts"].tolist() for f in full]
    assert bc.difference([full[1]], [got[1]]) is None      # a job that fits is complete
    for j, g in enumerate(got):
        for k, n in (("kf_member", 0), ("poses", 0), ("fixed", 0), ("point_id", 2), ("points", 2), ("e_pose", 3), ("e_point", 3), ("e_obs", 3), ("e_invsig2", 3), ("e_face", 3),
                     ("e_feat", 3)):
            kept = min(int(g["counts"][n]), o[k].shape[1])
            assert np.array_equal(o[k][j, :kept], full[j][k][:kept]) and (o[k][j, kept:].view(np.uint8) == 0xAB).all(), (j, k)
    assert all((o[k][len(c["jobs"])].view(np.uint8) == 0xAB).all() for k in api.BA_WINDOW_ARRAYS)


@pytest.mark.parametrize("name", ("fixed_order", "filters", "waves"))
def test_mirror_host_core_engine(name):
    """MapPointStore::LocalBAWindow (host/cubemap_hot_path.h) through its HOST_CORE engine: the first job of the case, the key frame of mnId 0 where the job says"""
    c = bc.case(name)
    local, first = c["jobs"][0] if name != "filters" else c["jobs"][2]
    mn = np.arange(1, len(c["members"]) + 1)
    if first >= 0:
        mn[first] = 0
    got = bh.mirror(1, c, local, mn_ids=mn)
    w = want(c, [(local, first)])
    assert bc.difference(w, [got]) is None, bc.difference(w, [got])


def test_core_under_the_sanitizers(tmp_path):
    """the host core in a stand-alone program built with -fsanitize=address,undefined: waves and many_members with output arrays of exactly the caps, and
    with every cap one below the largest count"""
    import os
    import subprocess
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu", "ba_window_core_emu.cpp")
    exe = str(tmp_path / "ba_window_core_emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe])
    names = ("waves", "many_members", "filters")
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        for name in names:
            c = bc.case(name)
            f.write(bc.to_text(c, bh.cos_fov(), [w["counts"] for w in bh.host_windows(c)[1]]))
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "ba_window_core_emu: ok (%d cases)" % len(names) in r.stdout and "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-4000:]
