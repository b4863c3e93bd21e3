"""The two references of the pose-only optimisation against each other on the inputs of the GPU parity matrix (tests/pose_cases.py): the C++
oracle (oracle/orc_ba.cpp) and the numpy restatement (tests/npref_pose.py).  The GPU matrix compares the device with the oracle alone; here
every family's expected answer is pinned a second time by a program that shares no code with it: outlier flags, inlier count and the
iteration count of every round identical, pose within 1e-9 absolute (the bar of test_pose_optimisation_against_a_numpy_restatement)."""
import numpy as np
import pytest
import orc
import npref_pose
import pose_cases as pc


def _agree(name, pr):
    n_w, pose_w, out_w, its_w = npref_pose.pose_optimize(pr)
    n_g, pose_g, out_g, st = orc.pose_optimize(pr)
    its_g = [st.iterations_done[i] for i in range(st.rounds)]
    assert n_g == n_w and np.array_equal(out_g, out_w), (name, n_g, n_w, int((out_g != out_w).sum()))
    assert its_g == its_w, (name, its_g, its_w)
    assert all(st.iterations_done[i] == 0 for i in range(st.rounds, 4)), name
    assert n_g == len(out_g) - st.n_bad if st.rounds else n_g == 0, name
    d = float(np.abs(pose_g - pose_w).max())
    assert np.isfinite(pose_g).all() and d <= 1e-9, (name, d)
    return n_g, its_g, pose_g, d


@pytest.mark.parametrize("fam", [f for f in pc.FAMILIES if f != "random"])
def test_references_agree_on_the_named_cases(fam):
    cases = [(n, p) for n, p in pc.family(fam) if len(p["Xw"]) <= 300]
    assert cases
    worst = 0.0
    for name, pr in cases:
        n_in, its, pose, d = _agree(fam + ": " + name, pr)
        worst = max(worst, d)
        N = len(pr["Xw"])
        if N < 3:                        # Optimizer.cpp:131-132
            assert n_in == 0 and its == [] and np.array_equal(pose, pr["pose0"]), name
        else:
            assert len(its) == (1 if N < 10 else 4), (name, its)
    print("%s: %d cases, worst pose distance between the references %.2e" % (fam, len(cases), worst))


def test_references_agree_on_the_branches_the_cases_were_built_for():
    """the cases that exist to reach one branch do reach it, in both references"""
    deg = dict(pc.degenerate()); st = dict(pc.starts())
    # the linear solve fails in every trial: ten rejected zero steps, one iteration per round, the (normalised) start pose comes back
    pr = deg["information all zero"]
    n_in, its, pose, _ = _agree("information all zero", pr)
    assert n_in == len(pr["Xw"]) and its == [1, 1, 1, 1]
    assert np.array_equal(pose[:3], pr["pose0"][:3]) and np.abs(pose - pc.normalized_start(pr)).max() <= 4 * np.finfo(np.float64).eps
    # 90 degrees / 2 m: after the first round every edge is an outlier, the other rounds have no active edge and do not iterate
    n_in, its, pose, _ = _agree("90 degrees", st["rot=90 deg, trans=2"])
    assert n_in == 0 and its[0] >= 1 and its[1:] == [0, 0, 0]
    # start at the optimum: the update is tiny, every exponential map takes the small-angle branch (|omega| < 1e-5)
    pr = st["exact observations, start at the optimum"]
    n_in, its, pose, _ = _agree("start at the optimum", pr)
    assert n_in == len(pr["Xw"]) and np.linalg.norm(pose - pc.normalized_start(pr)) < 1e-6
    # the sign of the returned quaternion: w >= 0 for a negated start, and the same rotation as for the start as it was
    _, _, pose_n, _ = _agree("negated", deg["start quaternion negated"])
    pr = dict(deg["start quaternion negated"]); pr["pose0"] = pr["pose0"].copy(); pr["pose0"][3:] *= -1.0
    _, _, pose_p, _ = _agree("not negated", pr)
    assert pose_n[6] > 0 and np.array_equal(pose_n, pose_p)
    # a start quaternion of length 1.7 is the unit one
    pr = dict(deg["start quaternion x 1.7"]); pr["pose0"] = pr["pose0"].copy(); pr["pose0"][3:] /= 1.7
    _, _, pose_a, _ = _agree("x 1.7", deg["start quaternion x 1.7"])
    _, _, pose_b, _ = _agree("x 1.0", pr)
    assert np.abs(pose_a - pose_b).max() <= 1e-12
    # four different intrinsics, observations re-projected with them: most edges are inliers
    cam = dict(pc.cameras())["fx=300 fy=250 cx=270 cy=281.5"]
    n_in, _, _, _ = _agree("skewed camera", cam)
    assert len({cam["fx"], cam["fy"], cam["cx"], cam["cy"]}) == 4 and n_in > 0.75 * len(cam["Xw"])


def test_references_agree_on_the_random_draw():
    cases = [(n, p) for n, p in pc.random() if len(p["Xw"]) <= 150][:60]
    assert len(cases) == 60
    worst = 0.0
    for name, pr in cases:
        worst = max(worst, _agree(name, pr)[3])
    print("random: 60 cases, worst pose distance between the references %.2e" % worst)


def test_the_generator_is_deterministic_and_leaves_synth_alone():
    from cubemapslam_amd import synth
    a = [p for f in pc.FAMILIES if f != "random" for p in pc.family(f)] + pc.random(12)
    b = [p for f in pc.FAMILIES if f != "random" for p in pc.family(f)] + pc.random(12)
    assert [n for n, _ in a] == [n for n, _ in b] and len({n for n, _ in a}) == len(a)
    for (_, p), (_, q) in zip(a, b):
        assert all(np.array_equal(p[k], q[k]) for k in ("Xw", "obs", "invsig2", "face", "pose0"))
        assert all(np.isfinite(np.asarray(p[k], np.float64)).all() for k in ("Xw", "obs", "invsig2", "pose0"))
        assert p["face"].dtype == np.int8 and p["face"].min(initial=0) >= 0 and p["face"].max(initial=0) <= 4
    assert [len(p["Xw"]) for _, p in pc.sizes()] == [0, 1, 2, 3, 4, 9, 10, 11, 63, 64, 65, 255, 256, 257, 511, 513, 1023, 1024, 1025, 2047, 2048, 4000]
    d = synth.pose_problem(N=40, seed=4)
    assert d["fx"] == d["fy"] == d["cx"] == d["cy"] == 275.0
