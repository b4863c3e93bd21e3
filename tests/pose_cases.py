"""Case generator of the pose-optimisation parity matrix (tests/test_pose_cases_cpu.py, tests/test_gpu_pose_matrix.py).

Every function returns a list of (name, problem); a problem is a dict like synth.pose_problem()'s.  Everything is deterministic: the seeds
are written here, and synth.pose_problem's own random stream is left as it is (bench.py and the golden vectors draw from it).  The inputs are
finite throughout.  What each family is for:

  sizes       the thread / register-slot / kernel-variant boundaries (one edge per thread: 256; four per thread: 1024; above: the in-memory
              kernel), the reference's own limits (N < 3: nothing happens; N < 10: one round)
  starts      the start pose from "at the optimum" (every step in the small-angle branch of the exponential map) to 90 degrees / 2 m (after
              round 1 no edge is active any more: rounds 2-4 do nothing)
  cameras     the reference's other face sizes, and intrinsics that are four different numbers
  outliers    gross mismatches up to every edge, every observation off by 200 px, edges on a wrong face (negative local depth)
  degenerate  rank-deficient systems, a system that cannot be solved at all (information zero), start quaternions that are not unit / negated,
              the same map point matched twice
  random      a broad draw over size, outlier share, start error and face size
"""
import numpy as np
from cubemapslam_amd import synth

FAMILIES = ("sizes", "starts", "cameras", "outliers", "degenerate", "random")
_EDGE_KEYS = ("Xw", "obs", "invsig2", "face", "gross")


def _subset(pr, mask):
    return {k: (np.ascontiguousarray(v[mask]) if k in _EDGE_KEYS else v) for k, v in pr.items()}


def _quat_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def sizes():
    return [("N=%d" % N, synth.pose_problem(N=N, seed=100 + N, outlier_frac=0.1))
            for N in (0, 1, 2, 3, 4, 9, 10, 11, 63, 64, 65, 255, 256, 257, 511, 513, 1023, 1024, 1025, 2047, 2048, 4000)]


def exact_start(N=200, seed=61, F=550):
    """observations replaced by the exact projections at the ground truth, start AT the ground truth: the optimum is the start (the update
    is the float rounding of the observations, ~1e-8), every edge an inlier, every step inside the small-angle branch"""
    pr = synth.pose_problem(N=N, seed=seed, outlier_frac=0.0, F=F)
    pr["pose0"] = pr["pose_gt"].copy()
    Xc = pr["Xw"] @ _quat_R(pr["pose_gt"][3:]).T + pr["pose_gt"][:3]
    face, up, vp = synth.rays_to_cubemap(F, Xc)
    keep = face == pr["face"]
    pr["obs"][keep, 0] = up[keep] - np.floor(up[keep] / F) * F
    pr["obs"][keep, 1] = vp[keep] - np.floor(vp[keep] / F) * F
    return _subset(pr, keep)


def starts():
    out = [("rot=%g deg, trans=%g" % (rot, tr), synth.pose_problem(N=200, seed=31, outlier_frac=0.1, rot_deg=rot, trans=tr))
           for rot, tr in ((0.0, 0.0), (0.01, 0.001), (5.0, 0.2), (15.0, 0.5), (40.0, 1.0), (90.0, 2.0))]
    out.append(("exact observations, start at the optimum", exact_start()))
    return out


def skewed_camera(N=200, seed=42, fx=300.0, fy=250.0, cx=270.0, cy=281.5, F=550):
    """four different intrinsics; the observations are re-projected with them so that most edges stay inliers"""
    pr = synth.pose_problem(N=N, seed=seed, outlier_frac=0.1, F=F)
    h = F / 2.0
    pr["obs"] = np.ascontiguousarray(np.stack([(pr["obs"][:, 0] - h) * fx / h + cx, (pr["obs"][:, 1] - h) * fy / h + cy], 1))
    pr["obs"] = pr["obs"].astype(np.float32).astype(np.float64)         # measurements are float key points in the reference
    pr["fx"], pr["fy"], pr["cx"], pr["cy"] = fx, fy, cx, cy
    return pr


def cameras():
    out = [("F=%d" % F, synth.pose_problem(N=200, F=F, seed=41, outlier_frac=0.1)) for F in (450, 650)]
    out.append(("fx=300 fy=250 cx=270 cy=281.5", skewed_camera()))
    out.append(("nlevels=1", synth.pose_problem(N=200, seed=95, outlier_frac=0.1, nlevels=1)))
    out.append(("scale=2.0", synth.pose_problem(N=200, seed=96, outlier_frac=0.1, scale=2.0)))
    return out


def outliers():
    out = [("outlier share %g" % o, synth.pose_problem(N=200, seed=s, outlier_frac=o)) for o, s in ((0.5, 54), (0.8, 53), (1.0, 52))]
    pr = synth.pose_problem(N=200, seed=51, outlier_frac=0.0)
    pr["obs"] = pr["obs"] + 200.0
    out.append(("every observation +200 px", pr))
    pr = synth.pose_problem(N=200, seed=81, outlier_frac=0.05)
    rs = np.random.RandomState(1)
    m = rs.uniform(size=200) < 0.2
    pr["face"] = np.where(m, (pr["face"] + 1 + rs.randint(0, 4, 200)) % 5, pr["face"]).astype(np.int8)
    out.append(("20% of the edges on a wrong face", pr))
    return out


def degenerate():
    out = []
    pr = synth.pose_problem(N=200, seed=91, outlier_frac=0.0)
    for f in range(5):
        m = pr["face"] == f
        if m.sum() >= 12:
            out.append(("face %d only" % f, _subset(pr, m)))
    pr = synth.pose_problem(N=50, seed=92, outlier_frac=0.0)
    pr["Xw"][:] = pr["Xw"][0]; pr["obs"][:] = pr["obs"][0]; pr["face"][:] = pr["face"][0]
    out.append(("all edges the same point", pr))
    pr = synth.pose_problem(N=50, seed=93, outlier_frac=0.0)
    pr["invsig2"][:] = 0.0
    out.append(("information all zero", pr))
    pr = synth.pose_problem(N=200, seed=71, outlier_frac=0.1)
    pr["pose0"][3:] *= 1.7
    out.append(("start quaternion x 1.7", pr))
    pr = synth.pose_problem(N=200, seed=71, outlier_frac=0.1)
    pr["pose0"][3:] *= -1.0
    out.append(("start quaternion negated", pr))
    pr = synth.pose_problem(N=100, seed=94, outlier_frac=0.1)
    idx = np.concatenate([np.arange(100), np.random.RandomState(2).randint(0, 100, 40)])
    out.append(("100 edges + 40 of them again", _subset(pr, idx)))
    return out


def random(n=240, seed=0, sizes=(12, 30, 60, 100, 150, 257, 600, 1024)):
    """n problems: size, outlier share, start error and face size drawn independently"""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        N = int(rs.choice(sizes)); o = float(rs.choice([0.0, 0.1, 0.3, 0.5])); rot = float(rs.choice([0.01, 1.5, 5.0, 15.0]))
        tr = float(rs.choice([0.001, 0.05, 0.3])); F = int(rs.choice([450, 550, 650]))
        out.append(("#%d N=%d outliers=%g rot=%g trans=%g F=%d" % (i, N, o, rot, tr, F),
                    synth.pose_problem(N=N, seed=1000 + i, outlier_frac=o, rot_deg=rot, trans=tr, F=F)))
    return out


def family(name):
    return {"sizes": sizes, "starts": starts, "cameras": cameras, "outliers": outliers, "degenerate": degenerate, "random": random}[name]()


def normalized_start(pr):
    """the start pose as the optimiser sees it (SE3Quat constructor: w >= 0, unit quaternion): the point pose updates are measured from"""
    q = np.array(pr["pose0"][3:], np.float64)
    if q[3] < 0:
        q = -q
    return np.concatenate([pr["pose0"][:3], q / np.linalg.norm(q)])
