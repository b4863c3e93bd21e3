"""Reference for the one-stage (global) bundle adjustment: SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg and the
Schur complement of BlockSolver_6_3, restated in numpy from optimize() of oracle/orc_ba.cpp (:313-379) over the oracle's own linearisation
(orc.ba_linearize) and pose update (orc_se3_exp_apply).  The oracle has no entry without the robust kernel and none without the
classification between its two stages; with the kernel, orc.ba_run(prob, its=(N, 0)) is the same optimisation and
tests/test_global_ba_cpu.py holds this file to it.  Optimizer::BundleAdjustment writes the kernel's width as sqrt(5.99) (Optimizer.cpp:497)
where LocalBundleAdjustment -- and with it the oracle -- writes sqrt(5.991) (:300): `delta` is an argument."""
import ctypes as C

import numpy as np

import orc

DELTA_LOCAL = float(np.sqrt(5.991))      # Optimizer.cpp:300, the oracle's
DELTA_GLOBAL = float(np.sqrt(5.99))      # Optimizer.cpp:497


def _normalised(poses):
    p = np.array(poses, np.float64, copy=True)
    q = p[:, 3:] / np.linalg.norm(p[:, 3:], axis=1, keepdims=True)
    p[:, 3:] = np.where(q[:, 3:4] < 0, -q, q)      # the SE3Quat constructor (se3quat.h:58-64)
    return p


def _exp_apply(upd6, pose7):
    f = orc.lib().orc_se3_exp_apply
    f.argtypes = [C.c_void_p, C.c_void_p]
    f.restype = None
    u = np.ascontiguousarray(upd6, np.float64)
    f(u.ctypes.data_as(C.c_void_p), pose7.ctypes.data_as(C.c_void_p))


class _Structure:
    """what does not change over the optimisation: the free poses' slots, the active points, the co-observing edge pairs of every point"""

    def __init__(self, prob):
        K, P = len(prob["poses"]), len(prob["points"])
        ep = np.asarray(prob["e_pose"], np.int64); el = np.asarray(prob["e_point"], np.int64)
        fixed = np.asarray(prob["fixed"]).astype(bool)
        pose_act = np.zeros(K, bool); pose_act[ep] = True
        self.pt_act = np.zeros(P, bool); self.pt_act[el] = True
        self.free = np.nonzero(pose_act & ~fixed)[0]
        self.slot = np.full(K, -1, np.int64); self.slot[self.free] = np.arange(len(self.free))
        self.np_ = len(self.free)
        self.e_slot = self.slot[ep]
        self.e_point = el
        # edge pairs (a1, a2) of one point, both poses free, in the point's edge order
        order = np.argsort(el, kind="stable")
        cnt = np.bincount(el, minlength=P)
        start = np.concatenate([[0], np.cumsum(cnt)])[:-1]
        a1, a2 = [], []
        for m in np.unique(cnt[cnt > 0]):
            pts = np.nonzero(cnt == m)[0]
            idx = order[start[pts][:, None] + np.arange(m)[None, :]]      # points x m edges
            a1.append(np.repeat(idx, m, axis=1).ravel()); a2.append(np.tile(idx, (1, m)).ravel())
        a1 = np.concatenate(a1) if a1 else np.zeros(0, np.int64); a2 = np.concatenate(a2) if a2 else np.zeros(0, np.int64)
        keep = (self.e_slot[a1] >= 0) & (self.e_slot[a2] >= 0)
        self.a1, self.a2 = a1[keep], a2[keep]


def reduced_system(lin, S, lam):
    """(H, b, Dinv): the reduced camera system of schur_solve (orc_ba.cpp) at lambda, dense, n = 6 x free poses"""
    n = 6 * S.np_
    Dinv = np.zeros_like(lin["Hll"])
    act = S.pt_act
    Dinv[act] = np.linalg.inv(lin["Hll"][act] + lam * np.eye(3)[None])
    H = np.zeros((S.np_, 6, S.np_, 6))
    Hpp = lin["Hpp"][S.free]
    ar = np.arange(S.np_)
    H[ar, :, ar, :] = Hpp + lam * np.eye(6)[None]
    b = lin["bp"][S.free].copy()
    Y = np.einsum("eij,ejk->eik", lin["Hpl"], Dinv[S.e_point])      # B D^-1, per edge
    blocks = np.einsum("eik,ejk->eij", Y[S.a1], lin["Hpl"][S.a2])
    np.subtract.at(H, (S.e_slot[S.a1], slice(None), S.e_slot[S.a2], slice(None)), blocks)
    fe = np.nonzero(S.e_slot >= 0)[0]
    np.subtract.at(b, S.e_slot[fe], np.einsum("eik,ek->ei", Y[fe], lin["bl"][S.e_point[fe]]))
    return H.reshape(n, n), b.reshape(n), Dinv


def _solve(lin, S, lam):
    """schur_solve: (ok, x_poses[np, 6], x_points[P, 3])"""
    H, b, Dinv = reduced_system(lin, S, lam)
    P = len(lin["bl"])
    xp = np.zeros((S.np_, 6))
    ok = True
    if S.np_ > 0:
        try:
            xp = np.linalg.solve(H, b).reshape(S.np_, 6)
        except np.linalg.LinAlgError:
            ok = False
        if not np.all(np.isfinite(xp)):
            ok = False
        if not ok:
            return False, np.zeros((S.np_, 6)), np.zeros((P, 3))
    cl = lin["bl"].copy()
    fe = np.nonzero(S.e_slot >= 0)[0]
    np.subtract.at(cl, S.e_point[fe], np.einsum("eij,ei->ej", lin["Hpl"][fe], xp[S.e_slot[fe]]))
    xl = np.einsum("pij,pj->pi", Dinv, cl)
    return True, xp, xl


def first_system(prob, robust, delta=DELTA_GLOBAL):
    """the reduced system of the first Levenberg trial (lambda0 = 1e-5 max diag): (H, b, lambda0)"""
    p = dict(prob); p["poses"] = _normalised(prob["poses"])
    S = _Structure(prob)
    lin = orc.ba_linearize(p, robust=robust, delta=delta)
    lam = 1e-5 * _max_diag(lin, S)
    H, b, _ = reduced_system(lin, S, lam)
    return H, b, lam


def _max_diag(lin, S):
    m = 0.0
    if S.np_:
        m = max(m, float(np.abs(np.diagonal(lin["Hpp"][S.free], axis1=1, axis2=2)).max()))
    if S.pt_act.any():
        m = max(m, float(np.abs(np.diagonal(lin["Hll"][S.pt_act], axis1=1, axis2=2)).max()))
    return m


def run(prob, iterations, robust, delta=DELTA_GLOBAL):
    """-> dict(poses, points, iterations_done, chi2_initial, chi2_final, lambda_final, trials)"""
    S = _Structure(prob)
    cur = dict(prob)
    cur["poses"] = _normalised(prob["poses"]); cur["points"] = np.array(prob["points"], np.float64, copy=True)
    out = dict(iterations_done=0, chi2_initial=0.0, chi2_final=0.0, lambda_final=0.0, trials=0)
    if S.np_ + int(S.pt_act.sum()) == 0:
        out["iterations_done"] = -1
        out.update(poses=cur["poses"], points=cur["points"])
        return out
    lam, ni, n_bad, done = -1.0, 2.0, 0, 0
    for it in range(iterations):
        lin = orc.ba_linearize(cur, robust=robust, delta=delta)
        current = float(lin["chi"][0])
        ini = current
        if it == 0:
            out["chi2_initial"] = ini
            lam = 1e-5 * _max_diag(lin, S); ni = 2.0; n_bad = 0
        rho, qmax = 0.0, 0
        while True:
            ok, xp, xl = _solve(lin, S, lam)
            trial = dict(cur)
            trial["poses"] = cur["poses"].copy(); trial["points"] = cur["points"].copy()
            for s, k in enumerate(S.free):
                _exp_apply(xp[s], trial["poses"][k])
            trial["points"][S.pt_act] += xl[S.pt_act]
            temp = float(orc.ba_linearize(trial, robust=robust, delta=delta)["chi"][0])
            if not ok:
                temp = np.finfo(np.float64).max
            rho = current - temp
            scale = float((xp * (lam * xp + lin["bp"][S.free])).sum()) + float((xl[S.pt_act] * (lam * xl[S.pt_act] + lin["bl"][S.pt_act])).sum()) + 1e-3
            rho /= scale
            if rho > 0 and np.isfinite(temp):
                alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha); ni = 2.0; current = temp
                cur = trial
            else:
                lam *= ni; ni *= 2
            qmax += 1
            out["trials"] += 1
            if not (rho < 0 and qmax < 10):
                break
        done += 1
        out["chi2_final"] = current; out["lambda_final"] = lam
        if qmax == 10 or rho == 0:
            break
        n_bad = n_bad + 1 if (ini - current) * 1e3 < ini else 0
        if n_bad >= 3:
            break
    out["iterations_done"] = done
    out.update(poses=cur["poses"], points=cur["points"])
    return out
