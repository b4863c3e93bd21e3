"""Optimizer::OptimizeEssentialGraph (src/Optimizer.cpp:623-886) restated in numpy / float64 from the reference's and g2o's text: Sim3::log
(ThirdParty/g2o/g2o/types/sim3.h:148-225) with its four branches and Eigen's 3 x 3 PartialPivLU, EdgeSim3::computeError
(types_seven_dof_expmap.h:106-114), the numeric linearizeOplus on both vertices (core/base_binary_edge.hpp:131-204), the quadratic form with identity
information and no robust kernel, and OptimizationAlgorithmLevenberg::solve with setUserLambdaInit.  A plain sequential version: one edge after the
other, a dense numpy.linalg solve of the full 7 Nf x 7 Nf system, plain sums.  g2o::Sim3's other members come from npref_sim3_opt.

log / acos / exp / sin / cos are injectable: libm's by default, the core's own through the probes for the bit-for-bit comparisons of the per-edge
quantities.  A Sim3 is (q xyzw, t, s) as in npref_sim3_opt; `to8` / `from8` convert to the job records' rows."""
import math

import numpy as np

import npref_sim3_opt as ns

f64 = np.float64
LIBM = dict(ns.LIBM, log=math.log, acos=math.acos)


def to8(S):
    return np.concatenate([np.asarray(S[0], f64), np.asarray(S[1], f64), [f64(S[2])]])


def from8(r):
    r = np.asarray(r, f64)
    return r[:4].copy(), r[4:7].copy(), f64(r[7])


def lu3_solve(W, t):
    """W.lu().solve(t): Eigen's PartialPivLU -- the first entry of largest magnitude in the column is the pivot -- then the two triangles"""
    a = np.array(W, f64); b = np.array(t, f64)
    for k in range(3):
        piv = k; best = abs(a[k, k])
        for i in range(k + 1, 3):
            if abs(a[i, k]) > best:
                best = abs(a[i, k]); piv = i
        if piv != k:
            a[[k, piv]] = a[[piv, k]]; b[[k, piv]] = b[[piv, k]]
        for i in range(k + 1, 3):
            a[i, k] = a[i, k] / a[k, k]
            for j in range(k + 1, 3):
                a[i, j] = a[i, j] - a[i, k] * a[k, j]
    b[1] = b[1] - a[1, 0] * b[0]
    b[2] = (b[2] - a[2, 0] * b[0]) - a[2, 1] * b[1]
    x = np.zeros(3)
    x[2] = b[2] / a[2, 2]
    x[1] = (b[1] - a[1, 2] * x[2]) / a[1, 1]
    x[0] = ((b[0] - a[0, 1] * x[1]) - a[0, 2] * x[2]) / a[0, 0]
    return x


def branch(S, fn=LIBM):
    """(|sigma| < eps, d > 1 - eps) of Sim3::log at S"""
    R = ns.quat_to_R(S[0])
    d = 0.5 * (((R[0, 0] + R[1, 1]) + R[2, 2]) - 1)
    return bool(abs(f64(fn["log"](float(S[2])))) < 0.00001), bool(d > 1 - 0.00001)


def sim3_log(S, fn=LIBM):
    """Sim3::log(), sim3.h:148-225"""
    q, t, s = S
    s = f64(s)
    sigma = f64(fn["log"](float(s)))
    R = ns.quat_to_R(q)
    d = 0.5 * (((R[0, 0] + R[1, 1]) + R[2, 2]) - 1)
    dR = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    eps = 0.00001
    I = np.eye(3)
    with np.errstate(all="ignore"):
        if abs(sigma) < eps:
            C = f64(1)
            if d > 1 - eps:
                omega = 0.5 * dR
                A = f64(1. / 2.); B = f64(1. / 6.)
            else:
                theta = f64(fn["acos"](float(d))); theta2 = theta * theta
                omega = theta / (2 * np.sqrt(1 - d * d)) * dR
                A = (1 - f64(fn["cos"](float(theta)))) / theta2
                B = (theta - f64(fn["sin"](float(theta)))) / (theta2 * theta)
        else:
            C = (s - 1) / sigma
            if d > 1 - eps:
                sigma2 = sigma * sigma
                omega = 0.5 * dR
                A = ((sigma - 1) * s + 1) / sigma2
                B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
            else:
                theta = f64(fn["acos"](float(d)))
                omega = theta / (2 * np.sqrt(1 - d * d)) * dR
                theta2 = theta * theta
                a = s * f64(fn["sin"](float(theta))); b = s * f64(fn["cos"](float(theta)))
                c = theta2 + sigma * sigma
                A = (a * sigma + (1 - b) * theta) / (theta * c)
                B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2
        Om = np.array([[0, -omega[2], omega[1]], [omega[2], 0, -omega[0]], [-omega[1], omega[0], 0]], f64)
        BO = B * Om
        W = np.zeros((3, 3))
        for i in range(3):
            for j in range(3):      # A*Omega + (B*Omega)*Omega + C*I
                bo2 = (BO[i, 0] * Om[0, j] + BO[i, 1] * Om[1, j]) + BO[i, 2] * Om[2, j]
                W[i, j] = (A * Om[i, j] + bo2) + C * I[i, j]
        ups = lu3_solve(W, t)
    return np.concatenate([omega, ups, [sigma]])


def measurement(Siw, Sjw):
    """Sji = Sjw * Swi"""
    return ns.sim3_times(Sjw, ns.sim3_inverse(Siw))


def edge_error(C, S0, S1, fn=LIBM):
    """EdgeSim3::computeError: log(C * v0 * v1^-1)"""
    return sim3_log(ns.sim3_times(ns.sim3_times(C, S0), ns.sim3_inverse(S1)), fn)


def numeric_jacobians(C, S0, S1, fix_scale, fn=LIBM, free=(True, True), delta=1e-9):
    """linearizeOplus of base_binary_edge.hpp: per free vertex and dimension, oplus(+delta), computeError, oplus(-delta), computeError,
    scalar * (e+ - e-).  -> [J0, J1], 7 x 7 each, None for a fixed vertex"""
    scalar = 1.0 / (2 * delta)
    out = [None, None]
    for which in (0, 1):
        if not free[which]:
            continue
        J = np.zeros((7, 7))
        for d in range(7):
            add = np.zeros(7); add[d] = delta
            Sp = ns.oplus((S0, S1)[which], add, fix_scale, fn)
            ep = edge_error(C, Sp, S1, fn) if which == 0 else edge_error(C, S0, Sp, fn)
            add = np.zeros(7); add[d] = -delta
            Sm = ns.oplus((S0, S1)[which], add, fix_scale, fn)
            em = edge_error(C, Sm, S1, fn) if which == 0 else edge_error(C, S0, Sm, fn)
            J[:, d] = scalar * (ep - em)
        out[which] = J
    return out


def envelope(N, fixed, edges):
    """first (per free vertex: its lowest free neighbour, or itself) and the set of stored blocks, from sets"""
    free = [v for v in range(N) if v != fixed]
    idx = {v: k for k, v in enumerate(free)}
    nb = {k: {k} for k in range(len(free))}
    for v0, v1, _ in edges:
        if v0 != fixed and v1 != fixed:
            nb[idx[v0]].add(idx[v1]); nb[idx[v1]].add(idx[v0])
    first = [min(nb[k]) for k in range(len(free))]
    return first, {(i, j) for i in range(len(free)) for j in range(first[i], i + 1)}


def optimize(graph, fix_scale=None, iterations=20, lambda_init=1e-16, fn=LIBM):
    """OptimizeEssentialGraph's optimisation on a graph dict (Scw, Snc: N x 8; fixed; edges: E x 3).
    -> dict(S (N x 8), chi2_initial, chi2_final, lambda_final, iterations_run, trials_run, end)"""
    fix_scale = int(graph.get("fix_scale", 0) if fix_scale is None else fix_scale)
    Scw = [from8(r) for r in graph["Scw"]]; Snc = [from8(r) for r in graph["Snc"]]
    N = len(Scw); fixed = int(graph["fixed"])
    edges = [(int(a), int(b), measurement((Snc if k else Scw)[a], (Snc if k else Scw)[b])) for a, b, k in np.asarray(graph["edges"]).reshape(-1, 3)]
    free = [v for v in range(N) if v != fixed]; idx = {v: k for k, v in enumerate(free)}; n = 7 * len(free)
    S = list(Scw)
    chi = lambda est: float(sum(float(e @ e) for e in (edge_error(C, est[i], est[j], fn) for i, j, C in edges)))
    chi0 = chi(S)
    lam = lambda_init; ni = 2.0; nBad = 0; cur = chi0; done = 0; trials = 0; end = "iterations"
    for it in range(iterations if (edges and free) else 0):
        H = np.zeros((n, n)); b = np.zeros(n); cur = 0.0
        for i, j, C in edges:
            e = edge_error(C, S[i], S[j], fn); cur += float(e @ e)
            J = numeric_jacobians(C, S[i], S[j], fix_scale, fn, free=(i != fixed, j != fixed))
            for v, Jv in ((i, J[0]), (j, J[1])):
                if Jv is not None:
                    a = 7 * idx[v]; b[a:a + 7] -= Jv.T @ e; H[a:a + 7, a:a + 7] += Jv.T @ Jv
            if J[0] is not None and J[1] is not None:
                a = 7 * idx[i]; c = 7 * idx[j]
                H[a:a + 7, c:c + 7] += J[0].T @ J[1]; H[c:c + 7, a:a + 7] += J[1].T @ J[0]
        ini = cur; q = 0
        if it == 0:
            lam = lambda_init; ni = 2.0; nBad = 0
        while True:
            try:
                x = np.linalg.solve(H + lam * np.eye(n), b); ok = bool(np.isfinite(x).all())
            except np.linalg.LinAlgError:
                ok = False
            if not ok:
                x = np.zeros(n)
            T = list(S)
            for v in free:
                T[v] = ns.oplus(S[v], x[7 * idx[v]:7 * idx[v] + 7], fix_scale, fn)      # zeroes x[6] in place under fix_scale
            tmp = chi(T) if ok else 1.7976931348623157e308
            rho = (cur - tmp) / (float(x @ (lam * x + b)) + 1e-3)
            trials += 1
            if rho > 0 and np.isfinite(tmp):
                alpha = min(1. - (2 * rho - 1) ** 3, 2. / 3.); lam *= max(1. / 3., alpha); ni = 2.0; cur = tmp; S = T
            else:
                lam *= ni; ni *= 2
            q += 1
            if not (rho < 0 and q < 10):
                break
        done += 1
        if q == 10 or rho == 0:
            end = "qmax" if q == 10 else "rho0"
            break
        nBad = nBad + 1 if (ini - cur) * 1e3 < ini else 0
        if nBad >= 3:
            end = "nbad"
            break
    return dict(S=np.stack([to8(s) for s in S]), chi2_initial=chi0, chi2_final=cur, lambda_final=lam, iterations_run=done, trials_run=trials, end=end)


def log_distance(Sa, Sb, fn=LIBM):
    """|log(Sa * Sb^-1)|inf per vertex, for N x 8 arrays"""
    return np.array([np.abs(sim3_log(ns.sim3_times(from8(a), ns.sim3_inverse(from8(b))), fn)).max() for a, b in zip(Sa, Sb)])


def pose_out(S8):
    """Tiw = [R | t / s] narrowed once (:833-852), 12 floats row major"""
    q, t, s = from8(S8)
    T = np.zeros((3, 4), np.float32)
    T[:, :3] = ns.quat_to_R(q).astype(np.float32)
    T[:, 3] = (t * (1. / s)).astype(np.float32)
    return T.ravel()


def correct_points(pos, ref, S_old, S_new):
    """correctedSwr.map(Srw.map(P)) in double, narrowed once; ref < 0: copied"""
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    out = pos.copy()
    for k in range(len(pos)):
        if ref[k] >= 0:
            y = ns.sim3_map(from8(S_old[ref[k]]), pos[k].astype(f64))
            out[k] = ns.sim3_map(ns.sim3_inverse(from8(S_new[ref[k]])), y).astype(np.float32)
    return out


def collect_essential_graph(m):
    """The pointer work of Optimizer.cpp:650-825 on a mirror case (ess_graph_cases.mirror_case): -> (vertex_kf, edges as (v0, v1, kind), fixed).
    Key frames are named by index; the containers the reference orders by pointer are walked in ascending index, as the mirror walks them."""
    minFeat = 100
    kfs = m["kfs"]
    vertex_kf = sorted([i for i, k in enumerate(kfs) if not k["bad"]], key=lambda i: kfs[i]["mnId"])
    vertex_of = {kf: v for v, kf in enumerate(vertex_kf)}
    mnId = lambda i: kfs[i]["mnId"]
    weight = lambda i, j: dict(zip(kfs[i]["cov"], kfs[i]["cov_w"])).get(j, 0)
    edges = []; inserted = set()

    def add(i, j, kind):
        if i in vertex_of and j in vertex_of:
            edges.append((vertex_of[i], vertex_of[j], kind))
            return True
        return False
    for i in sorted(m["loop_connections"]):                                   # :693-722
        for j in sorted(m["loop_connections"][i]):
            if (mnId(i) != mnId(m["cur"]) or mnId(j) != mnId(m["loop"])) and weight(i, j) < minFeat:
                continue
            if add(i, j, 0):
                inserted.add((min(mnId(i), mnId(j)), max(mnId(i), mnId(j))))
    for i, k in enumerate(kfs):                                               # :724-825
        if k["bad"]:
            continue
        if k["parent"] >= 0:
            add(i, k["parent"], 1)
        for l in sorted(k["loop_edges"]):
            if mnId(l) < mnId(i):
                add(i, l, 1)
        for n, w in zip(k["cov"], k["cov_w"]):
            if w < minFeat:
                break
            if n == k["parent"] or n in k["children"] or n in k["loop_edges"]:
                continue
            if not kfs[n]["bad"] and mnId(n) < mnId(i):
                if (min(mnId(i), mnId(n)), max(mnId(i), mnId(n))) in inserted:
                    continue
                add(i, n, 1)
    return vertex_kf, edges, vertex_of[m["loop"]]
