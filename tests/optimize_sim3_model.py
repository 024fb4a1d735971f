"""Float64 numpy restatement of Optimizer::OptimizeSim3 (src/Optimizer.cc:1173-1358) and of the
parts of g2o it runs.  Test-only: the reference for orbx_optimize_sim3*.

File:line of every step (g2o = Thirdparty/g2o/g2o):
  pairs and their order          Optimizer.cc:1224-1298 (slot order; the active edges are sorted by
                                 insertion id: e12 of a pair, then its e21)
  fixed points                   Optimizer.cc:1240, 1250: CV_32F; the order declared in DESIGN.md
                                 App. B: float (r0 x + r1 y) + r2 z, the translation added in
                                 double, one rounding to float
  schedule                       Optimizer.cc:1301-1357
  vertex, errors                 types/types_seven_dof_expmap.h:60-88, 138-145, 160-167
  Sim3 exp, map, inverse, *      types/sim3.h:70-142, 144, 233, 266 (the quaternion is never normalised)
  numeric Jacobian               core/base_binary_edge.hpp:131-205 (delta 1e-9, central)
  quadratic form                 core/base_binary_edge.hpp:55-120 (robust branch, `to` vertex only)
  chi2, robust information       core/base_edge.h:59-61, 96-102
  Huber                          core/robust_kernel_impl.cpp:78-91
  LM, iteration loop, solve      as tests/pose_opt_model.py, 7 x 7

Variants: `order` chooses how the per-edge terms of H, b and chi2 are added ("forward": edge
order, what g2o does; "reversed"; "pairwise"; "tree": the HIP kernel's shape), `probe` how the
exp() of the 14 probe increments Sim3(+-1e-9 e_d) is taken ("asis", or moved one ulp "up" /
"down": another libm).  They differ by rounding only; their disagreement is the scale of
legitimate differences between correct implementations.
"""
from __future__ import annotations

import functools

import numpy as np

import pose_opt_model as P
from pose_opt_model import quat_from_matrix, quat_mul, quat_rotate, quat_to_matrix

MAX_TRIALS = 10
DBL_MAX = np.finfo(np.float64).max
DELTA = 1e-9                       # base_binary_edge.hpp:147
SCALAR = 1.0 / (2 * DELTA)
TREE_THREADS = 256
ORDERS = ("forward", "reversed", "pairwise", "tree")
PROBES = ("asis", "up", "down")
VARIANTS = tuple((o, p) for o in ORDERS for p in PROBES)
_IU = [(r, c) for r in range(7) for c in range(r, 7)]   # the 28 upper entries of H, row-major


# ---- g2o::Sim3 as (q xyzw, t, s) ----------------------------------------------------------------

def sim3_from_rts(R9, t3, s):
    """g2o::Sim3(R, t, s) from floats: Quaterniond(R), not normalised."""
    R = np.asarray(R9, np.float32).astype(np.float64).reshape(3, 3)
    return quat_from_matrix(R), np.asarray(t3, np.float32).astype(np.float64).reshape(3), float(np.float32(s))


def sim3_exp(x, probe="asis"):
    """Sim3(const Vector7d&), sim3.h:70-142."""
    w, u, sigma = x[:3], x[3:6], x[6]
    theta = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    O = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    s = np.exp(sigma)
    if sigma != 0.0 and probe != "asis":
        s = np.nextafter(s, np.inf if probe == "up" else -np.inf)
    O2 = np.array([[O[i, 0] * O[0, j] + O[i, 1] * O[1, j] + O[i, 2] * O[2, j] for j in range(3)] for i in range(3)])
    I = np.eye(3)
    eps = 0.00001
    if abs(sigma) < eps:
        C = 1.0
        if theta < eps:
            A, B = 1. / 2., 1. / 6.
            R = I + O + O2
        else:
            theta2 = theta * theta
            A = (1 - np.cos(theta)) / theta2
            B = (theta - np.sin(theta)) / (theta2 * theta)
            R = I + np.sin(theta) / theta * O + (1 - np.cos(theta)) / (theta * theta) * O2
    else:
        C = (s - 1) / sigma
        if theta < eps:
            sigma2 = sigma * sigma
            A = ((sigma - 1) * s + 1) / sigma2
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
            R = I + O + O2
        else:
            R = I + np.sin(theta) / theta * O + (1 - np.cos(theta)) / (theta * theta) * O2
            a = s * np.sin(theta)
            b = s * np.cos(theta)
            theta2 = theta * theta
            sigma2 = sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2
    W = A * O + B * O2 + C * I
    t = np.array([W[i, 0] * u[0] + W[i, 1] * u[1] + W[i, 2] * u[2] for i in range(3)])
    return quat_from_matrix(R), t, float(s)


def sim3_mul(a, b):
    """Sim3::operator*, sim3.h:266-272."""
    return quat_mul(a[0], b[0]), a[2] * quat_rotate(a[0], b[1]) + a[1], a[2] * b[2]


def sim3_inverse(a):
    """Sim3::inverse, sim3.h:233-236."""
    qc = np.array([-a[0][0], -a[0][1], -a[0][2], a[0][3]])
    return qc, quat_rotate(qc, (-1. / a[2]) * a[1]), 1. / a[2]


def sim3_map(a, X):
    return a[2] * quat_rotate(a[0], X) + a[1]


def probe_increments(fix_scale, probe="asis"):
    """The 14 increments of the central difference, index 2 d + (0: +delta, 1: -delta); oplusImpl
    zeroes the seventh entry with _fix_scale."""
    out = []
    for d in range(7):
        for sgn in (DELTA, -DELTA):
            x = np.zeros(7)
            x[d] = sgn
            if fix_scale:
                x[6] = 0.0
            out.append(sim3_exp(x, probe))
    return out


# ---- pairs -----------------------------------------------------------------------------------------

def cam_points(Tcw12, X):
    """Rcw Xw + tcw as a CV_32F expression, the order declared in DESIGN.md App. B."""
    T = np.asarray(Tcw12, np.float32).reshape(3, 4)
    X = np.asarray(X, np.float32).reshape(-1, 3)
    out = np.empty((len(X), 3), np.float32)
    for r in range(3):
        s = (T[r, 0] * X[:, 0] + T[r, 1] * X[:, 1]) + T[r, 2] * X[:, 2]          # float32 throughout
        out[:, r] = (s.astype(np.float64) + np.float64(T[r, 3])).astype(np.float32)
    return out


class Pairs:
    def __init__(self, sc):
        n1, n2 = int(sc["n1"]), int(sc["n2"])
        mp1 = np.asarray(sc["mp1"][:n1], np.int64)
        m12 = np.asarray(sc["matches12"][:n1], np.int64)
        i2 = np.asarray(sc["idx2"][:n1], np.int64)
        pos = np.asarray(sc["mp_pos"], np.float32).reshape(-1, 3)
        n_mp = len(pos)
        keep = (mp1 >= 0) & (mp1 < n_mp) & (m12 >= 0) & (m12 < n_mp) & (i2 >= 0) & (i2 < n2)
        self.index = np.nonzero(keep)[0]
        self.n = len(self.index)
        ix = self.index
        self.X1 = cam_points(sc["Tcw1"], pos[mp1[ix]]).astype(np.float64)
        self.X2 = cam_points(sc["Tcw2"], pos[m12[ix]]).astype(np.float64)
        self.obs1 = np.asarray(sc["k1_xy"], np.float32)[ix].astype(np.float64).reshape(-1, 2)
        self.obs2 = np.asarray(sc["k2_xy"], np.float32)[i2[ix]].astype(np.float64).reshape(-1, 2)
        nl = len(sc["inv_sigma2_1"])
        o1 = np.clip(np.asarray(sc["k1_oct"], np.int64)[ix], 0, nl - 1)
        o2 = np.clip(np.asarray(sc["k2_oct"], np.int64)[i2[ix]], 0, nl - 1)
        self.w1 = np.asarray(sc["inv_sigma2_1"], np.float32)[o1].astype(np.float64)
        self.w2 = np.asarray(sc["inv_sigma2_2"], np.float32)[o2].astype(np.float64)
        self.K1 = tuple(float(np.float32(v)) for v in sc["K1"])
        self.K2 = tuple(float(np.float32(v)) for v in sc["K2"])
        self.delta = float(np.float32(np.sqrt(np.float32(sc["th2"]))))   # cc:1221: the float sqrt(th2)
        self.th2 = float(np.float32(sc["th2"]))


def _err(T, X, obs, K):
    fx, fy, cx, cy = K
    with np.errstate(all="ignore"):
        x = sim3_map(T, X)
        return np.stack([obs[:, 0] - ((x[:, 0] / x[:, 2]) * fx + cx), obs[:, 1] - ((x[:, 1] / x[:, 2]) * fy + cy)],
                        axis=1)


def pair_errors(E, S):
    """computeError of both edges of every pair at estimate S: [n, 2 (e12, e21), 2]."""
    return np.stack([_err(S, E.X2, E.obs1, E.K1), _err(sim3_inverse(S), E.X1, E.obs2, E.K2)], axis=1)


def pair_chi2(E, err):
    w = np.stack([E.w1, E.w2], axis=1)
    return err[:, :, 0] * (w * err[:, :, 0]) + err[:, :, 1] * (w * err[:, :, 1])


def huber(chi2, delta):
    dsqr = delta * delta
    with np.errstate(all="ignore"):
        sq = np.sqrt(chi2)
        out = chi2 > dsqr
        return np.where(out, 2.0 * sq * delta - dsqr, chi2), np.where(out, delta / sq, 1.0)


def ordered_sum(a, active, order):
    """Sum of the active pairs' rows of a [n, 2, m] array (e12 then e21 of each pair) in the
    chosen order.  "tree": thread t adds its pairs t, t + 256, ... in index order, each pair's
    e12 before its e21; lanes by an xor butterfly, the four waves in wave order."""
    a = np.asarray(a, np.float64)
    n, _, m = a.shape
    if order == "tree":
        rows = -(-max(n, 1) // TREE_THREADS)
        pad = np.zeros((rows * TREE_THREADS, 2, m))
        pad[:n][active] = a[active]
        seq = pad.reshape(rows, TREE_THREADS, 2, m).transpose(0, 2, 1, 3).reshape(rows * 2, TREE_THREADS, m)
        v = np.cumsum(seq, axis=0)[-1].reshape(TREE_THREADS // 64, 64, m)
        idx = np.arange(64)
        for step in (32, 16, 8, 4, 2, 1):
            v = v + v[:, idx ^ step]
        out = v[0, 0]
        for w in range(1, TREE_THREADS // 64):
            out = out + v[w, 0]
        return out
    flat = a[active].reshape(-1, m)
    if flat.shape[0] == 0:
        return np.zeros(m)
    if order == "forward":
        return np.cumsum(flat, axis=0)[-1]
    if order == "reversed":
        return np.cumsum(flat[::-1], axis=0)[-1]
    if order == "pairwise":
        return np.ascontiguousarray(flat.T).sum(axis=1)
    raise ValueError(order)


def numeric_jacobians(E, S, incs):
    """linearizeOplus by central difference: [n, 2 (e12, e21), 2, 7]."""
    J = np.empty((E.n, 2, 2, 7))
    for d in range(7):
        ep = pair_errors(E, sim3_mul(incs[2 * d], S))
        em = pair_errors(E, sim3_mul(incs[2 * d + 1], S))
        J[:, :, :, d] = SCALAR * (ep - em)
    return J


def build_system(E, S, active, order, incs, want_terms=False):
    """computeActiveErrors + activeRobustChi2 + buildSystem: chi, H [7, 7], b [7]."""
    err = pair_errors(E, S)
    chi2 = pair_chi2(E, err)
    rho0, rho1 = huber(chi2, E.delta)
    J = numeric_jacobians(E, S, incs)
    w = np.stack([E.w1, E.w2], axis=1)
    ww = rho1 * w                                          # robustInformation: rho' * Omega
    r = (w[:, :, None] * err) * rho1[:, :, None]           # -omega_r = (Omega e) rho'
    terms = np.empty((E.n, 2, 36))
    for k, (a, c) in enumerate(_IU):
        terms[:, :, k] = J[:, :, 0, a] * ww * J[:, :, 0, c] + J[:, :, 1, a] * ww * J[:, :, 1, c]
    for a in range(7):
        terms[:, :, 28 + a] = J[:, :, 0, a] * r[:, :, 0] + J[:, :, 1, a] * r[:, :, 1]
    terms[:, :, 35] = rho0
    s = ordered_sum(terms, active, order)
    H = np.zeros((7, 7))
    for k, (a, c) in enumerate(_IU):
        H[a, c] = H[c, a] = s[k]
    if want_terms:
        return float(s[35]), H, -s[28:35], J
    return float(s[35]), H, -s[28:35]


def robust_chi(E, S, active, order):
    rho0, _ = huber(pair_chi2(E, pair_errors(E, S)), E.delta)
    return float(ordered_sum(rho0[:, :, None], active, order)[0])


def ldlt_solve(A, b):
    """pose_opt_model.ldlt_solve for any dimension."""
    D = len(b)
    L = np.eye(D)
    d = np.zeros(D)
    for j in range(D):
        s = A[j, j]
        for k in range(j):
            s = s - L[j, k] * L[j, k] * d[k]
        if not (s > 0.0) or not np.isfinite(s):
            return None
        d[j] = s
        for i in range(j + 1, D):
            v = A[i, j]
            for k in range(j):
                v = v - L[i, k] * L[j, k] * d[k]
            L[i, j] = v / s
    y = np.zeros(D)
    for i in range(D):
        v = b[i]
        for k in range(i):
            v = v - L[i, k] * y[k]
        y[i] = v
    x = np.zeros(D)
    for i in range(D - 1, -1, -1):
        v = y[i] / d[i]
        for k in range(i + 1, D):
            v = v - L[k, i] * x[k]
        x[i] = v
    return x


def optimize(E, S, active, max_its, fix_scale, order, incs):
    """SparseOptimizer::optimize(max_its) with OptimizationAlgorithmLevenberg from estimate S."""
    accepts, dchi, H0 = [], [], None
    err_S = S
    lam = ni = 0.0
    nbad = its = 0
    x = np.zeros(7)
    stop = "iterations"
    with np.errstate(all="ignore"):
        for it in range(max_its):
            chi, H, b = build_system(E, S, active, order, incs)
            if H0 is None:
                H0 = H
            err_S = S
            ini_chi = chi
            if it == 0:
                lam = 1e-5 * max(abs(H[j, j]) for j in range(7))
                ni = 2.0
                nbad = 0
            qmax = 0
            rho = 0.0
            while True:
                A = H.copy()
                for j in range(7):
                    A[j, j] = A[j, j] + lam
                sol = ldlt_solve(A, b)
                ok = sol is not None
                if ok:
                    x = sol
                if fix_scale:
                    x[6] = 0.0
                trial = sim3_mul(sim3_exp(x), S)
                temp = robust_chi(E, trial, active, order)
                err_S = trial
                if not ok:
                    temp = DBL_MAX
                rho = chi - temp
                dchi.append(rho)
                scale = 0.0
                for j in range(7):
                    scale += x[j] * (lam * x[j] + b[j])
                scale += 1e-3
                rho = rho / scale
                if rho > 0 and np.isfinite(temp):
                    tt = 2.0 * rho - 1.0
                    alpha = 1.0 - tt * tt * tt
                    alpha = min(alpha, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    chi = temp
                    S = trial
                    accepts.append(True)
                else:
                    lam *= ni
                    ni *= 2.0
                    accepts.append(False)
                qmax += 1
                if not (rho < 0 and qmax < MAX_TRIALS):
                    break
            its += 1
            if qmax == MAX_TRIALS or rho == 0:
                stop = "trials" if qmax == MAX_TRIALS else "rho0"
                break
            dchi.append((ini_chi - chi) * 1e3 - ini_chi)
            if (ini_chi - chi) * 1e3 < ini_chi:
                nbad += 1
            else:
                nbad = 0
            if nbad >= 3:
                stop = "nbad"
                break
    return S, err_S, its, len(accepts), accepts, stop, dchi, H0


def optimize_sim3(sc, order="forward", probe="asis"):
    """Optimizer::OptimizeSim3.  Returns a dict: R12 [9], t12 [3] float32 and s12, matches12 [n1]
    (rejected entries -1), ninliers (the return value), ncorr, nbad, trace [2, 2], S64 (the 13
    output entries in double), chi2 (per classification [n, 2]; nan for pairs already out),
    accepts / stop / decisions per optimisation, H0 (the first system's H per optimisation)."""
    E = Pairs(sc)
    fix = bool(sc["fix_scale"])
    incs = probe_increments(fix, probe)
    n1 = int(sc["n1"])
    R_in = np.asarray(sc["R12"], np.float32).reshape(9)
    t_in = np.asarray(sc["t12"], np.float32).reshape(3)
    s_in = np.float32(sc["s12"])
    out = dict(R12=R_in.copy(), t12=t_in.copy(), s12=s_in, matches12=np.asarray(sc["matches12"][:n1], np.int32).copy(),
               ninliers=0, ncorr=E.n, nbad=0, trace=np.zeros((2, 2), np.int32), chi2=[], accepts=[], stop=[],
               decisions=[], H0=[], index=E.index,
               S64=np.concatenate([R_in, t_in, [s_in]]).astype(np.float64))
    S = sim3_from_rts(R_in, t_in, s_in)
    active = np.ones(E.n, bool)
    if E.n > 0:                                            # with zero edges optimize() runs no iteration
        S, err_S, its, trials, acc, stop, dchi, H0 = optimize(E, S, active, 5, fix, order, incs)
        out["trace"][0] = (its, trials)
        out["accepts"].append(acc)
        out["stop"].append(stop)
        out["decisions"].append(dchi)
        out["H0"].append(H0)
        chi2 = pair_chi2(E, pair_errors(E, err_S))
        out["chi2"].append(chi2)
        with np.errstate(all="ignore"):
            bad = (chi2[:, 0] > E.th2) | (chi2[:, 1] > E.th2)
        active = ~bad
        out["matches12"][E.index[bad]] = -1
        out["nbad"] = int(bad.sum())
    more = 10 if out["nbad"] > 0 else 5
    if E.n - out["nbad"] < 10:                             # cc:1331: return 0, g2oS12 untouched
        return out
    S, err_S, its, trials, acc, stop, dchi, H0 = optimize(E, S, active, more, fix, order, incs)
    out["trace"][1] = (its, trials)
    out["accepts"].append(acc)
    out["stop"].append(stop)
    out["decisions"].append(dchi)
    out["H0"].append(H0)
    chi2 = pair_chi2(E, pair_errors(E, err_S))
    chi2[~active] = np.nan
    out["chi2"].append(chi2)
    with np.errstate(all="ignore"):
        bad = active & ((chi2[:, 0] > E.th2) | (chi2[:, 1] > E.th2))
    out["matches12"][E.index[bad]] = -1
    out["ninliers"] = int((active & ~bad).sum())
    R = quat_to_matrix(S[0]).reshape(9)
    out["S64"] = np.concatenate([R, S[1], [S[2]]])
    out["R12"], out["t12"], out["s12"] = R.astype(np.float32), S[1].astype(np.float32), np.float32(S[2])
    return out


# ---- scenes ----------------------------------------------------------------------------------------

TUM1 = (517.306408, 516.469215, 318.643040, 255.313989)
KITTI = (718.856, 718.856, 607.1928, 185.2157)
INV_SIGMA2 = (1.2 ** (-2.0 * np.arange(8))).astype(np.float32)
TH2 = 10.0                                                 # LoopClosing.cc:352


def _rot(axis_angle):
    x = np.zeros(7)
    x[:3] = axis_angle
    return quat_to_matrix(sim3_exp(x)[0])


def make_scene(seed, npairs, cap1=None, fix_scale=False, K1=TUM1, K2=TUM1, noise=1.0, nout=0, holes=True,
               off_deg=2.0, off_m=0.05, off_s=0.03, n_slots=None, th2=TH2):
    """One loop candidate: `npairs` kept slots among n1 <= cap1, the others with a hole in one of
    mp1 / matches12 / idx2 interleaved; `nout` pairs carry a gross error of 20-60 px in one of
    their two observations; the start is off_deg / off_m / off_s off the true Sim3."""
    rng = np.random.default_rng(seed)
    N = npairs
    n1 = n_slots if n_slots is not None else (N + max(3, N // 3) if holes else N)
    cap1 = max(n1, 1) if cap1 is None else cap1
    n1 = min(n1, cap1)
    n2 = N + 7
    cap2 = n2 + 3
    s_true = 1.0 if fix_scale else 1.3
    R12, t12 = _rot(rng.normal(size=3) * 0.15), rng.normal(size=3) * 0.2

    def pose(ang, tr):
        T = np.zeros((3, 4))
        T[:, :3], T[:, 3] = _rot(rng.normal(size=3) * ang), rng.normal(size=3) * tr
        return T

    Tcw1, Tcw2 = pose(0.2, 1.0), pose(0.25, 1.5)
    z = rng.uniform(1.5, 8.0, N)
    u, v = rng.uniform(60, 580, N), rng.uniform(60, 420, N)
    X1 = np.stack([(u - K1[2]) / K1[0] * z, (v - K1[3]) / K1[1] * z, z], axis=1)
    X2 = (X1 - t12) @ R12 / s_true                       # (1 / s) R^T (X1 - t)
    inv = lambda T, X: (X - T[:, 3]) @ T[:, :3]          # noqa: E731
    pos = np.concatenate([inv(Tcw1, X1), inv(Tcw2, X2), rng.normal(size=(5, 3))]).astype(np.float32)
    n_mp = len(pos)
    o1, o2 = rng.integers(0, 8, N), rng.integers(0, 8, N)
    p1 = np.stack([K1[0] * X1[:, 0] / X1[:, 2] + K1[2], K1[1] * X1[:, 1] / X1[:, 2] + K1[3]], axis=1)
    p2 = np.stack([K2[0] * X2[:, 0] / X2[:, 2] + K2[2], K2[1] * X2[:, 1] / X2[:, 2] + K2[3]], axis=1)
    p1 += rng.normal(size=(N, 2)) * noise * (1.2 ** o1)[:, None]
    p2 += rng.normal(size=(N, 2)) * noise * (1.2 ** o2)[:, None]
    gross = np.zeros(N, bool)
    if nout:
        pick = rng.permutation(N)[:nout]
        ang, mag = rng.uniform(0, 2 * np.pi, nout), rng.uniform(20, 60, nout)
        d = np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=1)
        first = rng.integers(0, 2, nout).astype(bool)
        p1[pick[first]] += d[first]
        p2[pick[~first]] += d[~first]
        gross[pick] = True
    slots = np.sort(rng.choice(n1, N, replace=False)) if n1 > N else np.arange(N)
    k2slot = rng.permutation(n2)[:N]
    k1_xy = rng.uniform(0, 600, (cap1, 2)).astype(np.float32)
    k1_oct = rng.integers(-2, 10, cap1).astype(np.int32)
    k2_xy = rng.uniform(0, 600, (cap2, 2)).astype(np.float32)
    k2_oct = rng.integers(-2, 10, cap2).astype(np.int32)
    mp1 = np.zeros(cap1, np.int32)
    m12 = np.full(cap1, min(N, n_mp - 1), np.int32)      # beyond n1: valid ids that must not be read
    idx2 = np.zeros(cap1, np.int32)
    k1_xy[slots], k1_oct[slots] = p1.astype(np.float32), o1
    k2_xy[k2slot], k2_oct[k2slot] = p2.astype(np.float32), o2
    mp1[slots], m12[slots], idx2[slots] = np.arange(N), N + np.arange(N), k2slot
    kinds = [(-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, n2), (0, -7, 0), (0, n_mp, 0), (n_mp + 3, 0, 0), (0, 0, cap2 + 5),
             (-2147483648, 0, 0), (0, 2147483647, 0)]
    skipped = np.setdiff1d(np.arange(n1), slots)
    for j, sl in enumerate(skipped):                      # one of the three invalid, the others valid
        a, b, c = kinds[j % len(kinds)]
        mp1[sl] = a if a else rng.integers(0, max(N, 1))
        m12[sl] = b if b else N + rng.integers(0, max(N, 1))
        idx2[sl] = c if c else rng.integers(0, n2)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    dt = rng.normal(size=3)
    dt *= off_m / np.linalg.norm(dt)
    R0 = _rot(ax * np.deg2rad(off_deg)) @ R12
    s0 = s_true if fix_scale else s_true * (1.0 + off_s)
    full = np.full(cap1, False)
    full[slots] = gross
    return dict(seed=seed, n1=n1, cap1=cap1, n2=n2, cap2=cap2, k1_xy=k1_xy, k1_oct=k1_oct, k2_xy=k2_xy, k2_oct=k2_oct,
                mp1=mp1, matches12=m12, idx2=idx2, mp_pos=pos, Tcw1=Tcw1.astype(np.float32).reshape(12),
                Tcw2=Tcw2.astype(np.float32).reshape(12), inv_sigma2_1=INV_SIGMA2, inv_sigma2_2=INV_SIGMA2,
                K1=np.array(K1, np.float32), K2=np.array(K2, np.float32), R12=R0.astype(np.float32).reshape(9),
                t12=(t12 + dt).astype(np.float32), s12=np.float32(s0), th2=np.float32(th2), fix_scale=bool(fix_scale),
                npairs=N, slots=slots, gross=full, R_true=R12, t_true=t12, s_true=s_true)


def variants(sc):
    return [optimize_sim3(sc, o, p) for o, p in VARIANTS]


def guard(vs, th2=TH2):
    """The conditions on a scene: every variant agrees on the whole LM trace (every accepted or
    rejected trial, every stop reason, the rho == 0 stop included), on both classifications and
    on the counts, and every chi2 at both classifications is further from th2 than 1000 x the
    largest chi2 difference between the variants.  Returns (ok, text)."""
    a = vs[0]
    for v in vs[1:]:
        if v["accepts"] != a["accepts"] or v["stop"] != a["stop"] or not np.array_equal(v["trace"], a["trace"]):
            return False, "LM traces differ"
        if not np.array_equal(v["matches12"], a["matches12"]) or (v["ninliers"], v["ncorr"], v["nbad"]) != (
                a["ninliers"], a["ncorr"], a["nbad"]):
            return False, "classifications differ"
        if len(v["chi2"]) != len(a["chi2"]):
            return False, "classification counts differ"
    if not a["chi2"]:
        return True, "no classification"
    th2 = float(np.float32(th2))
    spread, margin = 0.0, np.inf
    for r in range(len(a["chi2"])):
        c = np.stack([v["chi2"][r] for v in vs])
        live = ~np.isnan(c[0])
        if not np.array_equal(np.isnan(c), np.broadcast_to(~live, c.shape)) or not np.isfinite(c[:, live]).all():
            return False, "non-finite chi2"
        if live.any():
            spread = max(spread, float((c[:, live].max(axis=0) - c[:, live].min(axis=0)).max()))
            margin = min(margin, float(np.abs(c[:, live] - th2).min()))
    if not margin > 1000.0 * spread:
        return False, f"chi2 margin {margin:g} within 1000 x spread {spread:g}"
    return True, f"margin {margin:g}, spread {spread:g}"


decision_margin = P.decision_margin


def s12_spread(vs):
    t = np.stack([v["S64"] for v in vs])
    return float((t.max(axis=0) - t.min(axis=0)).max())


# ---- the scenes of the GPU tests ---------------------------------------------------------------
# Pair counts: 0, 9, 10 and 11 with one outlier (the early exits), 63 / 64 / 65 (wave), 255 / 256 /
# 257 (the workgroup's stride), one sparse row (cap1 2000, 300 pairs among 1900 slots with holes).
# name -> (seed, make_scene arguments).  A scene that fails guard() gets another seed here
# (python tests/optimize_sim3_spread.py --find prints them).
SPECS = {
    "n0": dict(npairs=0), "n9": dict(npairs=9), "n10": dict(npairs=10, noise=0.3), "n11-out1": dict(npairs=11, nout=1),
    "n10-out1": dict(npairs=10, nout=1),
    "n63": dict(npairs=63, nout=6), "n64": dict(npairs=64, nout=6), "n65": dict(npairs=65, nout=6),
    "n255": dict(npairs=255, nout=25), "n256": dict(npairs=256, nout=25), "n257": dict(npairs=257, nout=25),
    "sparse-300": dict(npairs=300, nout=30, cap1=2000, n_slots=1900),
    "clean-150": dict(npairs=150, noise=0.3), "out-150": dict(npairs=150, nout=30),
    "k1k2-150": dict(npairs=150, nout=15, K2=KITTI),
}
# With a fixed scale and no rejection nothing slows Gauss-Newton down: every such scene has
# converged to rounding level by the third iteration and the variants' later trials part, so
# the two scenes without a rejection exist with a free scale only.
FREE_ONLY = ("n10", "clean-150")
SEEDS: dict = {f"{_k}-{_f}": 0 for _k in SPECS for _f in ("free", "fix") if not (_f == "fix" and _k in FREE_ONLY)}
SEEDS.update({
    "n0-free": 0, "n0-fix": 0, "n9-free": 4, "n9-fix": 8, "n10-free": 5, "n11-out1-free": 5,
    "n11-out1-fix": 35, "n10-out1-free": 1, "n10-out1-fix": 1, "n63-free": 2, "n63-fix": 52, "n64-free": 4,
    "n64-fix": 152, "n65-free": 9, "n65-fix": 249, "n255-free": 9, "n255-fix": 182, "n256-free": 6,
    "n256-fix": 125, "n257-free": 4, "n257-fix": 302, "sparse-300-free": 6, "sparse-300-fix": 91, "clean-150-free": 22,
    "out-150-free": 4, "out-150-fix": 137, "k1k2-150-free": 8, "k1k2-150-fix": 9,
})


@functools.lru_cache(maxsize=None)
def scene(name, seed=None):
    base, fix = name.rsplit("-", 1)
    return make_scene(SEEDS[name] if seed is None else seed, fix_scale=(fix == "fix"), **SPECS[base])


@functools.lru_cache(maxsize=None)
def scene_variants(name):
    return variants(scene(name))


def scene_extra(name, r):
    """What a scene must show beyond the guard."""
    base = name.rsplit("-", 1)[0]
    if base in ("clean-150", "n10"):
        return r["nbad"] == 0 and r["ninliers"] == r["ncorr"] and r["trace"][1, 0] > 0
    if base == "out-150":
        return r["nbad"] >= 5
    if base == "n11-out1":
        return r["nbad"] == 1 and r["trace"][1, 0] > 0
    if base == "n10-out1":
        return r["nbad"] == 1 and r["trace"][1, 0] == 0 and r["ninliers"] == 0
    return True


ALL_SCENES = tuple(SEEDS)
# one camera pair and one fix_scale per batch: 16 candidates of different counts
BATCH16 = ("n0", "n9", "n10", "n10-out1", "n11-out1", "n63", "n64", "n65", "n255", "n256", "n257", "sparse-300",
           "clean-150", "out-150", "n64", "n9")


# ---- batch arrays (the GPU tests and benchmarks/optsim3_bench.py) ----------------------------------
def keypoints(xy, octave):
    from orbslam2commentedbyxcm_amd import KEYPOINT_DTYPE
    k = np.zeros(len(xy), KEYPOINT_DTYPE)
    k["x"], k["y"], k["octave"] = xy[:, 0], xy[:, 1], octave
    return k


def pack(scenes):
    """Candidates of one camera pair and one fix_scale into batch arrays: a shared MapPoint
    table, ids offset per candidate (negative ids stay; ids outside a candidate's table go
    outside the shared one)."""
    from orbslam2commentedbyxcm_amd import KEYPOINT_DTYPE
    B = len(scenes)
    cap1, cap2 = max(s["cap1"] for s in scenes), max(s["cap2"] for s in scenes)
    total = sum(len(s["mp_pos"]) for s in scenes)
    assert len({s["fix_scale"] for s in scenes}) == 1
    assert all(np.array_equal(s["K1"], scenes[0]["K1"]) and np.array_equal(s["K2"], scenes[0]["K2"]) for s in scenes)
    P = dict(kps1=np.zeros((B, cap1), KEYPOINT_DTYPE), kps2=np.zeros((B, cap2), KEYPOINT_DTYPE),
             mp1=np.full((B, cap1), -1, np.int32), m12=np.full((B, cap1), -1, np.int32),
             idx2=np.full((B, cap1), -1, np.int32), n1=np.zeros(B, np.int32), n2=np.zeros(B, np.int32),
             pos=np.concatenate([s["mp_pos"] for s in scenes]).astype(np.float32),
             Tcw1=np.stack([s["Tcw1"] for s in scenes]), Tcw2=np.stack([s["Tcw2"] for s in scenes]),
             R12=np.stack([s["R12"] for s in scenes]), t12=np.stack([s["t12"] for s in scenes]),
             s12=np.array([s["s12"] for s in scenes], np.float32), cap1=cap1, cap2=cap2)
    off = 0
    for b, s in enumerate(scenes):
        c1, c2, n = s["cap1"], s["cap2"], len(s["mp_pos"])
        P["kps1"][b, :c1] = keypoints(s["k1_xy"], s["k1_oct"])
        P["kps2"][b, :c2] = keypoints(s["k2_xy"], s["k2_oct"])
        for key, src in (("mp1", "mp1"), ("m12", "matches12")):
            ids = s[src].astype(np.int64)
            P[key][b, :c1] = np.where(ids < 0, ids, np.where(ids < n, ids + off, np.minimum(ids + total, 2147483647)))
        P["idx2"][b, :c1] = s["idx2"]
        P["n1"][b], P["n2"][b] = s["n1"], s["n2"]
        off += n
    return P


# ---- the chain test: Sim3Solver's result as the start ------------------------------------------
def sim3_solver_scene(sc, draws_seed=0, min_inliers=20, max_iterations=300, probability=0.99):
    """The tests/sim3_model.py scene of the same candidate: vpMatched12 = matches12, the octaves
    of the matched keypoints, draws from a seeded generator."""
    import sim3_model as S
    n1, cap1 = sc["n1"], sc["cap1"]
    i2 = np.clip(sc["idx2"], 0, sc["cap2"] - 1)
    N = int(sc["npairs"])
    rng = np.random.default_rng(draws_seed)
    draws = np.zeros((max_iterations, 3), np.int32)
    for k in range(max_iterations):
        for j in range(3):
            draws[k, j] = rng.integers(0, max(1, N - j))
    return dict(seed=draws_seed, cap=cap1, n1=n1, mp1=sc["mp1"].copy(), mp2=sc["matches12"].copy(),
                oct1=sc["k1_oct"].copy(), oct2=sc["k2_oct"][i2].astype(np.int32), mp_pos=sc["mp_pos"],
                Tcw1=sc["Tcw1"], Tcw2=sc["Tcw2"], K1=sc["K1"], K2=sc["K2"], level_sigma2=S.LEVEL_SIGMA2,
                fix_scale=sc["fix_scale"], probability=probability, min_inliers=min_inliers,
                max_iterations=max_iterations, draws=draws, n_valid=N)


CHAIN = ("n64-free", 1)   # the scene and the draws' seed of the chain test: both guards hold


def chain_start(sc, r):
    """The candidate with a Sim3Solver result's best_R / best_t / best_s (floats) as its start."""
    fed = dict(sc)
    fed["R12"] = np.asarray(r["best_R"], np.float32).reshape(9)
    fed["t12"] = np.asarray(r["best_t"], np.float32).reshape(3)
    fed["s12"] = np.float32(r["best_s"])
    return fed
