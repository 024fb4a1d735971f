"""Float64 numpy restatement of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:873-1150) and
of the parts of g2o it runs.  Test-only: the reference for orbx_optimize_essential_graph*.

File:line of every step (g2o = Thirdparty/g2o/g2o):
  vertices, vScw, the fixed keyframe    Optimizer.cc:913-945
  measurements                          Optimizer.cc:954-986 (kind 0), 989-1089 (kind 1)
  schedule                              Optimizer.cc:890 (lambda 1e-16), 1093 (optimize(20))
  recovery                              Optimizer.cc:1100-1149
  vertex, error                         types/types_seven_dof_expmap.h:60-69, 106-114
  Sim3 exp, log, map, inverse, *        types/sim3.h:70-272 (the quaternion is never normalised);
                                        deltaR: types/se3_ops.hpp:40-47; W.lu().solve: Eigen's
                                        PartialPivLU (largest absolute value, first on ties)
  numeric Jacobians                     core/base_binary_edge.hpp:131-205 (delta 1e-9, central)
  quadratic form                        core/base_binary_edge.hpp:55-120 (information = I)
  LM                                    core/optimization_algorithm_levenberg.cpp:61-189
  linear solve                          LDL^T without pivoting in natural order; only an exactly
                                        zero or non-finite pivot fails

Variants: `order` chooses how a vertex's per-edge terms of H and b and the terms of chi2 and
computeScale are added ("forward": edge order, what g2o does; "reversed"; "pairwise"; "tree": the
HIP kernel's shape -- H and b in edge order, chi2 and computeScale by 256 threads and a
butterfly), `probe` how the exp() of the 14 probe increments is taken (optimize_sim3_model).
They differ by rounding only; their disagreement is the scale of legitimate differences between
correct implementations.
"""
from __future__ import annotations

import numpy as np

import optimize_sim3_model as O
from optimize_sim3_model import DELTA, MAX_TRIALS, ORDERS, PROBES, SCALAR, VARIANTS  # noqa: F401
from pose_opt_model import quat_from_matrix

STATUS_CAPACITY, STATUS_NO_FIXED_KF, STATUS_BAD_INDEX = 1, 2, 4
DBL_MAX = np.finfo(np.float64).max
EPS = 0.00001
TREE_THREADS = 256
BRANCHES = ("sigma0_rot0", "sigma0_rot", "sigma_rot0", "sigma_rot")


# ---- g2o::Sim3 as arrays [8, ...]: q xyzw, t, s ---------------------------------------------------

def s_rot(q, x, y, z):
    ux = q[1] * z - q[2] * y
    uy = q[2] * x - q[0] * z
    uz = q[0] * y - q[1] * x
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    return (x + q[3] * ux + (q[1] * uz - q[2] * uy), y + q[3] * uy + (q[2] * ux - q[0] * uz),
            z + q[3] * uz + (q[0] * uy - q[1] * ux))


def s_mul(a, b):
    """Sim3::operator*, sim3.h:266-272."""
    rx, ry, rz = s_rot(a, b[4], b[5], b[6])
    return np.stack(np.broadcast_arrays(
        a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
        a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
        a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
        a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2],
        a[7] * rx + a[4], a[7] * ry + a[5], a[7] * rz + a[6], a[7] * b[7]))


def s_inv(a):
    """Sim3::inverse, sim3.h:233-236."""
    k = -1. / a[7]
    qc = (-a[0], -a[1], -a[2], a[3])
    tx, ty, tz = s_rot(qc, k * a[4], k * a[5], k * a[6])
    return np.stack(np.broadcast_arrays(qc[0], qc[1], qc[2], qc[3], tx, ty, tz, 1. / a[7]))


def s_map(a, X):
    """Sim3::map of points X [..., 3]."""
    rx, ry, rz = s_rot(a, X[..., 0], X[..., 1], X[..., 2])
    return np.stack([a[7] * rx + a[4], a[7] * ry + a[5], a[7] * rz + a[6]], axis=-1)


def rot_matrix(q):
    """Eigen's toRotationMatrix, entries [3][3] of arrays."""
    tx, ty, tz = 2.0 * q[0], 2.0 * q[1], 2.0 * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz = tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def lu3_solve(W, t):
    """W.lu().solve(t): W [3][3] and t [3] of arrays; partial pivoting, the first largest."""
    W = [[np.array(W[i][j], np.float64) for j in range(3)] for i in range(3)]
    b = [np.array(t[i], np.float64) for i in range(3)]
    for k in range(2):
        best = np.abs(W[k][k])
        p = np.full(best.shape, k)
        for i in range(k + 1, 3):
            m = np.abs(W[i][k]) > best
            best = np.where(m, np.abs(W[i][k]), best)
            p = np.where(m, i, p)
        for i in range(k + 1, 3):
            m = p == i
            for c in range(3):
                W[k][c], W[i][c] = np.where(m, W[i][c], W[k][c]), np.where(m, W[k][c], W[i][c])
            b[k], b[i] = np.where(m, b[i], b[k]), np.where(m, b[k], b[i])
        for i in range(k + 1, 3):
            W[i][k] = W[i][k] / W[k][k]
            for c in range(k + 1, 3):
                W[i][c] = W[i][c] - W[i][k] * W[k][c]
    c0 = b[0]
    c1 = b[1] - W[1][0] * c0
    c2 = b[2] - (W[2][0] * c0 + W[2][1] * c1)
    x2 = c2 / W[2][2]
    x1 = (c1 - W[1][2] * x2) / W[1][1]
    x0 = (c0 - (W[0][1] * x1 + W[0][2] * x2)) / W[0][0]
    return x0, x1, x2


def s_log(a, hist=None):
    """Sim3::log, sim3.h:148-230, of a [8, ...]: [7, ...] = (omega, upsilon, sigma).  hist [4]
    counts the branches taken (BRANCHES)."""
    a = np.asarray(a, np.float64)
    with np.errstate(all="ignore"):
        s = a[7]
        sigma = np.log(s)
        R = rot_matrix(a)
        d = 0.5 * (R[0][0] + R[1][1] + R[2][2] - 1)
        dR = (R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1])
        small_rot = d > 1 - EPS
        small_sig = np.abs(sigma) < EPS
        theta = np.where(small_rot, 0.0, np.arccos(d))
        k = np.where(small_rot, 0.5, theta / (2 * np.sqrt(1 - d * d)))
        w = [k * dR[0], k * dR[1], k * dR[2]]
        theta2 = theta * theta
        sigma2 = sigma * sigma
        C = np.where(small_sig, 1.0, (s - 1) / sigma)
        A00, B00 = 1. / 2., 1. / 6.
        A01 = (1 - np.cos(theta)) / theta2
        B01 = (theta - np.sin(theta)) / (theta2 * theta)
        A10 = ((sigma - 1) * s + 1) / sigma2
        B10 = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
        sa = s * np.sin(theta)
        sb = s * np.cos(theta)
        c = theta2 + sigma * sigma
        A11 = (sa * sigma + (1 - sb) * theta) / (theta * c)
        B11 = (C - ((sb - 1) * sigma + sa * theta) / c) * 1. / theta2
        A = np.where(small_sig, np.where(small_rot, A00, A01), np.where(small_rot, A10, A11))
        B = np.where(small_sig, np.where(small_rot, B00, B01), np.where(small_rot, B10, B11))
        zero = np.zeros_like(s)
        Om = [[zero, -w[2], w[1]], [w[2], zero, -w[0]], [-w[1], w[0], zero]]
        W = [[A * Om[i][j] + ((B * Om[i][0]) * Om[0][j] + (B * Om[i][1]) * Om[1][j] + (B * Om[i][2]) * Om[2][j])
              + (C if i == j else 0.0) for j in range(3)] for i in range(3)]
        u = lu3_solve(W, (a[4], a[5], a[6]))
    if hist is not None:
        code = np.where(small_sig, 0, 2) + np.where(small_rot, 0, 1)
        hist += np.bincount(np.ravel(code), minlength=4)
    return np.stack(np.broadcast_arrays(w[0], w[1], w[2], u[0], u[1], u[2], sigma))


def s_exp(x, probe="asis"):
    q, t, s = O.sim3_exp(np.asarray(x, np.float64), probe)
    return np.concatenate([q, t, [s]])


def s_from_tcw(T12):
    """g2o::Sim3(Rcw, tcw, 1.0): Quaterniond(R), not normalised."""
    T = np.asarray(T12, np.float32).reshape(3, 4).astype(np.float64)
    return np.concatenate([quat_from_matrix(T[:, :3]), T[:, 3], [1.0]])


def s_to_tcw64(S):
    """[R | t / s] (cc:1106-1112) of S [8, K]: [K, 12] in double."""
    R = rot_matrix(S)
    k = 1. / S[7]
    return np.stack([R[0][0], R[0][1], R[0][2], S[4] * k, R[1][0], R[1][1], R[1][2], S[5] * k,
                     R[2][0], R[2][1], R[2][2], S[6] * k], axis=1)


# ---- sums ------------------------------------------------------------------------------------------

def osum(a, order):
    """Sum of the rows of a [n, m] (m sub-terms per item, added one after the other) in the chosen
    order.  "tree": thread t adds its items t, t + 256, ... in index order, the 64 lanes of a wave
    by an xor butterfly, the four waves in wave order."""
    a = np.asarray(a, np.float64)
    if a.ndim == 1:
        a = a[:, None]
    n, m = a.shape
    if n == 0:
        return 0.0
    if order == "tree":
        rows = -(-n // TREE_THREADS)
        pad = np.zeros((rows * TREE_THREADS, m))
        pad[:n] = a
        seq = pad.reshape(rows, TREE_THREADS, m).transpose(0, 2, 1).reshape(rows * m, TREE_THREADS)
        v = np.cumsum(np.concatenate([np.zeros((1, TREE_THREADS)), seq]), axis=0)[-1].reshape(TREE_THREADS // 64, 64)
        idx = np.arange(64)
        for step in (32, 16, 8, 4, 2, 1):
            v = v + v[:, idx ^ step]
        out = v[0, 0]
        for w in range(1, TREE_THREADS // 64):
            out = out + v[w, 0]
        return float(out)
    flat = a.reshape(-1)
    if order == "forward":
        return float(np.cumsum(np.concatenate([[0.0], flat]))[-1])
    if order == "reversed":
        return float(np.cumsum(flat[::-1])[-1])
    if order == "pairwise":
        return float(_pairwise(flat))
    raise ValueError(order)


def _pairwise(v):
    return v[0] if len(v) == 1 else _pairwise(v[:len(v) // 2]) + _pairwise(v[len(v) // 2:])


def vsum(terms, order):
    """A vertex's per-edge terms [n, ...] added in the chosen order; "tree" is the kernel's, which
    is edge order."""
    if order in ("forward", "tree"):
        out = terms[0].copy()
        for t in terms[1:]:
            out = out + t
        return out
    if order == "reversed":
        return vsum(terms[::-1], "forward")
    if len(terms) == 1:
        return terms[0].copy()
    return vsum(terms[:len(terms) // 2], order) + vsum(terms[len(terms) // 2:], order)


# ---- the linear solver -----------------------------------------------------------------------------

def envelope(n_kf, fixed, edge_v, dense=False):
    """free_idx [n_kf] (-1: fixed or without an edge), first [F], blocks: what
    orbx_essential_graph_envelope counts (every edge with two different indices inside the rows)."""
    ev = np.asarray(edge_v, np.int64).reshape(-1, 2)
    okm = (ev[:, 0] >= 0) & (ev[:, 0] < n_kf) & (ev[:, 1] >= 0) & (ev[:, 1] < n_kf) & (ev[:, 0] != ev[:, 1])
    return _envelope(n_kf, fixed, ev[okm], dense)


def _envelope(n_kf, fixed, ev, dense=False):
    has = np.zeros(n_kf, bool)
    has[ev.reshape(-1)] = True
    if 0 <= fixed < n_kf:
        has[fixed] = False
    idx = np.where(has, np.cumsum(has) - 1, -1)
    F = int(has.sum())
    first = np.arange(F)
    for i, j in ev:
        a, b = idx[i], idx[j]
        if a >= 0 and b >= 0:
            first[max(a, b)] = min(first[max(a, b)], min(a, b))
    if dense:
        first[:] = 0
    return idx, first, int((np.arange(F) - first + 1).sum())


def ldlt_solve_env(A, b, first):
    """(A) x = b by LDL^T without pivoting over the block envelope first [F] (blocks of 7): the
    right-looking order of lm::ldlt_solve_block -- the pivots ascending, every entry's term
    (l u) d -- with the entries outside the envelope, which are exact zeros, left out.  None: a
    pivot is exactly zero or not finite."""
    n = len(b)
    A = np.array(A, np.float64)
    x = np.array(b, np.float64)
    fs = np.repeat(np.asarray(first) * 7, 7)
    with np.errstate(all="ignore"):
        for j in range(n):
            d = A[j, j]
            if d == 0.0 or not np.isfinite(d):
                return None
            idx = j + 1 + np.nonzero(fs[j + 1:] <= j)[0]
            if len(idx):
                r = A[j, idx] / d
                A[j, idx] = r
                ix = np.ix_(idx, idx)
                A[ix] = A[ix] - (r[:, None] * r[None, :]) * d
                x[idx] = x[idx] - r * x[j]
        x = x / np.diag(A)
        for k in range(n - 1, 0, -1):
            lo = fs[k]
            x[lo:k] = x[lo:k] - A[lo:k, k] * x[k]
    return x


def ldlt_solve_dense(A, b):
    """The same factorisation without numpy, every entry by its own loop (as
    optimize_sim3_model.ldlt_solve, with the exactly-zero pivot rule): the terms k ascending,
    (L L) d; the back substitution's terms k descending."""
    D = len(b)
    A = [[float(v) for v in row] for row in np.asarray(A)]
    L = [[0.0] * D for _ in range(D)]
    d = [0.0] * D
    for j in range(D):
        s = A[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k] * d[k]
        if s == 0.0 or not np.isfinite(s):
            return None
        d[j] = s
        for i in range(j + 1, D):
            v = A[j][i]
            for k in range(j):
                v = v - L[j][k] * L[i][k] * d[k]
            L[i][j] = v / s
    y = [0.0] * D
    for i in range(D):
        v = float(b[i])
        for k in range(i):
            v = v - L[i][k] * y[k]
        y[i] = v
    x = [y[i] / d[i] for i in range(D)]
    for k in range(D - 1, 0, -1):
        for i in range(k):
            x[i] = x[i] - L[k][i] * x[k]
    return np.array(x)


# ---- the optimisation ------------------------------------------------------------------------------

class Graph:
    """The vertices, the valid edges and their measurements."""

    def __init__(self, sc):
        T = np.asarray(sc["Tcw"], np.float32).reshape(-1, 12)
        self.K = K = len(T)
        self.loop = int(sc["loop"])
        corr = np.asarray(sc["corr"], np.int64)
        cS = np.asarray(sc["corr_S"], np.float64).reshape(-1, 8)
        self.status = 0
        self.Snc = np.stack([s_from_tcw(T[k]) for k in range(K)], axis=1) if K else np.zeros((8, 0))
        self.S0 = self.Snc.copy()
        for k in range(K):
            if 0 <= corr[k] < len(cS):
                self.S0[:, k] = cS[corr[k]]
            elif corr[k] != -1:
                self.status |= STATUS_BAD_INDEX
        ev = np.asarray(sc["edge_v"], np.int64).reshape(-1, 2)
        kind = np.asarray(sc["edge_kind"], np.int64)
        ok = (ev[:, 0] >= 0) & (ev[:, 0] < K) & (ev[:, 1] >= 0) & (ev[:, 1] < K) & (ev[:, 0] != ev[:, 1]) & \
            ((kind == 0) | (kind == 1))
        if not ok.all():
            self.status |= STATUS_BAD_INDEX
        self.index = np.nonzero(ok)[0]
        self.ev = ev[ok]
        self.E = len(self.ev)
        i, j = self.ev[:, 0], self.ev[:, 1]
        k0 = (kind[ok] == 0)
        Si = np.where(k0, self.S0[:, i], self.Snc[:, i])
        Sj = np.where(k0, self.S0[:, j], self.Snc[:, j])
        self.meas = s_mul(Sj, s_inv(Si))
        self.hist = np.zeros(4, np.int64)

    def errors(self, S, Si=None, Sj=None, count=False):
        """computeError of every edge: [7, E]."""
        Si = S[:, self.ev[:, 0]] if Si is None else Si
        Sj = S[:, self.ev[:, 1]] if Sj is None else Sj
        return s_log(s_mul(s_mul(self.meas, Si), s_inv(Sj)), self.hist if count else None)

    def chi(self, S, order, count=False):
        e = self.errors(S, count=count)
        c = e[0] * e[0]
        for r in range(1, 7):
            c = c + e[r] * e[r]
        full = np.zeros(int(self.index.max()) + 1 if self.E else 0)
        full[self.index] = c
        return osum(full, order), e


def linearize(G, S, idx, F, incs, order):
    """computeActiveErrors, linearizeOplus of every edge and buildSystem at estimate S: chi, H
    [7 F, 7 F] (the upper blocks) and b."""
    vi, vj = G.ev[:, 0], G.ev[:, 1]
    chi, err = G.chi(S, order, count=True)
    # linearizeOplus: central differences over the 14 probes of either vertex
    J = np.zeros((2, G.E, 7, 7))                       # [side, edge, row, column]
    Si, Sj = S[:, vi], S[:, vj]
    for d in range(7):
        ip, im = incs[2 * d][:, None], incs[2 * d + 1][:, None]
        J[0, :, :, d] = (SCALAR * (G.errors(S, Si=s_mul(ip, Si)) - G.errors(S, Si=s_mul(im, Si)))).T
        J[1, :, :, d] = (SCALAR * (G.errors(S, Sj=s_mul(ip, Sj)) - G.errors(S, Sj=s_mul(im, Sj)))).T
    # buildSystem
    H = np.zeros((7 * F, 7 * F))
    b = np.zeros(7 * F)
    JtJ = np.zeros((2, G.E, 7, 7))
    Jte = np.zeros((2, G.E, 7))
    for sd in range(2):
        Js = J[sd]
        acc = Js[:, 0, :, None] * Js[:, 0, None, :]
        bb = Js[:, 0, :] * -err[0][:, None]
        for r in range(1, 7):
            acc = acc + Js[:, r, :, None] * Js[:, r, None, :]
            bb = bb + Js[:, r, :] * -err[r][:, None]
        JtJ[sd], Jte[sd] = acc, bb
    Jij = J[0][:, 0, :, None] * J[1][:, 0, None, :]     # J_i^T J_j
    for r in range(1, 7):
        Jij = Jij + J[0][:, r, :, None] * J[1][:, r, None, :]
    terms = [[] for _ in range(F)]
    for e in range(G.E):
        a, c = idx[vi[e]], idx[vj[e]]
        if a >= 0:
            terms[a].append((JtJ[0, e], Jte[0, e]))
        if c >= 0:
            terms[c].append((JtJ[1, e], Jte[1, e]))
        if a >= 0 and c >= 0:
            if a < c:
                H[7 * a:7 * a + 7, 7 * c:7 * c + 7] += Jij[e]
            else:
                H[7 * c:7 * c + 7, 7 * a:7 * a + 7] += Jij[e].T
    for f in range(F):
        H[7 * f:7 * f + 7, 7 * f:7 * f + 7] = vsum([t[0] for t in terms[f]], order)
        b[7 * f:7 * f + 7] = vsum([t[1] for t in terms[f]], order)
    return chi, H, b


def essential_graph(sc, order="forward", probe="asis", iterations=0, dense=False, max_env_blocks=None):
    """Optimizer::OptimizeEssentialGraph.  Returns a dict: Tcw [K, 12] and pos [P, 3] float32,
    their doubles T64 / pos64, Scw [K, 8], trace (LM iterations, linear solves), chi2 (initial,
    final), status, accepts and dchi (currentChi - tempChi) per trial, hist (the branches of
    Sim3::log over the errors at the linearisation points), blocks."""
    T_in = np.asarray(sc["Tcw"], np.float32).reshape(-1, 12)
    pos_in = np.asarray(sc["pos"], np.float32).reshape(-1, 3)
    ref = np.asarray(sc["pt_ref"], np.int64)
    G = Graph(sc)
    K = G.K
    out = dict(Tcw=T_in.copy(), pos=pos_in.copy(), T64=T_in.astype(np.float64), pos64=pos_in.astype(np.float64),
               Scw=G.S0.T.copy(), trace=np.zeros(2, np.int32), chi2=np.zeros(2), status=0, accepts=[], dchi=[],
               hist=G.hist, blocks=0)
    if not 0 <= G.loop < K:
        out["status"] = STATUS_NO_FIXED_KF
        return out
    idx, first, blocks = _envelope(K, G.loop, G.ev, dense)
    out["blocks"] = blocks
    if max_env_blocks is not None and blocks > max_env_blocks:
        out["status"] = STATUS_CAPACITY | G.status
        return out
    F = len(first)
    fix = bool(sc["fix_scale"])
    incs = [np.concatenate([q, t, [s]]) for q, t, s in O.probe_increments(fix, probe)]
    S = G.S0.copy()
    free_kf = np.nonzero(idx >= 0)[0]
    vi, vj = G.ev[:, 0], G.ev[:, 1]
    max_its = iterations if iterations > 0 else 20
    chi, _ = G.chi(S, order)
    out["chi2"][:] = chi
    its = trials = 0
    x = np.zeros(7 * F)
    lam = ni = 0.0
    nbad = 0
    with np.errstate(all="ignore"):
        for it in range(max_its if F else 0):
            chi, H, b = linearize(G, S, idx, F, incs, order)
            if it == 0:
                out["chi2"][0] = chi
                lam, ni, nbad = 1e-16, 2.0, 0
            ini_chi = chi
            qmax = 0
            rho = 0.0
            while True:
                A = H.copy()
                A[np.diag_indices(7 * F)] = A[np.diag_indices(7 * F)] + lam
                sol = ldlt_solve_env(A, b, first)
                ok = sol is not None
                if ok:
                    x = sol
                if fix:
                    x[6::7] = 0.0
                trial = S.copy()
                for f in range(F):
                    v = free_kf[f]
                    trial[:, v] = s_mul(s_exp(x[7 * f:7 * f + 7]), S[:, v])
                temp, _ = G.chi(trial, order)
                if not ok:
                    temp = DBL_MAX
                rho = chi - temp
                out["dchi"].append(rho)
                scale = osum((x * (lam * x + b)).reshape(F, 7), order) + 1e-3
                rho = rho / scale
                if rho > 0 and np.isfinite(temp):
                    tt = 2.0 * rho - 1.0
                    alpha = min(1.0 - tt * tt * tt, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    chi = temp
                    S = trial
                    out["accepts"].append(True)
                else:
                    lam *= ni
                    ni *= 2.0
                    out["accepts"].append(False)
                qmax += 1
                if not (rho < 0 and qmax < MAX_TRIALS):
                    break
            trials += qmax
            its += 1
            if qmax == MAX_TRIALS or rho == 0:
                break
            if (ini_chi - chi) * 1e3 < ini_chi:
                nbad += 1
            else:
                nbad = 0
            if nbad >= 3:
                break
    out["chi2"][1] = chi
    out["trace"][:] = (its, trials)
    out["status"] = G.status
    out["Scw"] = S.T.copy()
    out["T64"] = s_to_tcw64(S) if K else out["T64"]
    out["Tcw"] = out["T64"].astype(np.float32)
    good = (ref >= 0) & (ref < K)
    if not good.all():
        out["status"] |= STATUS_BAD_INDEX
    r = ref[good]
    if len(r):
        with np.errstate(all="ignore"):
            X = s_map(G.S0[:, r], pos_in[good].astype(np.float64))
            out["pos64"][good] = s_map(s_inv(S[:, r]), X)
    out["pos"] = np.where(good[:, None], out["pos64"].astype(np.float32), pos_in)
    return out


# ---- scenes ----------------------------------------------------------------------------------------

def _se3(axis_angle, t):
    x = np.zeros(7)
    x[:3] = axis_angle
    q = s_exp(x)[:4]
    T = np.eye(4)
    T[:3, :3] = np.array(rot_matrix(q))
    T[:3, 3] = t
    return T


def _sim3_of(T, s=1.0):
    return np.concatenate([quat_from_matrix(T[:3, :3]), T[:3, 3], [s]])


def make_scene(seed, n, fix_scale=False, fixed=0, band=1, loops=(), n_corr=3, kind0=None, drift_deg=4.0,
               drift_pos=0.10, drift_s=0.05, step=0.3, extra_edges=(), isolated=0):
    """A closed trajectory of n keyframes `step` apart whose estimates drifted by drift_deg degrees,
    drift_pos of the path and drift_s of scale over the loop; the last n_corr keyframes carry the
    corrected Sim3 CorrectLoop would leave (LoopClosing.cc:488-530).  Edges in the reference's
    order: the kind-0 LoopConnections edges, then per keyframe its spanning-tree edge (to k - 1),
    its loop edges and its covisibility edges to k - 2 .. k - band.  `loops`: (k, l) loop edges,
    l < k.  `isolated` more keyframes without an edge follow.  3 points per keyframe."""
    rng = np.random.default_rng(seed)
    if fix_scale:
        drift_s = 0.0
    radius = n * step / (2 * np.pi)
    ang = 2 * np.pi * np.arange(n) / n
    Twc = []
    for k in range(n):                                       # the true poses: on a circle, looking along it
        T = _se3(np.array([0.0, ang[k], 0.0]), np.array([radius * np.cos(ang[k]), 0.0, -radius * np.sin(ang[k])]))
        Twc.append(T)
    # the drifted estimates: every relative motion is off by a little rotation, translation and scale
    per = 1.0 / max(n - 1, 1)
    order_k = list(range(fixed, n)) + list(range(fixed - 1, -1, -1))
    prev = {fixed: (Twc[fixed].copy(), 1.0)}
    Tdr = {fixed: Twc[fixed].copy()}
    for a in range(1, len(order_k)):
        k = order_k[a]
        p = k - 1 if k > fixed else k + 1
        Tp, sp = prev[p]
        rel = np.linalg.inv(Twc[p]) @ Twc[k]
        noise = _se3(rng.normal(size=3) * np.deg2rad(drift_deg) * np.sqrt(per), rng.normal(size=3) * drift_pos * step)
        s = sp * (1.0 + drift_s * per)
        rel = rel @ noise
        rel[:3, 3] *= s
        Tk = Tp @ rel
        prev[k] = (Tk, s)
        Tdr[k] = Tk
    K = n + isolated
    for k in range(n, K):
        Tdr[k] = _se3(rng.normal(size=3) * 0.2, rng.normal(size=3) * 3.0)
    Tcw = np.stack([np.linalg.inv(Tdr[k])[:3].reshape(12) for k in range(K)]).astype(np.float32)
    # CorrectLoop: the current keyframe n - 1 takes the loop's measured Sim3 to the fixed keyframe
    cur = n - 1
    corr = np.full(K, -1, np.int32)
    corr_S = []
    if n_corr and n > 1:
        s_cur = 1.0 / prev[cur][1]
        rel_true = np.linalg.inv(Twc[cur]) @ Twc[fixed]       # T_cur<-fixed of the true trajectory
        S_cw = s_mul(_sim3_of(rel_true, s_cur), s_from_tcw(Tcw[fixed]))
        for k in range(max(n - n_corr, 0), n):
            if k == fixed:
                continue
            S_kc = s_mul(s_from_tcw(Tcw[k]), s_inv(s_from_tcw(Tcw[cur])))
            corr[k] = len(corr_S)
            corr_S.append(s_mul(S_kc, S_cw))
    ev, kind = [], []
    for i, j in (kind0 if kind0 is not None else ()):
        ev.append((i, j))
        kind.append(0)
    for k in range(n):
        if k >= 1:
            ev.append((k, k - 1))
            kind.append(1)
        for kk, l in loops:
            if kk == k:
                ev.append((k, l))
                kind.append(1)
        for m in range(2, band + 1):
            if k - m >= 0:
                ev.append((k, k - m))
                kind.append(1)
    for i, j, kd in extra_edges:
        ev.append((i, j))
        kind.append(kd)
    pos, ref = [], []
    for k in range(K):
        for m, r in enumerate((k, (k + 1) % K, fixed if fixed < K else 0)):
            Xc = np.array([rng.uniform(-1, 1), rng.uniform(-0.5, 0.5), rng.uniform(2, 6)])
            pos.append(Tdr[k][:3, :3] @ Xc + Tdr[k][:3, 3])
            ref.append(r)
    return dict(Tcw=Tcw, corr=corr, corr_S=np.array(corr_S, np.float64).reshape(-1, 8), loop=fixed,
                edge_v=np.array(ev, np.int32).reshape(-1, 2), edge_kind=np.array(kind, np.int32),
                pos=np.array(pos, np.float32).reshape(-1, 3), pt_ref=np.array(ref, np.int32), fix_scale=int(fix_scale))


def _ring(n, seed, **kw):
    """n keyframes (n - 1 may move: the scenes are named by those): the loop edge cur -> 0 and the kind-0 edges of ring-9."""
    kw.setdefault("loops", ((n - 1, 0),))
    kw.setdefault("kind0", ((n - 1, 0), (n - 2, 0), (n - 2, 1)))
    kw.setdefault("band", 2)
    return make_scene(seed, n, **kw)


BIG = dict(drift_deg=60.0, drift_pos=0.6)   # see SPECS


def _bad_edges():
    sc = _ring(9, 3, fix_scale=True, **BIG)
    ev, kind = list(map(tuple, sc["edge_v"])), list(sc["edge_kind"])
    for at, (e, kd) in ((1, ((3, 9), 1)), (4, ((-1, 2), 1)), (6, ((5, 5), 1)), (9, ((4, 2), 2)), (12, ((2, 6), -1))):
        ev.insert(at, e)
        kind.insert(at, kd)
    sc["edge_v"], sc["edge_kind"] = np.array(ev, np.int32), np.array(kind, np.int32)
    sc["pt_ref"] = sc["pt_ref"].copy()
    sc["pt_ref"][[2, 11]] = (9, -1)
    return sc


# name: (maker, the iteration count k of the exact part).  Seeds and drifts: chosen so that
# guard() holds with k >= 4 (k >= 2 for pair, chain-3 and isolated); python
# tests/essential_graph_spread.py prints every scene's guard.  With a real loop's drift (a few
# degrees, 10 % of the path, 5 % of scale: make_scene's defaults) a fixed-scale optimisation has
# converged to rounding noise by its third iteration and its fourth decides on that noise, so the
# scenes that must be decided for four iterations drift by BIG (pair, whose single edge is solved by
# the first step but for the curvature, by more).  With a free scale an edge whose
# rotation error is below 0.26 degrees takes the branch of Sim3::log whose B lacks its "- 1"
# (sim3.h:199): W is then close to singular, the steps are wild and most trials are rejected --
# ring-9 and tiny are such scenes: they end in their second and third iteration on ten rejected
# trials in a row (qmax == 10), each rejection by the guard's margin; the rings of 63 and more
# vertices have a fixed scale.
SPECS = {
    "pair": (lambda: make_scene(14, 2, n_corr=1, drift_deg=90.0, drift_pos=1.0, drift_s=0.5), 2),
    "chain-3": (lambda: make_scene(2, 3, n_corr=1, kind0=((2, 0),)), 2),
    "ring-9": (lambda: _ring(9, 3), 4),
    "ring-9-fixed-scale": (lambda: _ring(9, 3, fix_scale=True, **BIG), 4),
    "ring-63": (lambda: _ring(64, 4, fix_scale=True, **BIG), 4),
    "ring-64": (lambda: _ring(65, 5, fix_scale=True, **BIG), 4),
    "ring-65": (lambda: _ring(66, 6, fix_scale=True, **BIG), 4),
    "ring-257": (lambda: _ring(258, 8, fix_scale=True, band=3, loops=((257, 0), (200, 40), (130, 5)), **BIG), 4),
    "fixed-mid": (lambda: make_scene(3, 9, fixed=4, band=2, n_corr=2, kind0=((8, 4), (7, 4)), **BIG,
                                     extra_edges=((2, 3, 1), (3, 2, 1), (6, 5, 1), (1, 5, 1), (5, 1, 1))), 4),
    "isolated": (lambda: _ring(6, 10, isolated=1), 2),
    "bad-edges": (_bad_edges, 4),
    "tiny": (lambda: _ring(9, 16, drift_deg=0.005, drift_pos=0.002, drift_s=0.05), 4),
    "large": (lambda: _ring(9, 4, drift_s=0.3, **BIG), 4),
}
_cache: dict = {}


def scene(name):
    if name not in _cache:
        _cache[name] = SPECS[name][0]()
    return _cache[name]


def exact_iterations(name):
    return SPECS[name][1]


_runs: dict = {}


def variants(name, iterations=0):
    """Every variant's result on a named scene, computed once."""
    key = (name, iterations)
    if key not in _runs:
        _runs[key] = [essential_graph(scene(name), o, p, iterations) for o, p in VARIANTS]
    return _runs[key]


def guard(name, iterations):
    """The conditions under which the trace at `iterations` is decided: every variant takes the
    same accept / reject decisions, and every trial's |currentChi - tempChi| is at least 1000 x
    its largest difference between the variants.  Returns (ok, why)."""
    rs = variants(name, iterations)
    acc = rs[0]["accepts"]
    for r in rs[1:]:
        if r["accepts"] != acc or tuple(r["trace"]) != tuple(rs[0]["trace"]):
            return False, "decisions differ between variants"
    d = np.array([r["dchi"] for r in rs])
    if d.size:
        spread = d.max(axis=0) - d.min(axis=0)
        if not (np.abs(d).min(axis=0) >= 1000.0 * spread).all():
            return False, f"margin: |dchi| {np.abs(d).min(axis=0)} vs spread {spread}"
    return True, ""


def spread(name, iterations=0):
    """The largest entry difference of Tcw_opt and pt_pos_opt (in double, before the rounding to
    float) between the variants, and the relative spread of the final chi2."""
    rs = variants(name, iterations)
    T = np.array([r["T64"] for r in rs])
    X = np.array([r["pos64"] for r in rs])
    c = np.array([r["chi2"][1] for r in rs])
    return (float((T.max(0) - T.min(0)).max()) if T.size else 0.0, float((X.max(0) - X.min(0)).max()) if X.size else 0.0,
            float((c.max() - c.min()) / max(abs(c).max(), np.finfo(float).tiny)))


def pack(scenes):
    """Concatenate scenes into the tables of orbx_essential_graph_batch."""
    kf_off, edge_off, pt_off, c_off = [0], [0], [0], 0
    corr = []
    for sc in scenes:
        kf_off.append(kf_off[-1] + len(sc["Tcw"]))
        edge_off.append(edge_off[-1] + len(sc["edge_v"]))
        pt_off.append(pt_off[-1] + len(sc["pos"]))
        corr.append(np.where(sc["corr"] >= 0, sc["corr"] + c_off, sc["corr"]))
        c_off += len(sc["corr_S"])
    cat = lambda k, dt, shape: np.concatenate([np.asarray(sc[k], dt).reshape(shape) for sc in scenes])  # noqa: E731
    return dict(kf_off=np.array(kf_off, np.int32), edge_off=np.array(edge_off, np.int32), pt_off=np.array(pt_off, np.int32),
                Tcw=cat("Tcw", np.float32, (-1, 12)), corr=np.concatenate(corr).astype(np.int32),
                corr_S=cat("corr_S", np.float64, (-1, 8)), loop=np.array([sc["loop"] for sc in scenes], np.int32),
                edge_v=cat("edge_v", np.int32, (-1, 2)), edge_kind=cat("edge_kind", np.int32, (-1,)),
                pos=cat("pos", np.float32, (-1, 3)), pt_ref=cat("pt_ref", np.int32, (-1,)))
