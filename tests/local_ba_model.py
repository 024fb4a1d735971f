"""Float64 numpy restatement of Optimizer::LocalBundleAdjustment (src/Optimizer.cc:586-853) and
of the parts of g2o it runs.  Test-only: the reference for orbx_local_bundle_adjustment*
(Eigen is absent, so no g2o binary can be built).

File:line of every step (g2o = Thirdparty/g2o/g2o):
  vertices, edges, their order   Optimizer.cc:601-735 (point order, then the order within a point)
  schedule, levels, vToErase     Optimizer.cc:743-821
  errors                         types/types_six_dof_expmap.h computeError, isDepthPositive;
                                 types_six_dof_expmap.cpp:141-157 (stereo: float invz, and bf is a
                                 const float& there, so bf * invz is a float product)
  Jacobians                      types_six_dof_expmap.cpp:103-139, 188-234 (divisions by z, z_2)
  quadratic form                 core/base_binary_edge.hpp:55-120
  Huber                          core/robust_kernel_impl.cpp:78-91
  LM                             core/optimization_algorithm_levenberg.cpp:61-189
  Schur complement, x_l          core/block_solver.hpp:354-486
  SE3Quat                        types/se3quat.h; update types_six_dof_expmap.h oplusImpl

Variants (their disagreement is the scale of legitimate differences between correct
implementations):
  order   how sums over edges / points are added: "forward" (what g2o does), "reversed",
          "pairwise", "kernel" (the shapes of csrc/orbx_localba.hip)
  inv3    the 3x3 inverse of Hll + lambda I: "cofactor" (Eigen's fixed-size inverse) or "ldlt"
  perm    the order in which the reduced system is factored: "natural", "reversed", or an
          integer seed of a random symmetric permutation (the reference's AMD ordering is one)
"""
from __future__ import annotations

import numpy as np

import pose_opt_model as PM
from pose_opt_model import quat_to_matrix, se3_exp, se3_mul, se3_from_tcw, se3_to_tcw, rot, TUM1, INV_SIGMA2, DBL_MAX

DELTA_MONO = PM.DELTA_MONO
DELTA_STEREO = PM.DELTA_STEREO
CHI2_MONO = 5.991          # cc:764: a double literal, no float cast
CHI2_STEREO = 7.815
MAX_TRIALS = 10
MAX_FREE_KF = 64           # ORBX_LOCAL_BA_MAX_FREE_KF
STATUS_CAPACITY, STATUS_NO_FREE_KF, STATUS_BAD_INDEX = 1, 2, 4
THREADS = 256


# ---- sums ------------------------------------------------------------------------------------

def _butterfly(lanes, waves):
    """lanes [waves * 64, m] -> the sum every thread ends with (xor butterfly, waves in order)."""
    v = lanes.reshape(waves, 64, -1)
    idx = np.arange(64)
    for step in (32, 16, 8, 4, 2, 1):
        v = v + v[:, idx ^ step]
    out = v[0, 0]
    for w in range(1, waves):
        out = out + v[w, 0]
    return out


def _strided(flat, owner, threads):
    """Thread t adds the rows it owns in row order; then the butterfly."""
    m = flat.shape[1]
    if flat.shape[0] == 0:
        return np.zeros(m)
    o = np.argsort(owner, kind="stable")
    cnt = np.bincount(owner, minlength=threads)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    pos = np.arange(len(o)) - start[owner[o]]
    M = np.zeros((threads, int(cnt.max()), m))
    M[owner[o], pos] = flat[o]
    return _butterfly(np.cumsum(M, axis=1)[:, -1], threads // 64)


def _pairwise(flat):
    n = flat.shape[0]
    if n == 1:
        return flat[0]
    return _pairwise(flat[:n // 2]) + _pairwise(flat[n // 2:])


def osum(a, order, owner=None, threads=THREADS):
    """Sum over axis 0 of a [n, ...] array from 0.0 in the chosen order; "kernel": rows are
    dealt to `threads` threads by `owner` (default: row index mod threads)."""
    a = np.asarray(a, np.float64)
    flat = a.reshape(a.shape[0], -1)
    if flat.shape[0] == 0:
        return np.zeros(a.shape[1:])
    if order == "forward":
        out = np.cumsum(flat, axis=0)[-1]
    elif order == "reversed":
        out = np.cumsum(flat[::-1], axis=0)[-1]
    elif order == "pairwise":
        out = _pairwise(flat)
    elif order == "kernel":
        if owner is None:
            owner = np.arange(flat.shape[0]) % threads
        out = _strided(flat, np.asarray(owner), threads)
    else:
        raise ValueError(order)
    return out.reshape(a.shape[1:])


def group_sum(a, group, ngroups, order, kind):
    """Per group g the sum of the rows with group == g, in row order under "forward".
    kind "point": the kernel's owner is one thread (forward); "kf": one wave, lane = position
    in the group's list mod 64."""
    a = np.asarray(a, np.float64)
    out = np.zeros((ngroups,) + a.shape[1:])
    o = np.argsort(group, kind="stable")
    cnt = np.bincount(group, minlength=ngroups)
    start = np.concatenate([[0], np.cumsum(cnt)])
    for g in range(ngroups):
        rows = o[start[g]:start[g + 1]]
        if len(rows) == 0:
            continue
        if order == "kernel":
            out[g] = osum(a[rows], "forward") if kind == "point" else osum(a[rows], "kernel", threads=64)
        else:
            out[g] = osum(a[rows], order)
    return out


# ---- edges -------------------------------------------------------------------------------------

def quat_rotate_v(q, v):
    """Eigen's Quaternion * Vector3 for per-row quaternions q [n, 4] and vectors v [n, 3]."""
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    ux = q[:, 1] * z - q[:, 2] * y
    uy = q[:, 2] * x - q[:, 0] * z
    uz = q[:, 0] * y - q[:, 1] * x
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    return np.stack([x + q[:, 3] * ux + (q[:, 1] * uz - q[:, 2] * uy),
                     y + q[:, 3] * uy + (q[:, 2] * ux - q[:, 0] * uz),
                     z + q[:, 3] * uz + (q[:, 0] * uy - q[:, 1] * ux)], axis=1)


class Edges:
    """The graph's edges in point order, then the order within a point (cc:656-735)."""

    def __init__(self, sc):
        K, P = len(sc["fixed"]), len(sc["pos"])
        off = np.asarray(sc["obs_off"], np.int64)
        kf = np.asarray(sc["obs_kf"], np.int64)
        kp = np.asarray(sc["obs_kp"], np.int64)
        n_slots, cap = sc["kps_xy"].shape[:2]
        pt = np.repeat(np.arange(P), np.diff(off))
        ok = (kf >= 0) & (kf < K) & (kp >= 0) & (kp < cap)
        slot = np.where(ok, np.asarray(sc["slot"], np.int64)[np.clip(kf, 0, max(K - 1, 0))], -1) if K else np.full(len(kf), -1)
        ok &= (slot >= 0) & (slot < n_slots)
        for j in range(P):                                  # one observation per keyframe
            seen = set()
            for e in range(off[j], off[j + 1]):
                if ok[e] and int(kf[e]) in seen:
                    ok[e] = False
                seen.add(int(kf[e]))
        self.bad_index = bool((~ok).any())
        self.index = np.nonzero(ok)[0]                      # observation of each edge
        self.pt, self.kf = pt[ok], kf[ok]
        s, k = slot[ok], kp[ok]
        xy = sc["kps_xy"][s, k].astype(np.float64)
        ur = np.full(len(s), -1.0, np.float32) if sc["u_right"] is None else sc["u_right"][s, k]
        self.stereo = ~(ur < 0)                             # cc:679
        self.obs = np.zeros((len(s), 3))
        self.obs[:, :2] = xy
        self.obs[self.stereo, 2] = ur[self.stereo].astype(np.float64)
        octv = np.clip(sc["kps_oct"][s, k], 0, len(sc["inv_sigma2"]) - 1)
        self.w = np.asarray(sc["inv_sigma2"], np.float32)[octv].astype(np.float64)
        self.delta = np.where(self.stereo, DELTA_STEREO, DELTA_MONO)
        self.n = len(s)


def edge_errors(E, cam, q, t, X):
    """computeError at poses (q [K, 4], t [K, 3]) and points X [P, 3]: err [n, 3], Xc [n, 3]."""
    fx, fy, cx, cy, bf = cam
    Xc = quat_rotate_v(q[E.kf], X[E.pt]) + t[E.kf]
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    err = np.zeros((E.n, 3))
    with np.errstate(all="ignore"):
        err[:, 0] = E.obs[:, 0] - ((x / z) * fx + cx)
        err[:, 1] = E.obs[:, 1] - ((y / z) * fy + cy)
        invz32 = (1.0 / z).astype(np.float32)               # const float invz = 1.0f / trans_xyz[2]
        invz = invz32.astype(np.float64)
        bfz = (np.float32(bf) * invz32).astype(np.float64)  # bf * invz: float * float
        r0 = x * invz * fx + cx
        r1 = y * invz * fy + cy
        r2 = r0 - bfz
        s = E.stereo
        err[s, 0] = E.obs[s, 0] - r0[s]
        err[s, 1] = E.obs[s, 1] - r1[s]
        err[s, 2] = E.obs[s, 2] - r2[s]
    return err, Xc


def edge_chi2(E, err):
    c = err[:, 0] * (E.w * err[:, 0]) + err[:, 1] * (E.w * err[:, 1])
    return c + err[:, 2] * (E.w * err[:, 2])


def huber(E, chi2, robust):
    if not robust:
        return chi2, np.ones_like(chi2)
    dsqr = E.delta * E.delta
    with np.errstate(all="ignore"):
        sq = np.sqrt(chi2)
        out = chi2 > dsqr
        return np.where(out, 2.0 * sq * E.delta - dsqr, chi2), np.where(out, E.delta / sq, 1.0)


def edge_jacobians(E, cam, Rk, Xc):
    """linearizeOplus: Ja [n, 3, 3] (the point), Jb [n, 3, 6] (the pose); row 2 zero for monocular."""
    fx, fy, cx, cy, bf = cam
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    R = Rk[E.kf]
    s = E.stereo
    with np.errstate(all="ignore"):
        z_2 = z * z
        Jb = np.zeros((E.n, 3, 6))
        Jb[:, 0, 0] = x * y / z_2 * fx
        Jb[:, 0, 1] = -(1 + (x * x / z_2)) * fx
        Jb[:, 0, 2] = y / z * fx
        Jb[:, 0, 3] = -1. / z * fx
        Jb[:, 0, 5] = x / z_2 * fx
        Jb[:, 1, 0] = (1 + y * y / z_2) * fy
        Jb[:, 1, 1] = -x * y / z_2 * fy
        Jb[:, 1, 2] = -x / z * fy
        Jb[:, 1, 4] = -1. / z * fy
        Jb[:, 1, 5] = y / z_2 * fy
        Jb[s, 2, 0] = Jb[s, 0, 0] - bf * y[s] / z_2[s]
        Jb[s, 2, 1] = Jb[s, 0, 1] + bf * x[s] / z_2[s]
        Jb[s, 2, 2] = Jb[s, 0, 2]
        Jb[s, 2, 3] = Jb[s, 0, 3]
        Jb[s, 2, 5] = Jb[s, 0, 5] - bf / z_2[s]
        Ja = np.zeros((E.n, 3, 3))
        sc = -1. / z                                         # (-1. / z * tmp) * R
        t00, t02, t11, t12 = sc * fx, sc * (-x / z * fx), sc * fy, sc * (-y / z * fy)
        for c in range(3):
            mono0 = t00 * R[:, 0, c] + t02 * R[:, 2, c]
            mono1 = t11 * R[:, 1, c] + t12 * R[:, 2, c]
            st0 = -fx * R[:, 0, c] / z + fx * x * R[:, 2, c] / z_2
            st1 = -fy * R[:, 1, c] / z + fy * y * R[:, 2, c] / z_2
            Ja[:, 0, c] = np.where(s, st0, mono0)
            Ja[:, 1, c] = np.where(s, st1, mono1)
            Ja[:, 2, c] = np.where(s, st0 - bf * R[:, 2, c] / z_2, 0.0)
    return Ja, Jb


_IU6 = [(r, c) for r in range(6) for c in range(r, 6)]
_IU3 = [(r, c) for r in range(3) for c in range(r, 3)]


def inverse3(M, how):
    """(Hll + lambda I)^-1 for M [n, 3, 3] symmetric."""
    with np.errstate(all="ignore"):
        if how == "cofactor":                               # Eigen's compute_inverse_size3
            m = M
            c00 = m[:, 1, 1] * m[:, 2, 2] - m[:, 1, 2] * m[:, 2, 1]
            c10 = m[:, 2, 1] * m[:, 0, 2] - m[:, 2, 2] * m[:, 0, 1]
            c20 = m[:, 0, 1] * m[:, 1, 2] - m[:, 0, 2] * m[:, 1, 1]
            det = (c00 * m[:, 0, 0] + c10 * m[:, 1, 0]) + c20 * m[:, 2, 0]
            inv = 1.0 / det
            D = np.empty_like(M)
            D[:, 0, 0], D[:, 0, 1], D[:, 0, 2] = c00 * inv, c10 * inv, c20 * inv
            D[:, 1, 0] = (m[:, 1, 2] * m[:, 2, 0] - m[:, 1, 0] * m[:, 2, 2]) * inv
            D[:, 1, 1] = (m[:, 2, 2] * m[:, 0, 0] - m[:, 2, 0] * m[:, 0, 2]) * inv
            D[:, 1, 2] = (m[:, 0, 2] * m[:, 1, 0] - m[:, 0, 0] * m[:, 1, 2]) * inv
            D[:, 2, 0] = (m[:, 1, 0] * m[:, 2, 1] - m[:, 1, 1] * m[:, 2, 0]) * inv
            D[:, 2, 1] = (m[:, 2, 0] * m[:, 0, 1] - m[:, 2, 1] * m[:, 0, 0]) * inv
            D[:, 2, 2] = (m[:, 0, 0] * m[:, 1, 1] - m[:, 0, 1] * m[:, 1, 0]) * inv
            return D
        d0 = M[:, 0, 0]                                       # LDL^T, then L^-T D^-1 L^-1
        l10, l20 = M[:, 1, 0] / d0, M[:, 2, 0] / d0
        d1 = M[:, 1, 1] - l10 * l10 * d0
        l21 = (M[:, 2, 1] - l20 * l10 * d0) / d1
        d2 = M[:, 2, 2] - l20 * l20 * d0 - l21 * l21 * d1
        D = np.empty_like(M)
        for c in range(3):
            b = [1.0 if c == 0 else 0.0, 1.0 if c == 1 else 0.0, 1.0 if c == 2 else 0.0]
            y0 = b[0] + 0 * d0
            y1 = b[1] - l10 * y0
            y2 = b[2] - l20 * y0 - l21 * y1
            x2 = y2 / d2
            x1 = y1 / d1 - l21 * x2
            x0 = y0 / d0 - l10 * x1 - l20 * x2
            D[:, 0, c], D[:, 1, c], D[:, 2, c] = x0, x1, x2
        return D


def ldlt_solve(S, b, perm):
    """The upper triangle of S: unpivoted LDL^T in the order `perm`, the arithmetic of
    lm::ldlt_solve_block.  Returns (x or None, pivots)."""
    n = len(b)
    A = np.triu(S) + np.triu(S, 1).T
    if perm == "natural":
        p = np.arange(n)
    elif perm == "reversed":
        p = np.arange(n)[::-1]
    else:
        p = np.random.default_rng(int(perm)).permutation(n)
    A = A[np.ix_(p, p)].copy()
    x = np.asarray(b, np.float64)[p].copy()
    piv = np.zeros(n)
    with np.errstate(all="ignore"):
        for j in range(n):
            d = A[j, j]
            piv[j] = d
            if d == 0.0 or not np.isfinite(d):
                return None, piv[:j + 1]
            A[j, j + 1:] = A[j, j + 1:] / d
            l = A[j, j + 1:]
            A[j + 1:, j + 1:] = A[j + 1:, j + 1:] - l[:, None] * l[None, :] * d
        for k in range(n - 1):
            x[k + 1:] = x[k + 1:] - A[k, k + 1:] * x[k]
        x = x / np.diag(A)
        for k in range(n - 1, 0, -1):
            x[:k] = x[:k] - A[:k, k] * x[k]
    out = np.empty(n)
    out[p] = x
    return out, piv


# ---- the optimisation ----------------------------------------------------------------------------

def linearize(E, cam, st, ae, ef, F, robust, order):
    """computeActiveErrors + activeRobustChi2 + buildSystem over the active edges ae: chi, the
    chi2 of every edge, Hll [P, 3, 3], bl [P, 3], Hpp [F, 6, 6], bp [6 F], the blocks
    W = A^T (rho' Omega) B [n, 3, 6] and the active edges at free keyframes."""
    P = len(st.X)
    n = 6 * F
    err, Xc = edge_errors(E, cam, st.q, st.t, st.X)
    c2 = edge_chi2(E, err)
    rho0, rho1 = huber(E, c2, robust)
    chi = float(osum(rho0[ae], order, owner=E.pt[ae] % THREADS))
    Ja, Jb = edge_jacobians(E, cam, st.R(), Xc)
    w = rho1 * E.w
    wr = -(E.w[:, None] * err) * rho1[:, None]
    hl = np.stack([Ja[:, 0, a] * w * Ja[:, 0, c] + Ja[:, 1, a] * w * Ja[:, 1, c] + Ja[:, 2, a] * w * Ja[:, 2, c]
                   for a, c in _IU3], axis=1)
    blt = np.stack([Ja[:, 0, a] * wr[:, 0] + Ja[:, 1, a] * wr[:, 1] + Ja[:, 2, a] * wr[:, 2] for a in range(3)], axis=1)
    hp = np.stack([Jb[:, 0, a] * w * Jb[:, 0, c] + Jb[:, 1, a] * w * Jb[:, 1, c] + Jb[:, 2, a] * w * Jb[:, 2, c]
                   for a, c in _IU6], axis=1)
    bpt = np.stack([Jb[:, 0, a] * wr[:, 0] + Jb[:, 1, a] * wr[:, 1] + Jb[:, 2, a] * wr[:, 2] for a in range(6)], axis=1)
    W = np.stack([np.stack([Ja[:, 0, a] * w * Jb[:, 0, c] + Ja[:, 1, a] * w * Jb[:, 1, c] + Ja[:, 2, a] * w * Jb[:, 2, c]
                            for c in range(6)], axis=1) for a in range(3)], axis=1)     # [n, 3, 6]
    hll = group_sum(hl[ae], E.pt[ae], P, order, "point")
    bl = group_sum(blt[ae], E.pt[ae], P, order, "point")
    fe = ae[ef[ae] >= 0]                             # active edges at free keyframes
    hpp = group_sum(hp[fe], ef[fe], F, order, "kf")
    bp = group_sum(bpt[fe], ef[fe], F, order, "kf").reshape(n)
    Hll = np.zeros((P, 3, 3))
    for q, (a, c) in enumerate(_IU3):
        Hll[:, a, c] = Hll[:, c, a] = hll[:, q]
    Hpp = np.zeros((F, 6, 6))
    for q, (a, c) in enumerate(_IU6):
        Hpp[:, a, c] = Hpp[:, c, a] = hpp[:, q]
    return chi, c2, Hll, bl, Hpp, bp, W, fe


def schur_solve(E, ef, fe, by_pt, Hll, bl, Hpp, bp, W, lam, apt, order, inv3, perm):
    """setLambda and BlockSolver::solve (block_solver.hpp:354-486): (x_p or None, x_l, pivots)."""
    P, F = len(Hll), len(Hpp)
    n = 6 * F
    pt_act = np.zeros(P, bool)
    pt_act[apt] = True
    M = Hll[apt].copy()
    M[:, range(3), range(3)] += lam
    Dinv = np.zeros((P, 3, 3))
    Dinv[apt] = inverse3(M, inv3)
    db = np.stack([Dinv[:, a, 0] * bl[:, 0] + Dinv[:, a, 1] * bl[:, 1] + Dinv[:, a, 2] * bl[:, 2]
                   for a in range(3)], axis=1)
    S = np.zeros((n, n))
    for f in range(F):
        S[6 * f:6 * f + 6, 6 * f:6 * f + 6] = Hpp[f]
    S[range(n), range(n)] += lam
    pts = sorted(by_pt)
    if order == "reversed":
        pts = pts[::-1]
    for j in pts:
        es = by_pt[j]
        Wj = W[es]                               # [m, 3, 6]
        D = Dinv[j]
        BD = (Wj[:, 0, :, None] * D[0][None, None, :] + Wj[:, 1, :, None] * D[1][None, None, :]
              + Wj[:, 2, :, None] * D[2][None, None, :])                          # [m, 6, 3]
        blk = (BD[:, None, :, 0, None] * Wj[None, :, 0, None, :] + BD[:, None, :, 1, None] * Wj[None, :, 1, None, :]
               + BD[:, None, :, 2, None] * Wj[None, :, 2, None, :])               # [m, m, 6, 6]
        rows = (6 * ef[es][:, None] + np.arange(6)[None, :]).reshape(-1)
        big = blk.transpose(0, 2, 1, 3).reshape(len(rows), len(rows))
        S[np.ix_(rows, rows)] -= big
    coef = group_sum(np.stack([W[fe][:, 0, r] * db[E.pt[fe], 0] + W[fe][:, 1, r] * db[E.pt[fe], 1]
                               + W[fe][:, 2, r] * db[E.pt[fe], 2] for r in range(6)], axis=1),
                     ef[fe], F, order, "kf").reshape(n)
    bs = bp - coef
    sol, piv = ldlt_solve(S, bs, perm)
    if sol is None:
        return None, None, piv
    xp = sol
    cl = bl.copy()
    tcl = np.zeros((E.n, 3))
    cp = -xp.reshape(F, 6)
    for a in range(3):
        acc = W[fe][:, a, 0] * cp[ef[fe], 0]
        for c in range(1, 6):
            acc = acc + W[fe][:, a, c] * cp[ef[fe], c]
        tcl[fe, a] = acc
    for e in fe:                             # edge order within each point
        cl[E.pt[e]] = cl[E.pt[e]] + tcl[e]
    xl = np.stack([Dinv[:, a, 0] * cl[:, 0] + Dinv[:, a, 1] * cl[:, 1] + Dinv[:, a, 2] * cl[:, 2]
                   for a in range(3)], axis=1)
    xl[~pt_act] = 0.0
    return xp, xl, piv


class State:
    def __init__(self, q, t, X):
        self.q, self.t, self.X = q, t, X

    def R(self):
        return np.stack([quat_to_matrix(q) for q in self.q]) if len(self.q) else np.zeros((0, 3, 3))


def optimize(E, cam, st, fixed, level, robust, iters, order, inv3, perm, log):
    """SparseOptimizer::optimize(iters) on the level-0 edges.  Returns the estimates, the chi2
    of every edge at the last computeActiveErrors (nan where not active), iterations, trials."""
    act = ~level
    K, P = len(st.q), len(st.X)
    chi_last = np.full(E.n, np.nan)
    kf_cnt = np.bincount(E.kf[act], minlength=K)
    free_rows = np.nonzero(~fixed & (kf_cnt > 0))[0]
    F = len(free_rows)
    fidx = np.full(K, -1)
    fidx[free_rows] = np.arange(F)
    pt_act = np.bincount(E.pt[act], minlength=P) > 0
    log["active_kf"].append(free_rows.tolist())
    log["active_pt"].append(np.nonzero(pt_act)[0].tolist())
    if not act.any() or F == 0:
        log["accepts"].append([])
        log["stop"].append("noactive")
        log["decisions"].append([])
        return st, chi_last, 0, 0
    ae = np.nonzero(act)[0]
    ef = fidx[E.kf]                                          # S block of every edge, -1: fixed
    n = 6 * F
    accepts, decisions = [], []
    stop = "iterations"
    lam = ni = 0.0
    nbad = its = 0
    xp, xl = np.zeros(n), np.zeros((P, 3))
    apt = np.nonzero(pt_act)[0]

    def chi_of(s):
        err, _ = edge_errors(E, cam, s.q, s.t, s.X)
        c2 = edge_chi2(E, err)
        chi_last[ae] = c2[ae]
        rho0, _ = huber(E, c2, robust)
        return float(osum(rho0[ae], order, owner=E.pt[ae] % THREADS))

    with np.errstate(all="ignore"):
        for it in range(iters):
            chi, c2, Hll, bl, Hpp, bp, W, fe = linearize(E, cam, st, ae, ef, F, robust, order)
            chi_last[ae] = c2[ae]
            ini_chi = chi
            if it == 0:                                      # computeLambdaInit
                md = 0.0
                if F:
                    md = max(md, float(np.abs(Hpp[:, range(6), range(6)]).max()))
                md = max(md, float(np.abs(Hll[apt][:, range(3), range(3)]).max()))
                lam = 1e-5 * md
                ni = 2.0
                nbad = 0
            # edges of every active point that reach S, in edge order
            by_pt = {}
            for e in fe:
                by_pt.setdefault(int(E.pt[e]), []).append(int(e))
            qmax = 0
            rho = 0.0
            while True:
                sol, xl_new, piv = schur_solve(E, ef, fe, by_pt, Hll, bl, Hpp, bp, W, lam, apt, order, inv3, perm)
                log["min_pivot"] = min(log["min_pivot"], float(np.min(piv)))
                ok = sol is not None
                if ok:
                    xp, xl = sol, xl_new
                tq, tt = st.q.copy(), st.t.copy()
                for f, k in enumerate(free_rows):
                    tq[k], tt[k] = se3_mul(se3_exp(xp[6 * f:6 * f + 6]), (st.q[k], st.t[k]))
                tX = st.X.copy()
                tX[apt] = st.X[apt] + xl[apt]
                trial = State(tq, tt, tX)
                temp = chi_of(trial)
                if not ok:
                    temp = DBL_MAX
                rho = chi - temp
                decisions.append(rho)
                if order == "kernel":                        # thread t: keyframe t, then its points
                    terms = [xp.reshape(F, 6)[:, r] * (lam * xp.reshape(F, 6)[:, r] + bp.reshape(F, 6)[:, r]) for r in range(6)]
                    seq = np.stack(terms, axis=1).reshape(-1)
                    own = np.repeat(np.arange(F) % THREADS, 6)
                    pseq = (xl[apt] * (lam * xl[apt] + bl[apt])).reshape(-1)
                    scale = float(osum(np.concatenate([seq, pseq]), "kernel",
                                       owner=np.concatenate([own, np.repeat(apt % THREADS, 3)])))
                else:
                    allx = np.concatenate([xp, xl[apt].reshape(-1)])
                    allb = np.concatenate([bp, bl[apt].reshape(-1)])
                    scale = float(osum(allx * (lam * allx + allb), order))
                scale += 1e-3
                rho = rho / scale
                if rho > 0 and np.isfinite(temp):
                    tt3 = 2.0 * rho - 1.0
                    alpha = min(1.0 - tt3 * tt3 * tt3, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    chi = temp
                    st = trial
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
            decisions.append((ini_chi - chi) * 1e3 - ini_chi)
            if (ini_chi - chi) * 1e3 < ini_chi:
                nbad += 1
            else:
                nbad = 0
            if nbad >= 3:
                stop = "nbad"
                break
    log["accepts"].append(accepts)
    log["stop"].append(stop)
    log["decisions"].append(decisions)
    return st, chi_last, its, len(accepts)


def local_ba(sc, order="forward", inv3="cofactor", perm="natural", max_free=MAX_FREE_KF):
    """Optimizer::LocalBundleAdjustment.  Returns a dict: Tcw [K, 12] and pos [P, 3] float32,
    erase / level1 [n_obs] uint8, n_erase, trace [2, 2], status, and what guard() reads."""
    cam = tuple(float(np.float32(v)) for v in sc["cam"])
    Tcw = np.asarray(sc["Tcw"], np.float32).reshape(-1, 12)
    pos = np.asarray(sc["pos"], np.float32).reshape(-1, 3)
    fixed = np.asarray(sc["fixed"]).astype(bool)
    K, nobs = len(fixed), len(sc["obs_kf"])
    out = dict(Tcw=Tcw.copy(), pos=pos.copy(), erase=np.zeros(nobs, np.uint8), level1=np.zeros(nobs, np.uint8),
               n_erase=0, trace=np.zeros((2, 2), np.int32), status=0, accepts=[], stop=[], decisions=[], chi2=[],
               depth=[], stereo=np.zeros(0, bool), active_kf=[], active_pt=[], min_pivot=np.inf,
               Tcw64=Tcw.astype(np.float64), pos64=pos.astype(np.float64))
    nfree = int((~fixed).sum())
    if nfree == 0 or nfree > min(max_free, MAX_FREE_KF):
        out["status"] = STATUS_NO_FREE_KF if nfree == 0 else STATUS_CAPACITY
        return out
    E = Edges(sc)
    out["stereo"] = E.stereo
    if E.bad_index:
        out["status"] |= STATUS_BAD_INDEX
    poses = [se3_from_tcw(T) for T in Tcw]
    st = State(np.array([p[0] for p in poses]), np.array([p[1] for p in poses]), pos.astype(np.float64))
    level = np.zeros(E.n, bool)
    chi_kept = np.zeros(E.n)
    thr = np.where(E.stereo, CHI2_STEREO, CHI2_MONO)
    for phase, iters in enumerate((5, 10)):
        st, chi_last, its, trials = optimize(E, cam, st, fixed, level, phase == 0, iters, order, inv3, perm, out)
        out["trace"][phase] = (its, trials)
        upd = ~np.isnan(chi_last)
        chi_kept[upd] = chi_last[upd]
        z = (quat_rotate_v(st.q[E.kf], st.X[E.pt]) + st.t[E.kf])[:, 2]
        with np.errstate(all="ignore"):
            bad = (chi_kept > thr) | ~(z > 0.0)
        out["chi2"].append(chi_kept.copy())
        out["depth"].append(z)
        if phase == 0:
            level = bad
            out["level1"][E.index] = bad
        else:
            out["erase"][E.index] = bad
            out["n_erase"] = int(bad.sum())
    T64 = Tcw.astype(np.float64)
    for k in range(K):
        if not fixed[k]:
            out["Tcw"][k] = se3_to_tcw(st.q[k], st.t[k])
            T64[k] = np.concatenate([quat_to_matrix(st.q[k]), st.t[k][:, None]], axis=1).reshape(12)
    out["Tcw64"] = T64
    out["pos64"] = st.X
    out["pos"] = st.X.astype(np.float32)
    return out


VARIANTS = (("forward", "cofactor", "natural"), ("reversed", "cofactor", "natural"), ("pairwise", "cofactor", "natural"),
            ("kernel", "cofactor", "natural"), ("forward", "ldlt", "natural"), ("forward", "cofactor", "reversed"),
            ("forward", "cofactor", 12345))


def variants(sc):
    return [local_ba(sc, o, i, p) for o, i, p in VARIANTS]


def guard(vs):
    """The conditions on a scene: all variants agree on the whole trace, on every level and
    erase flag and on the active sets; every LDL^T pivot is positive; every chi2 at both
    classifications is further from its threshold, and every tested depth further from 0, than
    1000 x the largest difference between the variants.  Returns (ok, text)."""
    a = vs[0]
    for v in vs[1:]:
        if v["accepts"] != a["accepts"] or v["stop"] != a["stop"] or not np.array_equal(v["trace"], a["trace"]):
            return False, "LM traces differ"
        if not np.array_equal(v["level1"], a["level1"]) or not np.array_equal(v["erase"], a["erase"]):
            return False, "flags differ"
        if v["active_kf"] != a["active_kf"] or v["active_pt"] != a["active_pt"] or v["status"] != a["status"]:
            return False, "active sets differ"
    if not all(v["min_pivot"] > 0 for v in vs):
        return False, "a pivot is not positive"
    if not a["chi2"] or len(a["stereo"]) == 0:
        return True, "no edges"
    thr = np.where(a["stereo"], CHI2_STEREO, CHI2_MONO)
    txt = []
    for key, ref in (("chi2", thr), ("depth", 0.0)):
        spread, margin = 0.0, np.inf
        for r in range(2):
            c = np.stack([v[key][r] for v in vs])
            if not np.isfinite(c).all():
                return False, f"non-finite {key}"
            spread = max(spread, float((c.max(axis=0) - c.min(axis=0)).max()))
            margin = min(margin, float(np.abs(c - ref).min()))
        if not margin > 1000.0 * spread:
            return False, f"{key} margin {margin:g} within 1000 x spread {spread:g}"
        txt.append(f"{key} margin {margin:g}, spread {spread:g}")
    return True, "; ".join(txt)


def spread(vs):
    """(largest pose-entry difference, largest position-entry difference) between the variants."""
    T = np.stack([v["Tcw64"] for v in vs])
    X = np.stack([v["pos64"] for v in vs])
    return (float((T.max(axis=0) - T.min(axis=0)).max()) if T.size else 0.0,
            float((X.max(axis=0) - X.min(axis=0)).max()) if X.size else 0.0)


# ---- scenes --------------------------------------------------------------------------------------

SIZE = (640, 480)


def make_scene(seed, n_free=2, n_fixed=1, n_pts=30, kind="mixed", max_obs=None, n_edges=None, noise=1.0,
               outlier_frac=0.0, off_deg=0.3, off_m=0.02, off_pt=0.02, kf0_fixed=False, single_obs=False, no_obs=False,
               idle_fixed=False, behind=False, starve_pt=False, starve_kf=False, cap=None, baseline=0.25):
    """A local map: n_free + n_fixed keyframes (free first) looking at n_pts points 3-8 m away.
    Keypoint rows and keyframe slots are dealt out of storage order.  n_edges trims the
    observations to an exact count.  single_obs / no_obs: the last point(s) keep one / no
    observation; idle_fixed: an extra fixed keyframe without an edge; behind: one point starts
    behind a camera; starve_pt / starve_kf: a point (a free keyframe) whose every observation is
    a 50 px outlier; kf0_fixed: the first keyframe of the local list is flagged fixed."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, bf = (float(np.float32(v)) for v in TUM1)
    K = n_free + n_fixed + (1 if idle_fixed else 0)
    fixed = np.zeros(K, bool)
    fixed[n_free:] = True
    if kf0_fixed:
        fixed[0] = True
    Rs = [rot(rng.normal(size=3) * 0.04) for _ in range(K)]
    ts = [rng.normal(size=3) * baseline for _ in range(K)]
    u = rng.uniform(120, SIZE[0] - 120, n_pts)
    v = rng.uniform(100, SIZE[1] - 100, n_pts)
    z = rng.uniform(3.0, 8.0, n_pts)
    Xw = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=1)
    cap = cap or max(n_pts + 3, 8)
    n_slots = K + 2
    slot = rng.permutation(n_slots)[:K].astype(np.int32)
    kps_xy = np.zeros((n_slots, cap, 2), np.float32)
    kps_oct = np.zeros((n_slots, cap), np.int32)
    u_right = np.full((n_slots, cap), -1.0, np.float32)
    rows = [list(rng.permutation(cap)) for _ in range(K)]
    obs_off, obs_kf, obs_kp, gross = [0], [], [], []
    n_real = K - (1 if idle_fixed else 0)
    for j in range(n_pts):
        ks = list(rng.permutation(n_real))
        if max_obs:
            ks = ks[:max(1, int(rng.integers(max(1, max_obs // 2), max_obs + 1)))]
        if single_obs and j == n_pts - 1:
            ks = [0 if not fixed[0] else 1]
        if no_obs and j == n_pts - (2 if single_obs else 1):
            ks = []
        for k in ks:
            Xc = Rs[k] @ Xw[j] + ts[k]
            if Xc[2] < 0.5:
                continue
            pu, pv = fx * Xc[0] / Xc[2] + cx, fy * Xc[1] / Xc[2] + cy
            if not (5 < pu < SIZE[0] - 5 and 5 < pv < SIZE[1] - 5):
                continue
            octv = int(rng.integers(0, 8))
            s = 1.2 ** octv
            pur = pu - bf / Xc[2]
            mono = kind == "mono" or (kind == "mixed" and rng.integers(0, 3) == 0)
            g = rng.uniform() < outlier_frac or (starve_pt and j == 0) or (starve_kf and k == n_free - 1)
            du, dv = rng.normal(size=2) * noise * s
            dr = rng.normal() * noise * s
            if g:
                ang = rng.uniform(0, 2 * np.pi)
                du, dv, dr = du + 50 * np.cos(ang), dv + 50 * np.sin(ang), dr + 50 * np.cos(ang)
            kp = int(rows[k].pop())
            kps_xy[slot[k], kp] = (pu + du, pv + dv)
            kps_oct[slot[k], kp] = octv
            u_right[slot[k], kp] = -1.0 if mono else max(pur + dr, 0.0)
            obs_kf.append(k)
            obs_kp.append(kp)
            gross.append(g)
        obs_off.append(len(obs_kf))
    if n_edges is not None:                                  # trim from the last points
        assert len(obs_kf) >= n_edges, (len(obs_kf), n_edges)
        obs_kf, obs_kp, gross = obs_kf[:n_edges], obs_kp[:n_edges], gross[:n_edges]
        obs_off = [min(o, n_edges) for o in obs_off]
    Tcw = np.zeros((K, 12), np.float32)
    Ttrue = np.zeros((K, 12))
    for k in range(K):
        T = np.concatenate([Rs[k], ts[k][:, None]], axis=1)
        Ttrue[k] = T.reshape(12)
        if not fixed[k]:
            ax = rng.normal(size=3)
            ax /= np.linalg.norm(ax)
            dR = rot(ax * np.deg2rad(off_deg))
            dt = rng.normal(size=3)
            dt *= off_m / np.linalg.norm(dt)
            T = np.concatenate([dR @ Rs[k], (dR @ ts[k] + dt)[:, None]], axis=1)
        Tcw[k] = T.reshape(12).astype(np.float32)
    pos = (Xw + rng.normal(size=Xw.shape) * off_pt).astype(np.float32)
    if behind:                                               # the second point starts behind keyframe 0
        pos[1] = (Rs[0].T @ (np.array([0.1, 0.1, -2.0]) - ts[0])).astype(np.float32)
    return dict(cam=(fx, fy, cx, cy, bf), Tcw=Tcw, fixed=fixed.astype(np.uint8), slot=slot, pos=pos,
                obs_off=np.asarray(obs_off, np.int32), obs_kf=np.asarray(obs_kf, np.int32),
                obs_kp=np.asarray(obs_kp, np.int32), kps_xy=kps_xy, kps_oct=kps_oct,
                u_right=None if kind == "mono" else u_right, inv_sigma2=INV_SIGMA2, Tcw_true=Ttrue, pos_true=Xw,
                gross=np.asarray(gross, bool), kind=kind)


# name -> make_scene arguments: the smallest scenes at which each piece can go wrong
SPECS = {
    "1+1-6pts": dict(n_free=1, n_fixed=1, n_pts=6),
    "2+0-kf0": dict(n_free=2, n_fixed=0, n_pts=12, kf0_fixed=True),
    "mono": dict(n_free=2, n_fixed=2, n_pts=24, kind="mono"),
    "stereo": dict(n_free=2, n_fixed=1, n_pts=24, kind="stereo"),
    "mixed": dict(n_free=3, n_fixed=2, n_pts=30),
    "single-obs": dict(n_free=2, n_fixed=1, n_pts=16, single_obs=True, no_obs=True, idle_fixed=True),
    "out10-starve-pt": dict(n_free=3, n_fixed=2, n_pts=40, outlier_frac=0.1, behind=True, starve_pt=True),
    "out10-starve-kf": dict(n_free=3, n_fixed=2, n_pts=40, outlier_frac=0.1, starve_kf=True),
    "edges-63": dict(n_free=3, n_fixed=2, n_pts=20, n_edges=63),
    "edges-64": dict(n_free=3, n_fixed=2, n_pts=20, n_edges=64),
    "edges-65": dict(n_free=3, n_fixed=2, n_pts=20, n_edges=65),
    "edges-255": dict(n_free=4, n_fixed=4, n_pts=40, n_edges=255),
    "edges-256": dict(n_free=4, n_fixed=4, n_pts=40, n_edges=256),
    "edges-257": dict(n_free=4, n_fixed=4, n_pts=40, n_edges=257),
    "pts-1": dict(n_free=1, n_fixed=2, n_pts=1, kind="stereo"),
    "pts-257": dict(n_free=2, n_fixed=2, n_pts=257, max_obs=3),
    "kf-cap": dict(n_free=MAX_FREE_KF, n_fixed=2, n_pts=40, kind="stereo", max_obs=8, baseline=0.15),
}
# seeds: the first for which guard() holds (python tests/local_ba_spread.py --find prints them)
SEEDS = {name: 0 for name in SPECS}
SEEDS.update({"out10-starve-kf": 1})


def scene(name, seed=None):
    return make_scene(SEEDS[name] if seed is None else seed, **SPECS[name])


def scene_extra(name, r):
    """What a scene must show beyond its guard."""
    if name == "out10-starve-pt":      # a point without a level-0 edge in the second optimisation
        return len(r["active_pt"][1]) < len(r["active_pt"][0]) and r["level1"].any()
    if name == "out10-starve-kf":      # a free keyframe without one
        return len(r["active_kf"][1]) < len(r["active_kf"][0])
    return True


# ---- batch arrays (the GPU tests and benchmarks/localba_bench.py) --------------------------------

def batch_arrays(scenes):
    """Concatenate scenes of one keypoint capacity into the tables of orbx_local_ba_batch."""
    cap = max(s["kps_xy"].shape[1] for s in scenes)
    kf_off, pt_off, obs_off = [0], [0], [0]
    Tcw, fixed, slot, pos, okf, okp, xy, octv, ur = [], [], [], [], [], [], [], [], []
    nslots = 0
    for s in scenes:
        ns, c = s["kps_xy"].shape[:2]
        Tcw.append(s["Tcw"])
        fixed.append(s["fixed"])
        slot.append(s["slot"] + nslots)
        pos.append(s["pos"])
        obs_off.extend((s["obs_off"][1:] + obs_off[-1]).tolist())
        okf.append(s["obs_kf"])
        okp.append(s["obs_kp"])
        pad = ((0, 0), (0, cap - c))
        xy.append(np.pad(s["kps_xy"], pad + ((0, 0),)))
        octv.append(np.pad(s["kps_oct"], pad))
        ur.append(np.pad(s["u_right"] if s["u_right"] is not None else np.full((ns, c), -1.0, np.float32), pad,
                         constant_values=-1.0))
        nslots += ns
        kf_off.append(kf_off[-1] + len(s["fixed"]))
        pt_off.append(pt_off[-1] + len(s["pos"]))
    cat = np.concatenate
    return dict(kf_off=np.asarray(kf_off, np.int32), pt_off=np.asarray(pt_off, np.int32),
                obs_off=np.asarray(obs_off, np.int32), Tcw=cat(Tcw).astype(np.float32), fixed=cat(fixed).astype(np.uint8),
                slot=cat(slot).astype(np.int32), pos=cat(pos).astype(np.float32).reshape(-1, 3),
                obs_kf=cat(okf).astype(np.int32), obs_kp=cat(okp).astype(np.int32), kps_xy=cat(xy), kps_oct=cat(octv),
                u_right=cat(ur), cap=cap, n_slots=nslots)
