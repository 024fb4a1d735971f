"""A float64 numpy restatement of PnPsolver (src/PnPsolver.cc:80-1345) under the conventions of
csrc/orbx_epnp.h, operation for operation: every sum runs in index order, nothing is fused.
tests/test_pnp_model.py checks the header compiled for the host against it bit for bit;
tests/test_gpu_pnp.py compares the device with it.

Two families of variants say which outputs may be compared, and how closely:

  Family A, arithmetic under the device's conventions (ARITH):
    "jacobi"    the model proper: the device's one-sided Jacobi everywhere
    "numpy"     numpy's eigh / svd / lstsq in place of every Jacobi; each eigenvector's sign is
                aligned to the Jacobi's, and for minimal sets (a 4-fold null space) the Jacobi's
                null vectors are projected onto eigh's null space
    "reversed"  the M^T M and centroid sums run from the last point to the first
    "lstsq"     qr_solve replaced by numpy's lstsq
    "flip"      every rep_errors comparison between two solutions that are the same pose (entries
                closer than SAME_POSE) decided the other way: such a comparison is between numbers
                equal up to rounding, and this variant carries the other outcome through
                CheckInliers and everything after

  Family B, conventions (CONVENTIONS), all with the Jacobi arithmetic:
    "pca0" "pca1" "pca2"          one PCA axis of choose_control_points negated
    "null0" .. "null3"            one null vector negated
    "nullrot"                     for minimal sets, the four null vectors multiplied by a fixed
                                  seeded orthogonal 4x4 (Refine's eigenvalues are distinct:
                                  nothing beyond signs applies there)
"""
from __future__ import annotations

import math

import numpy as np

EPS = 2.220446049250313e-16
TOL = 8.0 * EPS
SWEEPS = 30
ARITH = ("jacobi", "numpy", "reversed", "lstsq", "flip")
SAME_POSE = 1e-9   # two of compute_pose's solutions count as one pose when their entries are closer than this
CONVENTIONS = ("pca0", "pca1", "pca2", "null0", "null1", "null2", "null3", "nullrot")
STATUS_BAD_DRAW, STATUS_NO_DRAWS = 1, 2
F64 = np.float64
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
_NULLROT = np.linalg.qr(np.random.default_rng(20241).standard_normal((4, 4)))[0]


def _lstsq(a, b):
    """numpy's least squares; NaN where LAPACK gives up (non-finite input)."""
    try:
        return np.linalg.lstsq(a, b, rcond=None)[0]
    except np.linalg.LinAlgError:
        return np.full(a.shape[1], np.nan)


def _eigh(a):
    try:
        return np.linalg.eigh(a)
    except np.linalg.LinAlgError:
        return np.full(len(a), np.nan), np.full(a.shape, np.nan)


def seq(a):
    """The sum over the first axis in index order from 0.0."""
    a = np.asarray(a, F64)
    z = np.zeros((1,) + a.shape[1:], F64)
    return np.cumsum(np.concatenate([z, a], axis=0), axis=0)[-1]


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def hestenes(a):
    """A V = B by the cyclic one-sided Jacobi: (B, V)."""
    a = np.array(a, F64)
    rows, n = a.shape
    v = np.eye(n)
    for _ in range(SWEEPS):
        rot = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                x, y = a[:, p].copy(), a[:, q].copy()
                alpha, beta, gamma = seq(x * x), seq(y * y), seq(x * y)
                if gamma == 0.0 or abs(gamma) <= TOL * np.sqrt(alpha * beta):
                    continue
                zeta = (beta - alpha) / (2.0 * gamma)
                t = np.copysign(1.0, zeta) / (abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                c = 1.0 / np.sqrt(1.0 + t * t)
                sn = c * t
                a[:, p], a[:, q] = c * x - sn * y, sn * x + c * y
                x, y = v[:, p].copy(), v[:, q].copy()
                v[:, p], v[:, q] = c * x - sn * y, sn * x + c * y
                rot = True
        if not rot:
            break
    return a, v


def col_norm2(b, c):
    return seq(b[:, c] * b[:, c])


def lsq6(L, rho, arith):
    """cvSolve(L, rho, CV_SVD)."""
    if arith == "numpy":
        return _lstsq(L, rho)
    b, v = hestenes(L)
    nc = L.shape[1]
    s = F64(0.0)
    for j in range(nc):
        s = s + np.sqrt(col_norm2(b, j))
    thr = 2.0 * EPS * s
    x = np.zeros(nc)
    for j in range(nc):
        w2 = col_norm2(b, j)
        if not (np.sqrt(w2) > thr):
            continue
        coef = seq(b[:, j] * rho) / w2
        x = x + v[:, j] * coef
    return x


def qr_solve(a, b, x):
    """qr_solve (cc:1211-1345) on the 6x4 a and b; returns x, unchanged after the eta == 0 return."""
    a, b, x = np.array(a, F64), np.array(b, F64), np.array(x, F64)
    nr, nc = a.shape
    A1, A2 = np.zeros(nc), np.zeros(nc)
    for k in range(nc):
        eta = abs(a[k, k])
        for i in range(k, nr - 1):   # cc:1242-1247: the last row is never looked at
            elt = abs(a[i, k])
            if eta < elt:
                eta = elt
        if eta == 0.0:
            return x
        inv_eta = 1.0 / eta
        s = F64(0.0)
        for i in range(k, nr):
            a[i, k] = a[i, k] * inv_eta
            s = s + a[i, k] * a[i, k]
        sigma = np.sqrt(s)
        if a[k, k] < 0.0:
            sigma = -sigma
        a[k, k] = a[k, k] + sigma
        A1[k] = sigma * a[k, k]
        A2[k] = -eta * sigma
        for j in range(k + 1, nc):
            s = F64(0.0)
            for i in range(k, nr):
                s = s + a[i, k] * a[i, j]
            tau = s / A1[k]
            for i in range(k, nr):
                a[i, j] = a[i, j] - tau * a[i, k]
    for j in range(nc):
        tau = F64(0.0)
        for i in range(j, nr):
            tau = tau + a[i, j] * b[i]
        tau = tau / A1[j]
        for i in range(j, nr):
            b[i] = b[i] - tau * a[i, j]
    x[nc - 1] = b[nc - 1] / A2[nc - 1]
    for i in range(nc - 2, -1, -1):
        s = F64(0.0)
        for j in range(i + 1, nc):
            s = s + a[i, j] * x[j]
        x[i] = (b[i] - s) / A2[i]
    return x


def gauss_newton(L, rho, betas, arith):
    betas = np.array(betas, F64)
    x = np.zeros(4)
    for _ in range(5):
        b0, b1, b2, b3 = betas
        l = L.T  # l[c] is column c over the six rows
        a = np.empty((6, 4))
        a[:, 0] = ((2.0 * l[0] * b0 + l[1] * b1) + l[3] * b2) + l[6] * b3
        a[:, 1] = ((l[1] * b0 + 2.0 * l[2] * b1) + l[4] * b2) + l[7] * b3
        a[:, 2] = ((l[3] * b0 + l[4] * b1) + 2.0 * l[5] * b2) + l[8] * b3
        a[:, 3] = ((l[6] * b0 + l[7] * b1) + l[8] * b2) + 2.0 * l[9] * b3
        s = l[0] * b0 * b0
        s = s + l[1] * b0 * b1
        s = s + l[2] * b1 * b1
        s = s + l[3] * b0 * b2
        s = s + l[4] * b1 * b2
        s = s + l[5] * b2 * b2
        s = s + l[6] * b0 * b3
        s = s + l[7] * b1 * b3
        s = s + l[8] * b2 * b3
        s = s + l[9] * b3 * b3
        b = rho - s
        if arith == "lstsq":
            x = _lstsq(a, b)
        else:
            x = qr_solve(a, b, x)
        betas = betas + x
    return betas


def rotation_of(A, arith):
    """R = U V^T of the 3x3 A (cc:824-829)."""
    if arith == "numpy":
        try:
            u, _, vt = np.linalg.svd(A)
        except np.linalg.LinAlgError:
            return np.full((3, 3), np.nan)
        return u @ vt
    B, V = hestenes(A)
    w = np.array([np.sqrt((B[0, c] * B[0, c] + B[1, c] * B[1, c]) + B[2, c] * B[2, c]) for c in range(3)])
    for p, q in ((0, 1), (1, 2), (0, 1)):
        if w[p] < w[q]:
            w[[p, q]] = w[[q, p]]
            B[:, [p, q]] = B[:, [q, p]]
            V[:, [p, q]] = V[:, [q, p]]
    U = np.empty((3, 3))
    U[:, 0] = B[:, 0] / w[0]
    U[:, 1] = B[:, 1] / w[1]
    c = np.array([U[1, 0] * U[2, 1] - U[2, 0] * U[1, 1], U[2, 0] * U[0, 1] - U[0, 0] * U[2, 1],
                  U[0, 0] * U[1, 1] - U[1, 0] * U[0, 1]])
    if (c[0] * B[0, 2] + c[1] * B[1, 2]) + c[2] * B[2, 2] < 0.0:
        c = -c
    U[:, 2] = c
    R = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            R[i, j] = dot3(U[i], V[j])
    return R


def compute_R_and_t(pws, us, alphas, vv, betas, K, arith):
    fu, fv, uc, vc = K
    n = len(pws)
    ccs = np.zeros(12)
    for i in range(4):
        ccs = ccs + betas[i] * vv[i]
    ccs = ccs.reshape(4, 3)
    a = alphas
    pcs = ((a[:, 0:1] * ccs[0] + a[:, 1:2] * ccs[1]) + a[:, 2:3] * ccs[2]) + a[:, 3:4] * ccs[3]
    if pcs[0, 2] < 0.0:
        pcs = -pcs
    dn = F64(n)
    pc0, pw0 = seq(pcs) / dn, seq(pws) / dn
    dc, dw = pcs - pc0, pws - pw0
    abt = seq(dc[:, :, None] * dw[:, None, :])
    R = rotation_of(abt, arith)
    det = ((((R[0, 0] * R[1, 1] * R[2, 2] + R[0, 1] * R[1, 2] * R[2, 0]) + R[0, 2] * R[1, 0] * R[2, 1]) -
            R[0, 2] * R[1, 1] * R[2, 0]) - R[0, 1] * R[1, 0] * R[2, 2]) - R[0, 0] * R[1, 2] * R[2, 1]
    if det < 0.0:
        R[2] = -R[2]
    t = np.array([pc0[i] - dot3(R[i], pw0) for i in range(3)])
    X = pws.T
    Xc = dot3(R[0], X) + t[0]
    Yc = dot3(R[1], X) + t[1]
    inv = 1.0 / (dot3(R[2], X) + t[2])
    ue, ve = uc + fu * Xc * inv, vc + fv * Yc * inv
    du, dv = us[:, 0] - ue, us[:, 1] - ve
    return R, t, seq(np.sqrt(du * du + dv * dv)) / dn


def _order(w2, smallest):
    """Column indices by value: descending with the lower index first on a tie, or the
    `smallest` smallest, smallest first, the higher index first on a tie."""
    w2 = list(w2)
    if smallest:
        out, taken = [], set()
        for _ in range(smallest):
            bc, best = -1, 0.0
            for c in range(len(w2)):
                if c in taken:
                    continue
                if bc < 0 or w2[c] <= best:
                    best, bc = w2[c], c
            taken.add(bc)
            out.append(bc)
        return out
    o, d = [0, 1, 2], list(w2)
    for p, q in ((0, 1), (1, 2), (0, 1)):
        if d[p] < d[q]:
            d[p], d[q] = d[q], d[p]
            o[p], o[q] = o[q], o[p]
    return o


def compute_pose(pws, us, K, arith="jacobi", conv=None, trace=None, base=None, basis=None):
    """compute_pose (cc:644-719): (R (3, 3), t (3,), reprojection error).  `basis`, a dict, receives
    the PCA axes and the null vectors used; `base` is such a dict from the Jacobi variant, which
    a family-A variant aligns its own to: each vector's sign, and for a minimal set (a 4-fold
    null space, whose basis is decided by rounding noise) the base's null vectors projected onto
    the variant's null space."""
    with np.errstate(all="ignore"):
        return _compute_pose(np.array(pws, F64).reshape(-1, 3), np.array(us, F64).reshape(-1, 2),
                             [F64(k) for k in K], arith, conv, trace, base, basis)


def _align(own, ref):
    return own if own @ ref >= 0 else -own


def _compute_pose(pws, us, K, arith, conv, trace, base, basis):
    fu, fv, uc, vc = K
    n = len(pws)
    dn = F64(n)
    rev = arith == "reversed"
    c0 = (seq(pws[::-1]) if rev else seq(pws)) / dn
    d = pws - c0
    m = seq(np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2],
                      d[:, 2] * d[:, 2]], axis=1))
    P = np.array([[m[0], m[1], m[2]], [m[1], m[3], m[4]], [m[2], m[4], m[5]]])
    B, V = hestenes(P)
    w = [np.sqrt(col_norm2(B, c)) for c in range(3)]
    o = _order(w, 0)
    dcs = [w[i] for i in o]
    uct = np.array([V[:, i] for i in o])
    if arith == "numpy":
        ev, evec = _eigh(P)
        for r in range(3):
            uct[r] = _align(evec[:, 2 - r], uct[r])
            dcs[r] = max(ev[2 - r], 0.0)
    if base is not None:
        for r in range(3):
            uct[r] = _align(uct[r], base["uct"][r])
    if conv in ("pca0", "pca1", "pca2"):
        uct[int(conv[3])] = -uct[int(conv[3])]
    kk = [np.sqrt(dcs[i] / dn) for i in range(3)]
    cws = np.array([c0] + [c0 + kk[i] * uct[i] for i in range(3)])
    ci = np.array([np.zeros(3) if kk[j] == 0.0 else uct[j] / kk[j] for j in range(3)])
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    a1 = (ci[0, 0] * x + ci[0, 1] * y) + ci[0, 2] * z
    a2 = (ci[1, 0] * x + ci[1, 1] * y) + ci[1, 2] * z
    a3 = (ci[2, 0] * x + ci[2, 1] * y) + ci[2, 2] * z
    alphas = np.stack([((1.0 - a1) - a2) - a3, a1, a2, a3], axis=1)
    du, dv = uc - us[:, 0], vc - us[:, 1]
    M1, M2 = np.zeros((n, 12)), np.zeros((n, 12))
    for j in range(4):
        M1[:, 3 * j] = alphas[:, j] * fu
        M1[:, 3 * j + 2] = alphas[:, j] * du
        M2[:, 3 * j + 1] = alphas[:, j] * fv
        M2[:, 3 * j + 2] = alphas[:, j] * dv
    terms = np.empty((2 * n, 12, 12))
    terms[0::2] = M1[:, :, None] * M1[:, None, :]
    terms[1::2] = M2[:, :, None] * M2[:, None, :]
    if rev:
        terms = terms[::-1]
    MtM = seq(terms)
    MtM = np.triu(MtM) + np.triu(MtM, 1).T
    B, V = hestenes(MtM)
    vi = _order([col_norm2(B, c) for c in range(12)], 4)
    vv = np.array([V[:, i] for i in vi])
    if arith == "numpy":
        ev, evec = _eigh(MtM)
        if n == 4:   # a 4-fold null space: the Jacobi's vectors projected onto eigh's
            Nn = evec[:, :4]
            for k in range(4):
                pk = Nn @ (Nn.T @ vv[k])
                vv[k] = pk / np.linalg.norm(pk)
        else:
            for k in range(4):
                vv[k] = _align(evec[:, k], vv[k])
    if base is not None:
        if n == 4:
            Nn = np.linalg.qr(vv.T)[0]
            for k in range(4):
                pk = Nn @ (Nn.T @ base["vv"][k])
                vv[k] = pk / np.linalg.norm(pk)
        else:
            for k in range(4):
                vv[k] = _align(vv[k], base["vv"][k])
    if basis is not None:
        basis.update(uct=uct.copy(), vv=vv.copy())
    if conv in ("null0", "null1", "null2", "null3"):
        vv[int(conv[4])] = -vv[int(conv[4])]
    if conv == "nullrot" and n == 4:
        vv = _NULLROT @ vv
    L = np.empty((6, 10))
    for r, (pa, pb) in enumerate(PAIRS):
        dvs = [vv[i][3 * pa:3 * pa + 3] - vv[i][3 * pb:3 * pb + 3] for i in range(4)]
        L[r] = [dot3(dvs[0], dvs[0]), 2.0 * dot3(dvs[0], dvs[1]), dot3(dvs[1], dvs[1]), 2.0 * dot3(dvs[0], dvs[2]),
                2.0 * dot3(dvs[1], dvs[2]), dot3(dvs[2], dvs[2]), 2.0 * dot3(dvs[0], dvs[3]),
                2.0 * dot3(dvs[1], dvs[3]), 2.0 * dot3(dvs[2], dvs[3]), dot3(dvs[3], dvs[3])]
    rho = np.empty(6)
    for r, (pa, pb) in enumerate(PAIRS):
        e = cws[pa] - cws[pb]
        rho[r] = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    # N = 4
    b4 = lsq6(L[:, [0, 1, 3, 6]], rho, arith)
    betas = np.zeros(4)
    if b4[0] < 0.0:
        betas[0] = np.sqrt(-b4[0])
        betas[1:] = -b4[1:] / betas[0]
    else:
        betas[0] = np.sqrt(b4[0])
        betas[1:] = b4[1:] / betas[0]
    R, t, err = compute_R_and_t(pws, us, alphas, vv, gauss_newton(L, rho, betas, arith), K, arith)
    errs = [err]
    # N = 2
    b3 = lsq6(L[:, [0, 1, 2]], rho, arith)
    betas = np.zeros(4)
    if b3[0] < 0.0:
        betas[0] = np.sqrt(-b3[0])
        betas[1] = np.sqrt(-b3[2]) if b3[2] < 0.0 else 0.0
    else:
        betas[0] = np.sqrt(b3[0])
        betas[1] = np.sqrt(b3[2]) if b3[2] > 0.0 else 0.0
    if b3[1] < 0.0:
        betas[0] = -betas[0]
    Rn, tn, e = compute_R_and_t(pws, us, alphas, vv, gauss_newton(L, rho, betas, arith), K, arith)
    errs.append(e)
    same = max(np.abs(Rn - R).max(), np.abs(tn - t).max())
    if trace is not None:
        trace.append(("rep", e, err, same))
    if (e < err) != (arith == "flip" and same < SAME_POSE):
        R, t, err = Rn, tn, e
    # N = 3
    b5 = lsq6(L[:, [0, 1, 2, 3, 4]], rho, arith)
    betas = np.zeros(4)
    if b5[0] < 0.0:
        betas[0] = np.sqrt(-b5[0])
        betas[1] = np.sqrt(-b5[2]) if b5[2] < 0.0 else 0.0
    else:
        betas[0] = np.sqrt(b5[0])
        betas[1] = np.sqrt(b5[2]) if b5[2] > 0.0 else 0.0
    if b5[1] < 0.0:
        betas[0] = -betas[0]
    betas[2] = b5[3] / betas[0]
    Rn, tn, e = compute_R_and_t(pws, us, alphas, vv, gauss_newton(L, rho, betas, arith), K, arith)
    same = max(np.abs(Rn - R).max(), np.abs(tn - t).max())
    if trace is not None:
        trace.append(("rep", e, err, same))
    if (e < err) != (arith == "flip" and same < SAME_POSE):
        R, t, err = Rn, tn, e
    return R, t, err


def check_inliers(R, t, K, p3d, p2d, max_err, trace=None):
    """CheckInliers (cc:381-418) with its mixed precision: the flags."""
    f32 = np.float32
    fu, fv, uc, vc = (F64(k) for k in K)
    with np.errstate(all="ignore"):
        X, Y, Z = (p3d[:, i].astype(F64) for i in range(3))
        Xc = (((R[0, 0] * X + R[0, 1] * Y) + R[0, 2] * Z) + t[0]).astype(f32)
        Yc = (((R[1, 0] * X + R[1, 1] * Y) + R[1, 2] * Z) + t[1]).astype(f32)
        iz = (1.0 / (((R[2, 0] * X + R[2, 1] * Y) + R[2, 2] * Z) + t[2])).astype(f32)
        ue = uc + fu * Xc.astype(F64) * iz.astype(F64)
        ve = vc + fv * Yc.astype(F64) * iz.astype(F64)
        dx = (p2d[:, 0].astype(F64) - ue).astype(f32)
        dy = (p2d[:, 1].astype(F64) - ve).astype(f32)
        e2 = dx * dx + dy * dy
        assert e2.dtype == f32
        if trace is not None:
            trace.append(("err", e2.astype(F64) / max_err.astype(F64)))
        return e2 < max_err


def ransac_parameters(n, probability, min_inliers, max_iterations, min_set, epsilon):
    """SetRansacParameters (cc:141-183) at N = n: (mRansacMinInliers, mRansacMaxIts)."""
    f32 = np.float32
    nmin = int(f32(n) * f32(epsilon))
    nmin = max(nmin, min_inliers, min_set)
    if n < nmin or n <= 0:
        return nmin, 1
    eps = f32(epsilon)
    if eps < f32(nmin) / f32(n):
        eps = f32(nmin) / f32(n)
    if nmin == n:
        its = 1
    else:
        v = math.log(1 - probability) / math.log(1 - math.pow(float(eps), 3.0))
        its = max_iterations if not (v <= max_iterations) else int(math.ceil(v))
    return nmin, max(1, min(its, max_iterations))


def select4(draw, N):
    """The swap-with-last selection of cc:237-250; None if a draw is out of range."""
    avail = list(range(N))
    out = []
    for j in range(4):
        r = int(draw[j])
        if r < 0 or r >= len(avail) or len(avail) == 0:
            return None
        out.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return out


class PnPModel:
    """The solver for one candidate.  keys_xy (n, 2) f32, octaves (n,), matches (n,) MapPoint ids,
    mp_pos (n_mp, 3) f32, level_sigma2 (nlevels,) f32, K = fx fy cx cy (f32)."""

    def __init__(self, keys_xy, octaves, matches, mp_pos, level_sigma2, K, arith="jacobi", conv=None, base=None):
        f32 = np.float32
        self.arith, self.conv = arith, conv
        self.base = base        # the Jacobi variant's `basis`, for the family-A variants
        self.basis = {}         # per set of correspondences: the PCA axes and null vectors used
        matches = np.asarray(matches, np.int64)
        self.n = len(matches)
        self.matches = matches
        pos = np.asarray(mp_pos, f32).reshape(-1, 3)
        keep = np.nonzero((matches >= 0) & (matches < len(pos)))[0]
        self.idx = keep
        self.N = len(keep)
        self.p2d = np.asarray(keys_xy, f32)[keep].reshape(-1, 2)
        self.p3d = pos[matches[keep]].reshape(-1, 3)
        sig = np.asarray(level_sigma2, f32)
        self.sigma2 = sig[np.clip(np.asarray(octaves, np.int64)[keep], 0, len(sig) - 1)] if self.N else np.zeros(0, f32)
        self.K = [F64(f32(k)) for k in K]
        self.trace = []

    def set_params(self, draws, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4,
                   th2=5.991):
        assert min_set == 4
        self.draws = np.asarray(draws, np.int64).reshape(-1, 4)
        self.min_inliers, self.max_its = ransac_parameters(self.N, probability, min_inliers, max_iterations, min_set,
                                                           epsilon)
        self.max_error = (self.sigma2 * np.float32(th2)).astype(np.float32)   # cc:189: a float product
        self.iterations, self.best_inliers, self.best_iteration, self.status = 0, 0, -1, 0
        self.best_flags = None
        self.best_T = np.full(12, np.nan, np.float32)
        self.refine_cache = None
        self.counts = {}
        self.events = []   # ("best", iteration) and ("refine", iteration, refined count), as they happen
        self.spans = {}    # iteration -> (first, one past last) trace entry of its hypothesis and count
        self.refine_ratios = []   # error2 / mvMaxError of every Refine that ran

    def _pose_of(self, sel):
        key = tuple(int(i) for i in sel)
        mine = self.basis.setdefault(key, {})
        return compute_pose(self.p3d[sel], self.p2d[sel], self.K, self.arith, self.conv, self.trace,
                            None if self.base is None else self.base.get(key), mine)

    def _refine(self):
        if self.refine_cache is None:
            sel = np.nonzero(self.best_flags)[0]
            R, t, _ = self._pose_of(sel)
            flags = check_inliers(R, t, self.K, self.p3d, self.p2d, self.max_error, self.trace)
            self.refine_ratios.append(self.trace[-1][1])
            self.refine_cache = (R, t, flags, int(flags.sum()))
        return self.refine_cache

    @staticmethod
    def _T(R, t):
        T = np.zeros((3, 4), np.float32)
        T[:, :3] = R.astype(np.float32)
        T[:, 3] = t.astype(np.float32)
        return T.reshape(12)

    def iterate(self, n_iterations):
        o = dict(found=0, no_more=0, n_inliers=0, inliers=np.zeros(self.n, np.uint8), Tcw=np.zeros(12, np.float32),
                 frame_mp=np.full(self.n, -1, np.int32), refined=0, n_corr=self.N, min_inliers_used=self.min_inliers,
                 max_its_used=self.max_its)
        flags = None
        if self.N < self.min_inliers:
            o["no_more"] = 1
        else:
            cur, returned = 0, False
            while self.iterations < self.max_its or cur < n_iterations:   # cc:226
                if self.iterations >= len(self.draws):
                    o["no_more"] = 1
                    self.status |= STATUS_NO_DRAWS
                    returned = True
                    break
                k = self.iterations
                cur += 1
                self.iterations += 1
                sel = select4(self.draws[k], self.N)
                first = len(self.trace)
                if sel is None:
                    self.status |= STATUS_BAD_DRAW
                    inl, f = 0, np.zeros(self.N, bool)
                    R = t = None
                else:
                    R, t, _ = self._pose_of(sel)
                    f = check_inliers(R, t, self.K, self.p3d, self.p2d, self.max_error, self.trace)
                    inl = int(f.sum())
                self.counts[k] = inl
                self.spans[k] = (first, len(self.trace))
                if inl >= self.min_inliers:
                    if inl > self.best_inliers:
                        self.best_inliers, self.best_iteration, self.best_flags = inl, k, f
                        self.best_T = self._T(R, t)
                        self.refine_cache = None
                        self.events.append(("best", k))
                    R2, t2, f2, n2 = self._refine()
                    self.events.append(("refine", k, n2))
                    if n2 > self.min_inliers:
                        o.update(found=1, refined=1, n_inliers=n2, Tcw=self._T(R2, t2))
                        flags = f2
                        returned = True
                        break
            if not returned and self.iterations >= self.max_its:
                o["no_more"] = 1
                if self.best_inliers >= self.min_inliers:
                    o.update(found=1, n_inliers=self.best_inliers, Tcw=self.best_T.copy())
                    flags = self.best_flags
        if flags is not None:
            o["inliers"][self.idx[flags]] = 1
            o["frame_mp"][self.idx[flags]] = self.matches[self.idx[flags]]
        o.update(best_Tcw=self.best_T.copy(), best_inliers=self.best_inliers, best_iteration=self.best_iteration,
                 iterations=self.iterations, status=self.status)
        return o
