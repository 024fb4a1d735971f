"""Float64 numpy restatement of Optimizer::BundleAdjustment / GlobalBundleAdjustemnt
(src/Optimizer.cc:41-281).  Test-only: the reference for orbx_global_bundle_adjustment*.

It is tests/local_ba_model.py with one phase: the same Edges, linearisation, Schur complement
and Levenberg-Marquardt (local_ba_model.optimize with every edge at level 0), and

  the monocular Huber delta      float sqrt(5.99) (cc:115), not the local BA's sqrt(5.991)
  bRobust, nIterations           parameters (cc:41-43)
  no chi2 / depth test, no second optimisation, no erase flags
  every keyframe's output        Converter::toCvMat(SE3Quat), the fixed ones too (cc:236-254)
  a point without an edge        vbNotIncludedMP (cc:223-228): pt_included 0, its input bytes

The variants are local_ba_model.VARIANTS.  The reduced system is factored by the arithmetic of
local_ba_model.ldlt_solve restricted to each pivot row's non-zeros (the terms left out are
exact zeros), so that a banded map of hundreds of keyframes costs what its envelope costs.
"""
from __future__ import annotations

import contextlib
import functools

import numpy as np

import local_ba_model as M
from pose_opt_model import quat_to_matrix, se3_from_tcw, se3_to_tcw, rot, TUM1, INV_SIGMA2

DELTA_MONO = float(np.float32(np.sqrt(5.99)))      # Optimizer.cc:115
DELTA_STEREO = M.DELTA_STEREO                       # Optimizer.cc:116
STATUS_CAPACITY, STATUS_NO_FREE_KF, STATUS_BAD_INDEX = 1, 2, 4
VARIANTS = M.VARIANTS


def ldlt_solve_sparse(S, b, perm):
    """local_ba_model.ldlt_solve with every pivot's update restricted to the pivot row's
    non-zero entries: the same terms in the same order, less the exact zeros."""
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
            nz = j + 1 + np.nonzero(A[j, j + 1:])[0]
            l = A[j, nz]
            A[np.ix_(nz, nz)] = A[np.ix_(nz, nz)] - l[:, None] * l[None, :] * d
        for k in range(n - 1):
            x[k + 1:] = x[k + 1:] - A[k, k + 1:] * x[k]
        x = x / np.diag(A)
        for k in range(n - 1, 0, -1):
            x[:k] = x[:k] - A[:k, k] * x[k]
    out = np.empty(n)
    out[p] = x
    return out, piv


@contextlib.contextmanager
def _sparse_solver():
    keep = M.ldlt_solve
    M.ldlt_solve = ldlt_solve_sparse
    try:
        yield
    finally:
        M.ldlt_solve = keep


def free_columns(sc, E):
    """Row of every block column of S: the keyframes that may move and have an edge, in table order."""
    K = len(sc["fixed"])
    cnt = np.bincount(E.kf, minlength=K)
    return np.nonzero(~np.asarray(sc["fixed"]).astype(bool) & (cnt > 0))[0]


def envelope_blocks(sc, dense=False):
    """The blocks of S's envelope by brute force: every pair of block columns that share a point."""
    E = M.Edges(sc)
    cols = free_columns(sc, E)
    F = len(cols)
    if dense:
        return F * (F + 1) // 2
    fidx = np.full(len(sc["fixed"]), -1)
    fidx[cols] = np.arange(F)
    first = np.arange(F)
    for j in np.unique(E.pt):
        fs = fidx[E.kf[E.pt == j]]
        fs = fs[fs >= 0]
        for a in fs:
            for c in fs:
                if a < first[c]:
                    first[c] = a
    return int((np.arange(F) - first + 1).sum())


def _chi(E, cam, st, robust, order):
    if E.n == 0:
        return 0.0
    err, _ = M.edge_errors(E, cam, st.q, st.t, st.X)
    rho0, _ = M.huber(E, M.edge_chi2(E, err), robust)
    return float(M.osum(rho0, order, owner=E.pt % M.THREADS))


def global_ba(sc, iterations=10, robust=True, order="forward", inv3="cofactor", perm="natural", max_env_blocks=None,
              dense=False, delta_mono=DELTA_MONO):
    """Optimizer::BundleAdjustment.  Returns a dict: Tcw [K, 12] and pos [P, 3] float32,
    pt_included [P] uint8, trace [2], chi2 [2], status, and what guard() reads."""
    cam = tuple(float(np.float32(v)) for v in sc["cam"])
    Tcw = np.asarray(sc["Tcw"], np.float32).reshape(-1, 12)
    pos = np.asarray(sc["pos"], np.float32).reshape(-1, 3)
    fixed = np.asarray(sc["fixed"]).astype(bool)
    K, P = len(fixed), len(pos)
    iterations = iterations if iterations > 0 else 10
    out = dict(Tcw=Tcw.copy(), pos=pos.copy(), pt_included=np.zeros(P, np.uint8), trace=np.zeros(2, np.int32),
               chi2=np.zeros(2), status=0, accepts=[], stop=[], decisions=[], active_kf=[], active_pt=[],
               min_pivot=np.inf, Tcw64=Tcw.astype(np.float64), pos64=pos.astype(np.float64), blocks=0)
    if int((~fixed).sum()) == 0:
        out["status"] = STATUS_NO_FREE_KF
        return out
    E = M.Edges(sc)
    E.delta = np.where(E.stereo, DELTA_STEREO, delta_mono)
    bad = STATUS_BAD_INDEX if E.bad_index else 0
    out["blocks"] = envelope_blocks(sc, dense)
    if max_env_blocks is not None and out["blocks"] > max_env_blocks:
        out["status"] = STATUS_CAPACITY | bad
        return out
    out["status"] = bad
    poses = [se3_from_tcw(T) for T in Tcw]
    st = M.State(np.array([p[0] for p in poses]), np.array([p[1] for p in poses]), pos.astype(np.float64))
    out["chi2"][0] = _chi(E, cam, st, robust, order)
    with _sparse_solver():
        st, _, its, trials = M.optimize(E, cam, st, fixed, np.zeros(E.n, bool), robust, iterations, order, inv3, perm, out)
    out["trace"][:] = (its, trials)
    out["chi2"][1] = _chi(E, cam, st, robust, order)
    inc = np.bincount(E.pt, minlength=P) > 0
    out["pt_included"] = inc.astype(np.uint8)
    T64 = np.zeros((K, 12))
    for k in range(K):                                       # cc:236-254: every keyframe
        out["Tcw"][k] = se3_to_tcw(st.q[k], st.t[k])
        T64[k] = np.concatenate([quat_to_matrix(st.q[k]), st.t[k][:, None]], axis=1).reshape(12)
    out["Tcw64"] = T64
    out["pos64"] = st.X
    out["pos"] = np.where(inc[:, None], st.X.astype(np.float32), pos)
    return out


def variants(sc, which=VARIANTS, **kw):
    return [global_ba(sc, order=o, inv3=i, perm=p, **kw) for o, i, p in which]


def guard(vs):
    """The conditions on a scene: all variants agree on the accepted / rejected sequence, the
    stop reason, the trace, the active sets, pt_included and the status; every LDL^T pivot is
    positive; every LM decision value (each rho and each (ini_chi - chi) 1e3 - ini_chi) lies
    farther from 0 than 1000 x its spread between the variants.  Returns (ok, text)."""
    a = vs[0]
    for v in vs[1:]:
        if v["accepts"] != a["accepts"] or v["stop"] != a["stop"] or not np.array_equal(v["trace"], a["trace"]):
            return False, "LM traces differ"
        if v["active_kf"] != a["active_kf"] or v["active_pt"] != a["active_pt"] or v["status"] != a["status"]:
            return False, "active sets differ"
        if not np.array_equal(v["pt_included"], a["pt_included"]):
            return False, "pt_included differs"
    if not all(v["min_pivot"] > 0 for v in vs):
        return False, "a pivot is not positive"
    if not a["decisions"] or not a["decisions"][0]:
        return True, "no decisions"
    d = np.array([v["decisions"][0] for v in vs], np.float64)
    if not np.isfinite(d).all():
        return False, "non-finite decision value"
    sp = d.max(axis=0) - d.min(axis=0)
    margin = np.abs(d).min(axis=0)
    if not (margin > 1000.0 * sp).all():
        i = int(np.argmin(margin / np.maximum(sp, 1e-300)))
        return False, f"decision {i}: |value| {margin[i]:g} within 1000 x spread {sp[i]:g}"
    ratio = float((margin / np.maximum(sp, 1e-300)).min())
    return True, f"{d.shape[1]} decisions, smallest |value| / spread {ratio:.3g}"


spread = M.spread
batch_arrays = M.batch_arrays


# ---- scenes --------------------------------------------------------------------------------------

def make_banded(seed, n_kf, window=4, pts_per_kf=2, n_loop=3, kind="mixed", noise=1.0, step=0.12, off_deg=0.3,
                off_m=0.02, off_pt=0.02):
    """A loop map: n_kf keyframes on an out-and-back line (keyframe 0 fixed, the last one back
    at the start), pts_per_kf points per keyframe seen by `window` consecutive keyframes from
    it on, and n_loop loop points seen by keyframes 1, 2, n_kf - 2 and n_kf - 1.  The envelope
    of S is then far smaller than dense, with two long columns.  The dict of
    local_ba_model.make_scene."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, bf = (float(np.float32(v)) for v in TUM1)
    K = n_kf
    fixed = np.zeros(K, bool)
    fixed[0] = True
    Rs = [rot(rng.normal(size=3) * 0.02) for _ in range(K)]
    cs = [np.array([step * min(k, K - 1 - k), 0.0, 0.0]) + rng.normal(size=3) * 0.01 for k in range(K)]
    ts = [-Rs[k] @ cs[k] for k in range(K)]
    views, Xw = [], []
    for k in range(K):
        ks = [k2 for k2 in range(k, k + window) if k2 < K]
        if len(ks) < 2:
            continue
        for _ in range(pts_per_kf):
            views.append(ks)
            c = np.mean([cs[k2] for k2 in ks], axis=0)
            Xw.append(c + np.array([rng.uniform(-1.0, 1.0), rng.uniform(-0.8, 0.8), rng.uniform(3.0, 8.0)]))
    for _ in range(n_loop):
        views.append([1, 2, K - 2, K - 1])
        Xw.append(cs[1] + np.array([rng.uniform(-1.0, 1.0), rng.uniform(-0.8, 0.8), rng.uniform(3.0, 8.0)]))
    Xw = np.array(Xw)
    per_kf = np.bincount(np.concatenate(views), minlength=K)
    cap = int(per_kf.max()) + 3
    n_slots = K + 2
    slot = rng.permutation(n_slots)[:K].astype(np.int32)
    kps_xy = np.zeros((n_slots, cap, 2), np.float32)
    kps_oct = np.zeros((n_slots, cap), np.int32)
    u_right = np.full((n_slots, cap), -1.0, np.float32)
    rows = [list(rng.permutation(cap)) for _ in range(K)]
    obs_off, obs_kf, obs_kp = [0], [], []
    for j, ks in enumerate(views):
        for k in ks:
            Xc = Rs[k] @ Xw[j] + ts[k]
            pu, pv = fx * Xc[0] / Xc[2] + cx, fy * Xc[1] / Xc[2] + cy
            assert Xc[2] > 0.5 and 5 < pu < M.SIZE[0] - 5 and 5 < pv < M.SIZE[1] - 5
            octv = int(rng.integers(0, 8))
            s = 1.2 ** octv
            mono = kind == "mono" or (kind == "mixed" and rng.integers(0, 3) == 0)
            du, dv = rng.normal(size=2) * noise * s
            dr = rng.normal() * noise * s
            kp = int(rows[k].pop())
            kps_xy[slot[k], kp] = (pu + du, pv + dv)
            kps_oct[slot[k], kp] = octv
            u_right[slot[k], kp] = -1.0 if mono else max(pu - bf / Xc[2] + dr, 0.0)
            obs_kf.append(k)
            obs_kp.append(kp)
        obs_off.append(len(obs_kf))
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
    return dict(cam=(fx, fy, cx, cy, bf), Tcw=Tcw, fixed=fixed.astype(np.uint8), slot=slot, pos=pos,
                obs_off=np.asarray(obs_off, np.int32), obs_kf=np.asarray(obs_kf, np.int32),
                obs_kp=np.asarray(obs_kp, np.int32), kps_xy=kps_xy, kps_oct=kps_oct,
                u_right=None if kind == "mono" else u_right, inv_sigma2=INV_SIGMA2, Tcw_true=Ttrue, pos_true=Xw,
                gross=np.zeros(len(obs_kf), bool), kind=kind)


def make_odd(seed):
    """A point with one observation, a point with none, a free keyframe without an edge (the
    last row), two fixed keyframes (rows 0 and 3) and slots / keypoint rows out of storage order."""
    sc = M.make_scene(seed, n_free=3, n_fixed=1, n_pts=16, single_obs=True, no_obs=True, idle_fixed=True, kf0_fixed=True)
    sc["fixed"] = sc["fixed"].copy()
    sc["fixed"][-1] = 0
    return sc


THREE = (VARIANTS[0], VARIANTS[3], VARIANTS[5])              # forward, kernel, the reversed factorisation

# name -> (maker, its arguments, iterations, robust, variants): the smallest scenes at which each
# piece can go wrong
SPECS = {
    "1+1-6pts": (M.make_scene, dict(n_free=1, n_fixed=1, n_pts=6), 10, True, VARIANTS),
    "init-60": (M.make_scene, dict(n_free=1, n_fixed=1, n_pts=60, kind="mono"), 20, True, VARIANTS),
    "init-300": (M.make_scene, dict(n_free=1, n_fixed=1, n_pts=300, kind="mono"), 20, True, VARIANTS),
    "mono": (M.make_scene, dict(n_free=5, n_fixed=1, n_pts=40, kind="mono", max_obs=4), 10, True, VARIANTS),
    "stereo": (M.make_scene, dict(n_free=7, n_fixed=1, n_pts=40, kind="stereo", max_obs=5), 10, False, VARIANTS),
    "mixed": (M.make_scene, dict(n_free=10, n_fixed=2, n_pts=60, max_obs=6), 10, False, VARIANTS),
    "mixed-out10": (M.make_scene, dict(n_free=8, n_fixed=1, n_pts=60, max_obs=6, outlier_frac=0.1), 10, True, VARIANTS),
    "odd": (make_odd, dict(), 10, True, VARIANTS),
    "edges-255": (M.make_scene, dict(n_free=4, n_fixed=4, n_pts=40, n_edges=255), 10, True, VARIANTS),
    "edges-256": (M.make_scene, dict(n_free=4, n_fixed=4, n_pts=40, n_edges=256), 10, False, VARIANTS),
    "edges-257": (M.make_scene, dict(n_free=4, n_fixed=4, n_pts=40, n_edges=257), 10, True, VARIANTS),
    "pts-1": (M.make_scene, dict(n_free=1, n_fixed=2, n_pts=1, kind="stereo"), 10, True, VARIANTS),
    "pts-257": (M.make_scene, dict(n_free=2, n_fixed=2, n_pts=257, max_obs=3), 10, True, VARIANTS),
    "banded-63": (make_banded, dict(n_kf=64), 10, False, VARIANTS),
    "banded-64": (make_banded, dict(n_kf=65, kind="stereo"), 10, True, VARIANTS),
    "banded-65": (make_banded, dict(n_kf=66), 10, False, VARIANTS),
    "banded-257": (make_banded, dict(n_kf=257, pts_per_kf=1), 2, False, THREE),
}
BANDED = ("banded-63", "banded-64", "banded-65", "banded-257")
# seeds: the first for which guard() holds (python tests/global_ba_spread.py --find prints them)
SEEDS = {name: 0 for name in SPECS}


def scene(name, seed=None):
    maker, kw = SPECS[name][:2]
    return maker(SEEDS[name] if seed is None else seed, **kw)


def params(name):
    return dict(iterations=SPECS[name][2], robust=SPECS[name][3])


@functools.lru_cache(maxsize=None)
def checked(name):
    """(scene, the variants' results, (ok, text) of the guard, (pose spread, position spread)),
    computed once per process: the CPU and the GPU tests share it."""
    sc = scene(name)
    vs = variants(sc, SPECS[name][4], **params(name))
    return sc, vs, guard(vs), spread(vs)
