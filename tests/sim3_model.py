"""float64 model of Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc:37-534): the parity
basis of orbx_sim3_* (the reference computes in float32 cv::Mat and cannot be built without
OpenCV; the kernel widens its float inputs to double and computes in double).

A literal transcription, each step citing its Sim3Solver.cc line, with switchable variants
whose disagreement is the scale of legitimate differences:

    eigh      numpy.linalg.eigh for the 4x4 eigenproblem (cc:347)
    jacobi    the model's own cyclic Jacobi, the kernel's form
    negated   the eigenvector negated (its sign is free)
    reversed  centroid and M sums in reversed order
    ulp_up / ulp_down   ang and every Rodrigues entry moved by one ulp: the device's atan2 / sincos

Scenes (scene(name)): TUM1 intrinsics, points 1-8 m away, pixel noise 1 px x 1.2^octave, an
outlier share per scene, octaves 0-7, true rotation about 0.3 rad, scale 1.3 or fixed;
fixed seeds (SEEDS).  guard(scene) holds when every variant agrees on every flag and count
over every iteration up to and including the stopping one, and every err / threshold is
further from 1 than 1000 x the largest relative err difference between the variants.
"""
from __future__ import annotations

import functools
import math

import numpy as np

VARIANTS = ("jacobi", "eigh", "negated", "reversed", "ulp_up", "ulp_down")
TUM1 = (517.306408, 516.469215, 318.643040, 255.313989)
KITTI = (718.856, 718.856, 607.1928, 185.2157)
NLEVELS = 8
_sf = [np.float32(1.0)]
for _l in range(1, NLEVELS):  # mvScaleFactor[i] = mvScaleFactor[i-1] * scaleFactor (float x double), mvLevelSigma2 its square
    _sf.append(np.float32(float(_sf[-1]) * 1.2))
LEVEL_SIGMA2 = np.array([np.float32(s * s) for s in _sf], np.float32)
STATUS_BAD_DRAW = 1


# ---- SetRansacParameters, cc:132-185 ------------------------------------------------------
def ransac_iterations(n: int, min_inliers: int, probability: float, max_iterations: int) -> int:
    """mRansacMaxIts for N = n correspondences; n < min_inliers is never used (1)."""
    if n < min_inliers or n <= 0:
        return 1
    if min_inliers == n:                                                   # cc:168
        its = 1
    else:
        eps = np.float32(np.float32(min_inliers) / np.float32(n))          # cc:145 float epsilon
        eps3 = math.pow(float(eps), 3.0)                                   # pow(float, int) promotes to double
        d = math.log(1.0 - eps3)
        if d == 0.0:
            its = max_iterations
        else:
            v = math.log(1.0 - probability) / d                            # cc:171
            its = max_iterations if not math.isfinite(v) or v > max_iterations else int(math.ceil(v))
    return max(1, min(its, max_iterations))                                # cc:181


def thresholds(level_sigma2) -> np.ndarray:
    """mvnMaxError (Sim3Solver.h:143-144, cc:98-99): a size_t, 9.210 * sigma2 truncated."""
    return np.array([float(int(9.210 * float(s))) for s in np.asarray(level_sigma2, np.float32)], np.float64)


# ---- sampling, cc:217-238 -------------------------------------------------------------------
def draw_indices_list(n: int, r) -> tuple:
    """The literal list: vAvailableIndices = 0..N-1, three swap-with-back removals."""
    avail = list(range(n))
    out = []
    for j in range(3):
        out.append(avail[r[j]])
        avail[r[j]] = avail[-1]
        avail.pop()
    return tuple(out)


def draw_indices_closed(n: int, r) -> tuple:
    """The kernel's closed form of the same removals."""
    r0, r1, r2 = (int(x) for x in r)
    l1 = lambda j: n - 1 if j == r0 else j                      # noqa: E731  the list after the first removal
    l2 = lambda j: l1(n - 2) if j == r1 else l1(j)              # noqa: E731  ... after the second
    return r0, l1(r1), l2(r2)


def draws_valid(n: int, r) -> bool:
    return all(0 <= int(r[j]) < n - j for j in range(3))


# ---- the 4x4 symmetric eigenproblem -------------------------------------------------------
def jacobi4(A):
    """Cyclic Jacobi in double (the kernel's form): sweeps over (p, q), p < q, a rotation is
    skipped when a_pq is exactly 0; at most 30 sweeps, stops when the off-diagonal sum is
    exactly 0.  Returns the eigenvector (q0..q3) of the largest eigenvalue (first on ties)."""
    a = [[float(A[i][j]) for j in range(4)] for i in range(4)]
    v = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for _ in range(30):
        off = 0.0
        for p in range(3):
            for q in range(p + 1, 4):
                off = off + abs(a[p][q])
        if not off > 0.0:            # 0, or NaN
            break
        for p in range(3):
            for q in range(p + 1, 4):
                apq = a[p][q]
                if apq == 0.0:
                    continue
                theta = (a[q][q] - a[p][p]) / (2.0 * apq)
                t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
                if theta < 0.0:
                    t = -t
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(4):   # A <- A J  (columns p, q)
                    akp, akq = a[k][p], a[k][q]
                    a[k][p] = c * akp - s * akq
                    a[k][q] = s * akp + c * akq
                for k in range(4):   # A <- J^T A (rows p, q)
                    apk, aqk = a[p][k], a[q][k]
                    a[p][k] = c * apk - s * aqk
                    a[q][k] = s * apk + c * aqk
                a[p][q] = 0.0
                a[q][p] = 0.0
                for k in range(4):   # V <- V J
                    vkp, vkq = v[k][p], v[k][q]
                    v[k][p] = c * vkp - s * vkq
                    v[k][q] = s * vkp + c * vkq
    best = 0
    for k in range(1, 4):
        if a[k][k] > a[best][best]:
            best = k
    return [v[0][best], v[1][best], v[2][best], v[3][best]]


def _ulp(x: float, direction: int) -> float:
    if direction == 0 or not math.isfinite(x):
        return x
    return float(np.nextafter(x, math.inf if direction > 0 else -math.inf))


# ---- ComputeSim3, cc:298-437 -----------------------------------------------------------------
def horn(P1, P2, fix_scale: bool, variant: str = "jacobi"):
    """P1, P2: three points each (rows), camera coordinates in keyframe 1 / 2.  Returns a dict
    with R (3x3), t (3), s, T12 (4x4), T21 (4x4), all float64 (NaN when |v| == 0, cc:371)."""
    rev = variant == "reversed"
    nudge = {"ulp_up": 1, "ulp_down": -1}.get(variant, 0)
    P1 = [[float(P1[k][i]) for i in range(3)] for k in range(3)]
    P2 = [[float(P2[k][i]) for i in range(3)] for k in range(3)]

    def centroid(P):                                     # cc:284-294
        if rev:
            return [((P[2][i] + P[1][i]) + P[0][i]) / 3.0 for i in range(3)]
        return [((P[0][i] + P[1][i]) + P[2][i]) / 3.0 for i in range(3)]

    O1, O2 = centroid(P1), centroid(P2)
    Pr1 = [[P1[k][i] - O1[i] for i in range(3)] for k in range(3)]   # point k, axis i
    Pr2 = [[P2[k][i] - O2[i] for i in range(3)] for k in range(3)]
    M = [[0.0] * 3 for _ in range(3)]                                # cc:318 M = Pr2 * Pr1^T
    for i in range(3):
        for j in range(3):
            if rev:
                M[i][j] = (Pr2[2][i] * Pr1[2][j] + Pr2[1][i] * Pr1[1][j]) + Pr2[0][i] * Pr1[0][j]
            else:
                M[i][j] = (Pr2[0][i] * Pr1[0][j] + Pr2[1][i] * Pr1[1][j]) + Pr2[2][i] * Pr1[2][j]
    N11 = (M[0][0] + M[1][1]) + M[2][2]                              # cc:326-335
    N12 = M[1][2] - M[2][1]
    N13 = M[2][0] - M[0][2]
    N14 = M[0][1] - M[1][0]
    N22 = (M[0][0] - M[1][1]) - M[2][2]
    N23 = M[0][1] + M[1][0]
    N24 = M[2][0] + M[0][2]
    N33 = (-M[0][0] + M[1][1]) - M[2][2]
    N34 = M[1][2] + M[2][1]
    N44 = (-M[0][0] - M[1][1]) + M[2][2]
    Nm = [[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]]
    if variant == "eigh":                                            # cc:347
        if not np.isfinite(np.array(Nm)).all():
            q = [math.nan] * 4
        else:
            w, V = np.linalg.eigh(np.array(Nm, np.float64))
            q = [float(x) for x in V[:, 3]]
    else:
        q = jacobi4(Nm)
    if variant == "negated":
        q = [-x for x in q]
    nv = math.sqrt((q[1] * q[1] + q[2] * q[2]) + q[3] * q[3])        # cc:368 norm(vec)
    ang = _ulp(math.atan2(nv, q[0]), nudge)
    with np.errstate(all="ignore"):
        rv = [float(np.float64(2.0 * ang * q[1 + i]) / np.float64(nv)) for i in range(3)]   # cc:371 (0/0 = NaN)
    # cv::Rodrigues, vector -> matrix (cc:375)
    theta = math.sqrt((rv[0] * rv[0] + rv[1] * rv[1]) + rv[2] * rv[2])
    if theta < 2.220446049250313e-16:
        R = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    else:
        c = math.cos(theta) if math.isfinite(theta) else math.nan
        s = math.sin(theta) if math.isfinite(theta) else math.nan
        c1 = 1.0 - c
        it = 1.0 / theta
        rx, ry, rz = rv[0] * it, rv[1] * it, rv[2] * it
        rrt = [rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz]
        r_x = [0.0, -rz, ry, rz, 0.0, -rx, -ry, rx, 0.0]
        eye = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
        R = [[_ulp((c * eye[3 * i + j] + c1 * rrt[3 * i + j]) + s * r_x[3 * i + j], nudge) for j in range(3)]
             for i in range(3)]
    # cc:379 P3 = R * Pr2 (columns are points)
    P3 = [[(R[i][0] * Pr2[k][0] + R[i][1] * Pr2[k][1]) + R[i][2] * Pr2[k][2] for i in range(3)] for k in range(3)]
    if not fix_scale:                                                # cc:383-405, row-major over (axis, point)
        nom = 0.0
        den = 0.0
        for i in range(3):
            for k in range(3):
                nom = nom + Pr1[k][i] * P3[k][i]
                den = den + P3[k][i] * P3[k][i]
        with np.errstate(all="ignore"):
            sc = float(np.float64(nom) / np.float64(den))
    else:
        sc = 1.0
    sR = [[sc * R[i][j] for j in range(3)] for i in range(3)]        # cc:421
    t = [O1[i] - ((sR[i][0] * O2[0] + sR[i][1] * O2[1]) + sR[i][2] * O2[2]) for i in range(3)]   # cc:413
    with np.errstate(all="ignore"):
        inv = float(np.float64(1.0) / np.float64(sc))
    sRi = [[inv * R[j][i] for j in range(3)] for i in range(3)]      # cc:432
    ti = [-((sRi[i][0] * t[0] + sRi[i][1] * t[1]) + sRi[i][2] * t[2]) for i in range(3)]         # cc:435
    T12 = np.eye(4)
    T21 = np.eye(4)
    T12[:3, :3], T12[:3, 3] = np.array(sR), np.array(t)
    T21[:3, :3], T21[:3, 3] = np.array(sRi), np.array(ti)
    return dict(R=np.array(R, np.float64), t=np.array(t, np.float64), s=float(sc), T12=T12, T21=T21)


def nan_hypothesis():
    n4 = np.full((4, 4), np.nan)
    n4[3] = (0.0, 0.0, 0.0, 1.0)
    return dict(R=np.full((3, 3), np.nan), t=np.full(3, np.nan), s=math.nan, T12=n4, T21=n4.copy())


# ---- constructor, cc:37-129 --------------------------------------------------------------------
def _transform(T, X):
    """Rcw * X + tcw, the kernel's order: ((r0 x + r1 y) + r2 z) + t."""
    T = np.asarray(T, np.float64).reshape(-1)
    X = np.asarray(X, np.float64).reshape(-1, 3)
    return np.stack([((T[4 * r] * X[:, 0] + T[4 * r + 1] * X[:, 1]) + T[4 * r + 2] * X[:, 2]) + T[4 * r + 3]
                     for r in range(3)], axis=1)


def _to_image(Xc, K):
    """FromCameraToImage / Project's tail (cc:506-510, 527-532): no depth check."""
    fx, fy, cx, cy = (float(np.float32(k)) for k in K)
    with np.errstate(all="ignore"):
        invz = 1.0 / Xc[:, 2]
        return np.stack([fx * (Xc[:, 0] * invz) + cx, fy * (Xc[:, 1] * invz) + cy], axis=1)


def setup(sc: dict) -> dict:
    """The constructor on a scene's arrays: compaction in slot order, camera coordinates,
    own projections, truncated thresholds."""
    n1 = int(sc["n1"])
    mp1, mp2 = np.asarray(sc["mp1"][:n1], np.int64), np.asarray(sc["mp2"][:n1], np.int64)
    n_mp = len(sc["mp_pos"])
    keep = (mp1 >= 0) & (mp1 < n_mp) & (mp2 >= 0) & (mp2 < n_mp)
    idx = np.nonzero(keep)[0]                                      # mvnIndices1
    pos = np.asarray(sc["mp_pos"], np.float32).astype(np.float64).reshape(-1, 3)
    X1 = _transform(np.asarray(sc["Tcw1"], np.float32), pos[mp1[idx]]) if len(idx) else np.zeros((0, 3))
    X2 = _transform(np.asarray(sc["Tcw2"], np.float32), pos[mp2[idx]]) if len(idx) else np.zeros((0, 3))
    thr = thresholds(sc["level_sigma2"])
    nl = len(thr)
    o1 = np.clip(np.asarray(sc["oct1"][:n1], np.int64)[idx], 0, nl - 1)
    o2 = np.clip(np.asarray(sc["oct2"][:n1], np.int64)[idx], 0, nl - 1)
    N = len(idx)
    return dict(N=N, idx=idx, X1=X1, X2=X2, p1=_to_image(X1, sc["K1"]), p2=_to_image(X2, sc["K2"]),
                thr1=thr[o1], thr2=thr[o2],
                max_its=ransac_iterations(N, sc["min_inliers"], sc["probability"], sc["max_iterations"]))


class Model:
    """Sim3Solver on a scene: iterate(n) and find() with the reference's persistent state."""

    def __init__(self, sc: dict, variant: str = "jacobi"):
        self.sc, self.variant = sc, variant
        self.S = setup(sc)
        self.iterations = 0          # mnIterations
        self.best_inliers = 0        # mnBestInliers
        self.best_iteration = -1
        self.best = nan_hypothesis()
        self.have_best = False
        self.status = 0
        self._cache = {}

    def hypothesis(self, k: int):
        """Iteration k's Sim3 and per-pair errors: (hyp, err1, err2, flags, valid draw)."""
        if k in self._cache:
            return self._cache[k]
        S, sc = self.S, self.sc
        r = sc["draws"][k]
        ok = draws_valid(S["N"], r)
        if ok:
            i = draw_indices_list(S["N"], r)
            h = horn(S["X1"][list(i)], S["X2"][list(i)], sc["fix_scale"], self.variant)   # cc:241
        else:
            h = nan_hypothesis()
        with np.errstate(all="ignore"):                                                    # cc:440-468
            q21 = _to_image(_transform(h["T12"][:3].reshape(-1), S["X2"]), sc["K1"])
            q12 = _to_image(_transform(h["T21"][:3].reshape(-1), S["X1"]), sc["K2"])
            d1 = S["p1"] - q21
            d2 = q12 - S["p2"]
            e1 = d1[:, 0] * d1[:, 0] + d1[:, 1] * d1[:, 1]
            e2 = d2[:, 0] * d2[:, 0] + d2[:, 1] * d2[:, 1]
            flags = (e1 < S["thr1"]) & (e2 < S["thr2"])                                    # cc:460
        out = (h, e1, e2, flags, ok)
        self._cache[k] = out
        return out

    def iterate(self, n_iterations: int) -> dict:
        S, sc = self.S, self.sc
        n1 = int(sc["n1"])
        res = dict(found=0, no_more=0, n_inliers=0, inliers=np.zeros(n1, np.uint8), T12=np.zeros((4, 4)),
                   walked=[])
        if S["N"] < sc["min_inliers"] or S["N"] < 3:                                       # cc:195
            res["no_more"] = 1
            return self._finish(res)
        cur = 0
        while self.iterations < S["max_its"] and cur < n_iterations:                       # cc:212
            cur += 1
            k = self.iterations
            self.iterations += 1
            h, _, _, flags, ok = self.hypothesis(k)
            if not ok:
                self.status |= STATUS_BAD_DRAW
            inl = int(flags.sum())
            res["walked"].append(k)
            if inl >= self.best_inliers:                                                   # cc:247
                self.best_inliers, self.best_iteration, self.best, self.have_best = inl, k, h, True
                if inl > sc["min_inliers"]:                                                # cc:256
                    res["found"], res["n_inliers"], res["T12"] = 1, inl, h["T12"]
                    res["inliers"][S["idx"][flags]] = 1                                    # cc:260-263
                    return self._finish(res)
        if self.iterations >= S["max_its"]:                                                # cc:270
            res["no_more"] = 1
        return self._finish(res)

    def find(self) -> dict:                                                                # cc:277-281
        return self.iterate(self.S["max_its"])

    def _finish(self, res):
        res.update(best_R=self.best["R"], best_t=self.best["t"], best_s=self.best["s"],
                   best_inliers=self.best_inliers, best_iteration=self.best_iteration,
                   iterations=self.iterations, n_pairs=self.S["N"], status=self.status)
        return res


def run(sc: dict, schedule, variant: str = "jacobi"):
    """The results of a list of calls (ints: iterate(n); "find") on a fresh solver."""
    m = Model(sc, variant)
    return [m.find() if c == "find" else m.iterate(int(c)) for c in schedule], m


def rounds_of(sc: dict, step: int):
    """LoopClosing::ComputeSim3's schedule for one candidate (LoopClosing.cc:298-340):
    iterate(step) until it returns a Sim3 or has no more."""
    m = Model(sc)
    out = []
    while True:
        r = m.iterate(step)
        out.append(r)
        if r["found"] or r["no_more"]:
            return out


# ---- guard ---------------------------------------------------------------------------------------
def guard(sc: dict, upto: int | None = None):
    """(ok, why, stats).  Over iterations 0..stop (the first returning iteration of a fresh
    solver, or the cap; `upto` overrides): every variant has the same flags and counts, and
    every err / threshold is further from 1 than 1000 x the largest relative err difference
    between variants."""
    models = [Model(sc, v) for v in VARIANTS]
    base = models[0]
    if upto is None:
        r = base.find()
        upto = base.iterations
        while not r["found"] and not r["no_more"]:
            r = base.find()
            upto = base.iterations
    spread, margin = 0.0, math.inf
    for k in range(upto):
        hs = [m.hypothesis(k) for m in models]
        f0 = hs[0][3]
        for v, h in zip(VARIANTS[1:], hs[1:]):
            if not np.array_equal(f0, h[3]):
                return False, f"iteration {k}: flags of {v} differ", None
        for which, thr in ((1, base.S["thr1"]), (2, base.S["thr2"])):
            E = np.stack([h[which] for h in hs])
            nan = np.isnan(E)
            if nan.any():
                if not (nan.all(axis=0) == nan.any(axis=0)).all():
                    return False, f"iteration {k}: NaN positions differ", None
            fin = np.isfinite(E).all(axis=0)
            if fin.any():
                e = E[:, fin]
                with np.errstate(all="ignore"):
                    rel = (e.max(axis=0) - e.min(axis=0)) / np.maximum(np.abs(e).max(axis=0), 1e-300)
                    dist = np.abs(e / thr[fin][None, :] - 1.0)
                spread = max(spread, float(rel.max()))
                margin = min(margin, float(dist.min()))
    ok = margin > 1000.0 * spread
    return ok, f"margin {margin:.3g} against 1000 x spread {spread:.3g}", dict(spread=spread, margin=margin, upto=upto)


# ---- scenes ----------------------------------------------------------------------------------------
def _rot(axis, ang):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(ang) * K + (1 - math.cos(ang)) * (K @ K)


def _pose(rng, ang, trans):
    R = _rot(rng.normal(size=3), ang)
    T = np.zeros((3, 4))
    T[:, :3], T[:, 3] = R, rng.normal(size=3) * trans
    return T


def build_scene(seed: int, n_valid: int, cap: int = 1024, fix_scale: bool = False, outliers: float = 0.3,
                min_inliers: int = 20, max_iterations: int = 300, probability: float = 0.99, K1=TUM1, K2=TUM1,
                identical: bool = False, skips: bool = True, noise: float = 1.0, n_slots: int | None = None) -> dict:
    """n_valid kept pairs among n1 <= cap slots (n_slots, or a third more than n_valid); the
    skipped slots (-1, negative, outside the table, in either id array) are interleaved when
    `skips`."""
    rng = np.random.default_rng(seed)
    N = n_valid
    n_skip = min(cap - N, max(6, N // 3)) if skips else 0
    n1 = N + n_skip if n_slots is None else n_slots
    Tcw1, Tcw2 = _pose(rng, 0.4, 1.0), _pose(rng, 0.5, 1.5)
    s12 = 1.0 if fix_scale else 1.3
    R12, t12 = _rot(rng.normal(size=3), 0.3), rng.normal(size=3) * 0.2
    o1, o2 = rng.integers(0, NLEVELS, N), rng.integers(0, NLEVELS, N)

    def sample(K, n):
        z = rng.uniform(1.0, 8.0, n)
        u, v = rng.uniform(20, 620, n), rng.uniform(20, 460, n)
        return np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], axis=1)

    def jitter(X, K, octv):
        sig = noise * 1.2 ** octv
        u = K[0] * X[:, 0] / X[:, 2] + K[2] + rng.normal(size=len(X)) * sig
        v = K[1] * X[:, 1] / X[:, 2] + K[3] + rng.normal(size=len(X)) * sig
        return np.stack([(u - K[2]) / K[0] * X[:, 2], (v - K[3]) / K[1] * X[:, 2], X[:, 2]], axis=1)

    X1 = sample(K1, N)
    X2 = (X1 - t12) @ R12 / s12                       # (1/s) R^T (X1 - t)
    bad = rng.random(N) < outliers
    X2[bad] = sample(K2, int(bad.sum()))
    X1n, X2n = jitter(X1, K1, o1), jitter(X2, K2, o2)
    inv = lambda T, X: (X - T[:, 3]) @ T[:, :3]       # noqa: E731  Rcw^T (X - tcw)
    W1, W2 = inv(Tcw1, X1n), inv(Tcw2, X2n)
    spare = rng.normal(size=(5, 3))
    pos = np.concatenate([W1, W2, spare]).astype(np.float32)
    n_mp = len(pos)
    mp1 = np.full(cap, -1, np.int32)
    mp2 = np.full(cap, -1, np.int32)
    oc1 = rng.integers(-2, NLEVELS + 2, cap).astype(np.int32)   # skipped slots: anything, clamped
    oc2 = rng.integers(-2, NLEVELS + 2, cap).astype(np.int32)
    slots = np.sort(rng.choice(n1, N, replace=False)) if n1 > N else np.arange(N)
    mp1[slots] = np.arange(N)
    mp2[slots] = N + np.arange(N)
    oc1[slots], oc2[slots] = o1, o2
    if identical:                                     # the same MapPoints seen from the same pose
        mp2[slots] = np.arange(N)
        Tcw2 = Tcw1.copy()
    skipped = np.setdiff1d(np.arange(n1), slots)
    kinds = [(-1, 0), (0, -1), (-7, 0), (0, -2147483648), (n_mp, 0), (0, n_mp + 3), (2147483647, 1), (-1, -1)]
    for j, sl in enumerate(skipped):                  # one id valid, the other not; both invalid
        a, b = kinds[j % len(kinds)]
        mp1[sl], mp2[sl] = a, b
    if n1 < cap:                                      # beyond n1: valid ids that must not be read as pairs
        mp1[n1:] = 0
        mp2[n1:] = min(N, n_mp - 1)
    draws = np.zeros((max_iterations, 3), np.int32)
    for k in range(max_iterations):
        for j in range(3):
            draws[k, j] = rng.integers(0, max(1, N - j))
    return dict(seed=seed, cap=cap, n1=n1, mp1=mp1, mp2=mp2, oct1=oc1, oct2=oc2, mp_pos=pos,
                Tcw1=Tcw1.astype(np.float32).reshape(12), Tcw2=Tcw2.astype(np.float32).reshape(12),
                K1=np.array(K1, np.float32), K2=np.array(K2, np.float32), level_sigma2=LEVEL_SIGMA2,
                fix_scale=bool(fix_scale), probability=probability, min_inliers=min_inliers,
                max_iterations=max_iterations, draws=draws, n_valid=N)


SIZES = (0, 2, 3, 4, 5, 19, 20, 21, 63, 64, 65, 255, 256, 257, 1000)
# name -> (seed, builder arguments).  A scene that fails its guard gets another seed here.
SEEDS: dict = {}
for _n in SIZES:
    for _fix in (False, True):
        SEEDS[f"n{_n}-{'fix' if _fix else 'free'}"] = (1000 + 2 * _n + int(_fix),
                                                      dict(n_valid=_n, fix_scale=_fix,
                                                           min_inliers=20 if _n > 19 else 3,
                                                           outliers=0.3 if _n > 5 else 0.0))
SEEDS["k1k2-257"] = (5001, dict(n_valid=257, K2=KITTI))
SEEDS["first-64"] = (5002, dict(n_valid=64, outliers=0.0, noise=0.3))           # returns on its first iteration
SEEDS["late-100"] = (5003, dict(n_valid=100, outliers=0.6, min_inliers=20))     # returns at iteration 92
SEEDS["exhaust-40"] = (5004, dict(n_valid=40, outliers=0.9, min_inliers=20))    # no_more at its cap
SEEDS["exhaust-25"] = (5005, dict(n_valid=25, outliers=0.9, min_inliers=20))    # cap 7 from the table
SEEDS["nan-50"] = (5006, dict(n_valid=50, identical=True, max_iterations=40))
SEEDS["continue-300"] = (5007, dict(n_valid=300, outliers=0.5, min_inliers=20))
for _n in (0, 2, 19):                                                           # min_inliers 20: no more at once
    SEEDS[f"b{_n}"] = (5100 + _n, dict(n_valid=_n, outliers=0.0))
SEEDS["tie-64"] = (5200, dict(n_valid=64, outliers=0.3, min_inliers=48, max_iterations=8))
SEEDS["bad-64"] = (5201, dict(n_valid=64, outliers=0.3, min_inliers=48, max_iterations=8))


@functools.lru_cache(maxsize=None)
def scene(name: str) -> dict:
    seed, kw = SEEDS[name]
    sc = build_scene(seed, **kw)
    if name == "tie-64":      # the best triple again in iterations 5 and 6: the tie goes to the later one
        m = Model(sc)
        counts = [int(m.hypothesis(k)[3].sum()) for k in range(5)]
        sc["draws"][5] = sc["draws"][int(np.argmax(counts))]
        sc["draws"][6] = sc["draws"][5]
    if name == "bad-64":      # draws outside [0, N - j): each costs its iteration only
        sc["draws"][1] = (64, 0, 0)
        sc["draws"][3] = (0, 63, 0)
        sc["draws"][5] = (0, 0, -1)
        sc["draws"][6] = (0, 0, 62)
        sc["draws"][7] = (63, 62, 61)   # the largest valid draws
    return sc


# calls a test makes beyond the first return: the guard then covers every iteration they walk
SCHEDULES = {"continue-300": ["find"] * 4}


@functools.lru_cache(maxsize=None)
def guard_for(name: str):
    """guard() of a named scene over every iteration the tests walk on it."""
    sc = scene(name)
    upto = None
    if name in SCHEDULES:
        upto = run(sc, SCHEDULES[name])[1].iterations
    return guard(sc, upto)


PARITY_SCENES = tuple(k for k in SEEDS if k.startswith("n") and k[1].isdigit()) + ("k1k2-257",)
CHUNK_SCENES = ("first-64", "late-100", "exhaust-40", "exhaust-25", "n257-free", "n20-fix")
# one camera pair, free scale, min_inliers 20, 300 iterations: what one batch shares
BATCH_SCENES = ("b0", "b2", "b19", "n20-free", "n21-free", "exhaust-25", "exhaust-40", "n63-free", "n64-free",
                "n65-free", "late-100", "n255-free", "n256-free", "n257-free", "continue-300", "n1000-free")
ALL_SCENES = tuple(SEEDS)


def pack(scenes) -> dict:
    """Candidates of one camera pair and one parameter set into batch arrays: a shared MapPoint
    table with ids offset per candidate (negative ids stay; ids outside a candidate's table
    go outside the shared one)."""
    B = len(scenes)
    cap = max(s["cap"] for s in scenes)
    its = scenes[0]["max_iterations"]
    for k in ("fix_scale", "probability", "min_inliers", "max_iterations"):
        assert len({s[k] for s in scenes}) == 1, k
    assert all(np.array_equal(s["K1"], scenes[0]["K1"]) and np.array_equal(s["K2"], scenes[0]["K2"]) for s in scenes)
    total = sum(len(s["mp_pos"]) for s in scenes)
    out = dict(n1=np.zeros(B, np.int32), mp1=np.full((B, cap), -1, np.int32), mp2=np.full((B, cap), -1, np.int32),
               oct1=np.zeros((B, cap), np.int32), oct2=np.zeros((B, cap), np.int32),
               pos=np.concatenate([s["mp_pos"] for s in scenes]).astype(np.float32).reshape(-1, 3),
               Tcw1=np.stack([s["Tcw1"] for s in scenes]), Tcw2=np.stack([s["Tcw2"] for s in scenes]),
               draws=np.stack([s["draws"] for s in scenes]).astype(np.int32), cap=cap, max_iterations=its)
    off = 0
    for b, s in enumerate(scenes):
        c, n = s["cap"], len(s["mp_pos"])
        for key in ("mp1", "mp2"):
            ids = s[key].astype(np.int64)
            out[key][b, :c] = np.where(ids < 0, ids, np.where(ids < n, ids + off, np.minimum(ids + total, 2147483647)))
        out["oct1"][b, :c], out["oct2"][b, :c] = s["oct1"], s["oct2"]
        out["n1"][b] = s["n1"]
        off += n
    return out


def _hex(a) -> str:
    return " ".join("%08x" % int(v) for v in np.asarray(a, np.float32).reshape(-1).view(np.uint32))


def cli_text(sc: dict) -> str:
    """The candidate file tests/cpp/sim3_cli.cpp reads."""
    n1 = int(sc["n1"])
    lines = [f"{n1} {len(sc['mp_pos'])} {len(sc['level_sigma2'])} {int(sc['fix_scale'])} {sc['min_inliers']} "
             f"{sc['max_iterations']}", _hex([sc["probability"]]), _hex(sc["K1"]), _hex(sc["K2"]), _hex(sc["Tcw1"]),
             _hex(sc["Tcw2"]), _hex(sc["level_sigma2"])]
    lines += [f"{int(sc['mp1'][i])} {int(sc['mp2'][i])} {int(sc['oct1'][i])} {int(sc['oct2'][i])}" for i in range(n1)]
    lines += [_hex(p) for p in sc["mp_pos"]]
    lines += [" ".join(str(int(v)) for v in d) for d in sc["draws"]]
    return "\n".join(lines) + "\n"


def cli_lines(call, r: dict) -> list:
    """What sim3_cli prints for one call whose outputs (host arrays of one candidate) are r."""
    g = lambda k: int(np.asarray(r[k]).reshape(-1)[0])  # noqa: E731
    found = g("found")
    return [f"call {call} found {found} no_more {g('no_more')} inliers {g('n_inliers')} best {g('best_inliers')} at "
            f"{g('best_iteration')} iterations {g('iterations')} pairs {g('n_pairs')} status {g('status')}",
            ("T12 " + _hex(r["T12"])) if found else "T12", "R " + _hex(r["best_R"]), "t " + _hex(r["best_t"]),
            "s " + _hex(r["best_s"]), "flags " + "".join("1" if f else "0" for f in r["inliers"])]
