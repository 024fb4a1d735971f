"""Float64 numpy restatement of Optimizer::PoseOptimization (src/Optimizer.cc:299-502) and of
the parts of g2o it runs.  Test-only: the reference for orbx_pose_optimization*.

File:line of every step (g2o = Thirdparty/g2o/g2o):
  edges and their order          Optimizer.cc:340-425 (keypoint order; sparse_optimizer sorts the
                                 active edges by insertion id)
  early return, rounds, levels   Optimizer.cc:428-493
  errors                         types/types_six_dof_expmap.h:153-157, 184-188;
                                 types_six_dof_expmap.cpp:290-306 (stereo: float invz),
                                 types/se3_ops.hpp project2d
  Jacobians                      types_six_dof_expmap.cpp:266-288, 335-364
  chi2, robust information       core/base_edge.h:59-61, 96-102
  Huber                          core/robust_kernel_impl.cpp:78-91
  quadratic form                 core/base_unary_edge.hpp:43-72
  LM                             core/optimization_algorithm_levenberg.cpp:61-189
  iteration loop                 core/sparse_optimizer.cpp:354-419 (activeRobustChi2: 100-114)
  dense solve                    solvers/linear_solver_dense.h:104-112
  SE3Quat exp, product, map      types/se3quat.h:104-110, 217-257, 280-285
  update                         types/types_six_dof_expmap.h:73-76
  pose in and out                src/Converter.cc toSE3Quat / toCvMat

`order` chooses how the per-edge terms of H, b and chi2 are added: "forward" (index order,
one at a time: what g2o does), "reversed" (the same from the last edge) and "pairwise"
(numpy's pairwise sum).  The three differ by rounding only; their disagreement is the scale
of legitimate differences between correct implementations.
"""
from __future__ import annotations

import numpy as np

DELTA_MONO = float(np.float32(np.sqrt(5.991)))    # Optimizer.cc:332
DELTA_STEREO = float(np.float32(np.sqrt(7.815)))  # Optimizer.cc:334
CHI2_MONO = np.float32(5.991)                     # Optimizer.cc:433
CHI2_STEREO = np.float32(7.815)                   # Optimizer.cc:434
ROUNDS = 4
ITERATIONS = 10                                   # Optimizer.cc:435
MAX_TRIALS = 10                                   # optimization_algorithm_levenberg.cpp:51
DBL_MAX = np.finfo(np.float64).max

_IU = [(r, c) for r in range(6) for c in range(r, 6)]   # the 21 upper entries of H, row-major


# ---- quaternion (x, y, z, w) and SE3 ------------------------------------------------------

def quat_from_matrix(m):
    """Eigen::Quaterniond(Matrix3d) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl)."""
    q = np.zeros(4)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0.0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[2, 1] - m[1, 2]) * t
        q[1] = (m[0, 2] - m[2, 0]) * t
        q[2] = (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    return q


def quat_normalize(q):
    """SE3Quat::normalizeRotation (se3quat.h:280-285)."""
    if q[3] < 0:
        q = -q
    n = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return q / n


def quat_mul(a, b):
    return np.array([
        a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
        a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
        a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
        a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def quat_rotate(q, v):
    """Eigen's Quaternion * Vector3: uv = 2 (q.vec x v); v + w uv + q.vec x uv.  v: [..., 3]."""
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    ux = q[1] * z - q[2] * y
    uy = q[2] * x - q[0] * z
    uz = q[0] * y - q[1] * x
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    return np.stack([x + q[3] * ux + (q[1] * uz - q[2] * uy),
                     y + q[3] * uy + (q[2] * ux - q[0] * uz),
                     z + q[3] * uz + (q[0] * uy - q[1] * ux)], axis=-1)


def quat_to_matrix(q):
    """Eigen's QuaternionBase::toRotationMatrix."""
    tx, ty, tz = 2.0 * q[0], 2.0 * q[1], 2.0 * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz = tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def se3_from_tcw(tcw12):
    """Converter::toSE3Quat: float rows widened, SE3Quat(R, t) normalises the rotation."""
    T = np.asarray(tcw12, np.float32).reshape(3, 4).astype(np.float64)
    return quat_normalize(quat_from_matrix(T[:, :3])), T[:, 3].copy()


def se3_to_tcw(q, t):
    """Converter::toCvMat(SE3Quat): to_homogeneous_matrix rounded to float."""
    out = np.empty((3, 4))
    out[:, :3] = quat_to_matrix(q)
    out[:, 3] = t
    return out.astype(np.float32).reshape(12)


def se3_exp(x):
    """SE3Quat::exp (se3quat.h:223-257): x = (omega, upsilon)."""
    w, u = x[:3], x[3:]
    theta = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    O = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    O2 = np.array([[O[i, 0] * O[0, j] + O[i, 1] * O[1, j] + O[i, 2] * O[2, j] for j in range(3)] for i in range(3)])
    I = np.eye(3)
    if theta < 0.00001:
        R = I + O + O2
        V = R
    else:
        s, c = np.sin(theta), np.cos(theta)
        R = I + s / theta * O + (1.0 - c) / (theta * theta) * O2
        V = I + (1.0 - c) / (theta * theta) * O + (theta - s) / (theta * theta * theta) * O2
    Vu = np.array([V[i, 0] * u[0] + V[i, 1] * u[1] + V[i, 2] * u[2] for i in range(3)])
    return quat_normalize(quat_from_matrix(R)), Vu


def se3_mul(a, b):
    """SE3Quat::operator* (se3quat.h:104-110)."""
    return quat_normalize(quat_mul(a[0], b[0])), quat_rotate(a[0], b[1]) + a[1]


# ---- edges ---------------------------------------------------------------------------------

class Edges:
    """The frame's edges in keypoint order (Optimizer.cc:340-425)."""

    def __init__(self, keys_xy, octave, u_right, mp, pos, inv_sigma2):
        keys_xy = np.asarray(keys_xy, np.float32).reshape(-1, 2)
        mp = np.asarray(mp, np.int64)
        n_mp = 0 if pos is None else len(pos)
        has = (mp >= 0) & (mp < n_mp)
        self.index = np.nonzero(has)[0]
        ids = mp[self.index]
        self.ids = ids
        self.Xw = np.asarray(pos, np.float32).reshape(-1, 3)[ids].astype(np.float64)
        self.obs = np.zeros((len(ids), 3))
        self.obs[:, :2] = keys_xy[self.index].astype(np.float64)
        if u_right is None:
            self.stereo = np.zeros(len(ids), bool)
        else:
            ur = np.asarray(u_right, np.float32)[self.index]
            self.stereo = ~(ur < 0)                   # cc:346
            self.obs[self.stereo, 2] = ur[self.stereo].astype(np.float64)
        self.w = np.asarray(inv_sigma2, np.float32)[np.asarray(octave)[self.index]].astype(np.float64)
        self.delta = np.where(self.stereo, DELTA_STEREO, DELTA_MONO)
        self.n = len(ids)


def edge_errors(E, cam, pose):
    """computeError of every edge at `pose`: error [n, 3] (third entry 0 for monocular), Xc."""
    fx, fy, cx, cy, bf = cam
    Xc = quat_rotate(pose[0], E.Xw) + pose[1]
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    err = np.zeros((E.n, 3))
    with np.errstate(all="ignore"):
        # monocular: project2d then fx, cx (cpp:290-296)
        err[:, 0] = E.obs[:, 0] - ((x / z) * fx + cx)
        err[:, 1] = E.obs[:, 1] - ((y / z) * fy + cy)
        # stereo: const float invz = 1.0f / z (cpp:299-306)
        invz = (1.0 / z).astype(np.float32).astype(np.float64)
        r0 = x * invz * fx + cx
        r1 = y * invz * fy + cy
        r2 = r0 - bf * invz
        s = E.stereo
        err[s, 0] = E.obs[s, 0] - r0[s]
        err[s, 1] = E.obs[s, 1] - r1[s]
        err[s, 2] = E.obs[s, 2] - r2[s]
    return err, Xc


def edge_chi2(E, err):
    """_error.dot(information() * _error), base_edge.h:59-61."""
    c = err[:, 0] * (E.w * err[:, 0]) + err[:, 1] * (E.w * err[:, 1])
    return np.where(E.stereo, c + err[:, 2] * (E.w * err[:, 2]), c)


def huber(E, chi2, robust):
    """rho(e), rho'(e) (robust_kernel_impl.cpp:78-91); without a kernel e and 1."""
    if not robust:
        return chi2, np.ones_like(chi2)
    dsqr = E.delta * E.delta
    with np.errstate(all="ignore"):
        sq = np.sqrt(chi2)
        out = chi2 > dsqr
        rho0 = np.where(out, 2.0 * sq * E.delta - dsqr, chi2)
        rho1 = np.where(out, E.delta / sq, 1.0)
    return rho0, rho1


def edge_jacobians(E, cam, Xc):
    """linearizeOplus (cpp:266-288, 335-364): [n, 3, 6]; row 2 is zero for monocular edges."""
    fx, fy, cx, cy, bf = cam
    x, y = Xc[:, 0], Xc[:, 1]
    with np.errstate(all="ignore"):
        invz = 1.0 / Xc[:, 2]
    invz_2 = invz * invz
    J = np.zeros((E.n, 3, 6))
    J[:, 0, 0] = x * y * invz_2 * fx
    J[:, 0, 1] = -(1.0 + (x * x * invz_2)) * fx
    J[:, 0, 2] = y * invz * fx
    J[:, 0, 3] = -invz * fx
    J[:, 0, 5] = x * invz_2 * fx
    J[:, 1, 0] = (1.0 + y * y * invz_2) * fy
    J[:, 1, 1] = -x * y * invz_2 * fy
    J[:, 1, 2] = -x * invz * fy
    J[:, 1, 4] = -invz * fy
    J[:, 1, 5] = y * invz_2 * fy
    s = E.stereo
    J[s, 2, 0] = J[s, 0, 0] - bf * y[s] * invz_2[s]
    J[s, 2, 1] = J[s, 0, 1] + bf * x[s] * invz_2[s]
    J[s, 2, 2] = J[s, 0, 2]
    J[s, 2, 3] = J[s, 0, 3]
    J[s, 2, 5] = J[s, 0, 5] - bf * invz_2[s]
    return J


TREE_THREADS = 256   # the kernel's workgroup: 4 waves of 64 lanes


def ordered_sum(a, active, order):
    """Sum over axis 0 of the active rows of a [n, ...] array in the chosen order, from 0.0.
    "tree" is the shape of the HIP kernel's reduction: thread t adds rows t, t + 256, ... in
    index order (inactive rows skipped), the 64 lanes of a wave are combined by an xor
    butterfly (32, 16, ... 1), the four waves are added in wave order."""
    a = np.asarray(a, np.float64)
    flat = a.reshape(a.shape[0], -1)
    if order == "tree":
        n, m = flat.shape
        rows = -(-max(n, 1) // TREE_THREADS)
        pad = np.zeros((rows * TREE_THREADS, m))
        pad[:n][active] = flat[active]                 # x + 0.0 == x: a skipped row adds nothing
        lanes = np.cumsum(pad.reshape(rows, TREE_THREADS, m), axis=0)[-1]
        v = lanes.reshape(TREE_THREADS // 64, 64, m)
        idx = np.arange(64)
        for step in (32, 16, 8, 4, 2, 1):
            v = v + v[:, idx ^ step]
        out = v[0, 0]
        for w in range(1, TREE_THREADS // 64):
            out = out + v[w, 0]
        return out.reshape(a.shape[1:])
    flat = flat[active]
    if flat.shape[0] == 0:
        return np.zeros(a.shape[1:])
    if order == "forward":
        out = np.cumsum(flat, axis=0)[-1]
    elif order == "reversed":
        out = np.cumsum(flat[::-1], axis=0)[-1]
    elif order == "pairwise":
        out = np.ascontiguousarray(flat.T).sum(axis=1)   # pairwise along the contiguous axis
    else:
        raise ValueError(order)
    return out.reshape(a.shape[1:])


def build_system(E, cam, pose, active, robust, order):
    """computeActiveErrors + activeRobustChi2 + buildSystem: chi, H [6, 6], b [6]."""
    err, Xc = edge_errors(E, cam, pose)
    chi2 = edge_chi2(E, err)
    rho0, rho1 = huber(E, chi2, robust)
    J = edge_jacobians(E, cam, Xc)
    w = rho1 * E.w                                   # robustInformation: rho' * Omega
    we = w[:, None] * err                            # [n, 3]
    # per edge: b_j = -(J_0j we_0 + J_1j we_1 (+ J_2j we_2)), H_jk = J_0j w J_0k + ...
    bt = J[:, 0, :] * we[:, 0:1] + J[:, 1, :] * we[:, 1:2]
    bt = np.where(E.stereo[:, None], bt + J[:, 2, :] * we[:, 2:3], bt)
    Ht = np.empty((E.n, 21))
    for k, (r, c) in enumerate(_IU):
        h = J[:, 0, r] * w * J[:, 0, c] + J[:, 1, r] * w * J[:, 1, c]
        Ht[:, k] = np.where(E.stereo, h + J[:, 2, r] * w * J[:, 2, c], h)
    chi = float(ordered_sum(rho0, active, order))
    hs = ordered_sum(Ht, active, order)
    b = -ordered_sum(bt, active, order)
    H = np.zeros((6, 6))
    for k, (r, c) in enumerate(_IU):
        H[r, c] = H[c, r] = hs[k]
    return chi, H, b


def robust_chi(E, cam, pose, active, robust, order):
    err, _ = edge_errors(E, cam, pose)
    rho0, _ = huber(E, edge_chi2(E, err), robust)
    return float(ordered_sum(rho0, active, order))


def ldlt_solve(A, b):
    """Dense LDL^T without pivoting; not positive (a pivot <= 0 or not finite): None
    (linear_solver_dense.h:107-112)."""
    L = np.eye(6)
    d = np.zeros(6)
    for j in range(6):
        s = A[j, j]
        for k in range(j):
            s = s - L[j, k] * L[j, k] * d[k]
        if not (s > 0.0) or not np.isfinite(s):
            return None
        d[j] = s
        for i in range(j + 1, 6):
            v = A[i, j]
            for k in range(j):
                v = v - L[i, k] * L[j, k] * d[k]
            L[i, j] = v / s
    y = np.zeros(6)
    for i in range(6):
        v = b[i]
        for k in range(i):
            v = v - L[i, k] * y[k]
        y[i] = v
    x = np.zeros(6)
    for i in range(5, -1, -1):
        v = y[i] / d[i]
        for k in range(i + 1, 6):
            v = v - L[k, i] * x[k]
        x[i] = v
    return x


def optimize_round(E, cam, pose, active, robust, order):
    """SparseOptimizer::optimize(10) with OptimizationAlgorithmLevenberg: the final pose, the
    pose of the last computeActiveErrors, iterations, trials, accept flags, stop reason."""
    accepts = []
    dchi = []
    err_pose = pose
    lam = ni = 0.0
    nbad = 0
    its = 0
    x = np.zeros(6)
    stop = "iterations"
    with np.errstate(all="ignore"):
        for it in range(ITERATIONS):
            chi, H, b = build_system(E, cam, pose, active, robust, order)
            err_pose = pose
            ini_chi = chi
            if it == 0:
                lam = 1e-5 * max(abs(H[j, j]) for j in range(6))   # computeLambdaInit, tau = 1e-5
                ni = 2.0
                nbad = 0
            qmax = 0
            rho = 0.0
            while True:
                A = H.copy()
                for j in range(6):
                    A[j, j] = A[j, j] + lam
                sol = ldlt_solve(A, b)
                ok = sol is not None
                if ok:
                    x = sol
                trial = se3_mul(se3_exp(x), pose)
                temp = robust_chi(E, cam, trial, active, robust, order)
                err_pose = trial
                if not ok:
                    temp = DBL_MAX
                rho = chi - temp
                dchi.append(rho)
                scale = 0.0
                for j in range(6):
                    scale += x[j] * (lam * x[j] + b[j])
                scale += 1e-3
                rho = rho / scale
                if rho > 0 and np.isfinite(temp):
                    tt = 2.0 * rho - 1.0
                    alpha = 1.0 - tt * tt * tt                       # pow(2 rho - 1, 3)
                    alpha = min(alpha, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    chi = temp
                    pose = trial
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
    return pose, err_pose, its, len(accepts), accepts, stop, dchi


def pose_optimization(keys_xy, octave, u_right, mp, pos, inv_sigma2, fx, fy, cx, cy, bf, tcw, order="forward"):
    """Optimizer::PoseOptimization.  Returns a dict: Tcw [12] float32, outlier [N] uint8 (entries
    of keypoints without a MapPoint stay 0), ninliers (the return value), ninit
    (nInitialCorrespondences), trace [4, 2] (iterations, trials per round), index (keypoint of
    each edge), chi2 [rounds run][nedges], accepts and stop per round."""
    cam = tuple(float(np.float32(v)) for v in (fx, fy, cx, cy, bf))
    tcw = np.asarray(tcw, np.float32).reshape(12)
    E = Edges(keys_xy, octave, u_right, mp, pos, inv_sigma2)
    N = len(np.asarray(mp))
    out = dict(Tcw=tcw.copy(), outlier=np.zeros(N, np.uint8), ninliers=0, ninit=E.n,
               trace=np.zeros((ROUNDS, 2), np.int32), index=E.index, chi2=[], accepts=[], stop=[], decisions=[],
               stereo=E.stereo, Tcw64=tcw.astype(np.float64))
    if E.n < 3:                                        # cc:428
        return out
    pose0 = se3_from_tcw(tcw)
    level = np.zeros(E.n, bool)                        # True: level 1, outlier
    pose = pose0
    nbad = 0
    for rnd in range(ROUNDS):
        active = ~level
        if active.any():
            pose, err_pose, its, trials, accepts, stop, dchi = optimize_round(E, cam, pose0, active, rnd < 3, order)
        else:                                          # no active vertex: optimize() returns at once
            pose, err_pose, its, trials, accepts, stop, dchi = pose0, pose0, 0, 0, [], "noactive", []
        out["trace"][rnd] = (its, trials)
        out["accepts"].append(accepts)
        out["stop"].append(stop)
        out["decisions"].append(dchi)
        chi_act = edge_chi2(E, edge_errors(E, cam, err_pose)[0])
        chi_out = edge_chi2(E, edge_errors(E, cam, pose)[0])   # cc:453-455
        chi2 = np.where(level, chi_out, chi_act)
        out["chi2"].append(chi2)
        with np.errstate(all="ignore"):
            level = chi2.astype(np.float32) > np.where(E.stereo, CHI2_STEREO, CHI2_MONO)
        nbad = int(level.sum())
        if E.n < 10:                                   # cc:491
            break
    out["outlier"][E.index] = level
    out["Tcw"] = se3_to_tcw(*pose)
    out["Tcw64"] = np.concatenate([quat_to_matrix(pose[0]), pose[1][:, None]], axis=1).reshape(12)
    out["ninliers"] = E.n - nbad
    return out


def epilogue(mp, n_mp, outlier, mp_obs, discard):
    """Tracking.cc:1004-1017 on MapPoint ids: (frame_mp, outlier, nmatches_map)."""
    mp = np.asarray(mp, np.int32).copy()
    outlier = np.asarray(outlier, np.uint8).copy()
    has = (mp >= 0) & (mp < n_mp)
    bad = has & (outlier != 0)
    good = has & (outlier == 0)
    if mp_obs is None:
        nmap = int(good.sum())
    else:
        nmap = int((np.asarray(mp_obs)[mp[good]] > 0).sum())
    if discard:
        mp[bad] = -1
        outlier[bad] = 0
    return mp, outlier, nmap


# ---- scenes --------------------------------------------------------------------------------

TUM1 = (517.306408, 516.469215, 318.643040, 255.313989, 40.0)
KITTI = (718.856, 718.856, 607.1928, 185.2157, 386.1448)
INV_SIGMA2 = (1.2 ** (-2.0 * np.arange(8))).astype(np.float32)


def rot(axis_angle):
    x = np.zeros(6)
    x[:3] = axis_angle
    return quat_to_matrix(se3_exp(x)[0])


def make_scene(seed, nedges, cap=None, kind="mono", cam=TUM1, size=(640, 480), noise=1.0, off_deg=1.0,
               off_m=0.03, outlier_frac=0.0, holes=True):
    """One frame: `nedges` keypoints with MapPoints 1-8 m away among cap slots, the others with
    ids of -1 or outside the table interleaved.  kind: mono / stereo / mixed (a third with
    mvuRight < 0)."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, bf = (float(np.float32(v)) for v in cam)
    n = nedges if not holes else nedges + max(2, nedges // 3)
    if cap is None:
        cap = n
    n = min(n, cap)
    n_mp = nedges + 5
    # true pose
    R = rot(rng.normal(size=3) * 0.2)
    t = rng.normal(size=3) * 0.5
    # stereo kinds: far enough for a right coordinate well inside the image (u - bf / z >= 15)
    u_lo = 20.0 if kind == "mono" else max(40.0, bf / 7.0 + 15.0)
    u = rng.uniform(u_lo, size[0] - 20, n)
    v = rng.uniform(20, size[1] - 20, n)
    z_lo = np.ones(n) if kind == "mono" else np.maximum(1.0, bf / (u - 15.0))
    z = rng.uniform(z_lo, 8.0)
    Xc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=1)
    Xw = (Xc - t) @ R                                  # R^T (Xc - t)
    octave = rng.integers(0, 8, n)
    sc = 1.2 ** octave
    uu = u + rng.normal(size=n) * noise * sc
    vv = v + rng.normal(size=n) * noise * sc
    ur = u - bf / z + rng.normal(size=n) * noise * sc
    slots = np.sort(rng.permutation(n)[:nedges])
    mp = np.full(cap, -1, np.int32)
    filler = rng.integers(0, 3, cap)
    mp[:n] = np.where(filler[:n] == 0, -1, np.where(filler[:n] == 1, n_mp + 7, -5))
    ids = rng.permutation(n_mp)[:nedges].astype(np.int32)
    mp[slots] = ids
    pos = rng.normal(size=(n_mp, 3)).astype(np.float32)
    pos[ids] = Xw[slots].astype(np.float32)
    nout = int(round(outlier_frac * nedges))
    gross = np.zeros(cap, bool)
    if nout:
        pick = slots[rng.permutation(nedges)[:nout]]
        ang = rng.uniform(0, 2 * np.pi, nout)
        mag = rng.uniform(20, 60, nout)
        uu[pick] += mag * np.cos(ang)
        vv[pick] += mag * np.sin(ang)
        ur[pick] += mag * np.cos(ang)
        gross[pick] = True
    keys = np.zeros((cap, 2), np.float32)
    keys[:n, 0], keys[:n, 1] = uu, vv
    octs = np.zeros(cap, np.int32)
    octs[:n] = octave
    u_right = None
    if kind != "mono":
        u_right = np.full(cap, -1.0, np.float32)
        u_right[:n] = ur
        if kind == "mixed":
            u_right[:n][rng.integers(0, 3, n) == 0] = -1.0
    # start pose: off by off_deg about a random axis and off_m
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    dR = rot(ax * np.deg2rad(off_deg))
    dt = rng.normal(size=3)
    dt *= off_m / np.linalg.norm(dt)
    T0 = np.empty((3, 4))
    T0[:, :3] = dR @ R
    T0[:, 3] = dR @ t + dt
    Ttrue = np.empty((3, 4))
    Ttrue[:, :3] = R
    Ttrue[:, 3] = t
    return dict(keys_xy=keys, octave=octs, u_right=u_right, mp=mp, pos=pos, n=n, cap=cap, cam=(fx, fy, cx, cy, bf),
                tcw=T0.astype(np.float32).reshape(12), tcw_true=Ttrue.reshape(12), gross=gross, nedges=nedges)


ORDERS = ("forward", "reversed", "pairwise", "tree")


def run_model(sc, order="forward"):
    fx, fy, cx, cy, bf = sc["cam"]
    n = sc["n"]
    ur = None if sc["u_right"] is None else sc["u_right"][:n]
    r = pose_optimization(sc["keys_xy"][:n], sc["octave"][:n], ur, sc["mp"][:n], sc["pos"], INV_SIGMA2, fx, fy, cx,
                          cy, bf, sc["tcw"], order)
    return r


def variants(sc):
    return [run_model(sc, o) for o in ORDERS]


def guard(vs):
    """The conditions on a scene: the three variants agree on the whole LM trace, and every
    chi2 at every classification is further from its threshold than 1000 x the largest chi2
    difference between the variants.  Returns (ok, text)."""
    a = vs[0]
    for v in vs[1:]:
        if v["accepts"] != a["accepts"] or v["stop"] != a["stop"] or not np.array_equal(v["trace"], a["trace"]):
            return False, "LM traces differ"
        if len(v["chi2"]) != len(a["chi2"]):
            return False, "round counts differ"
    if not a["chi2"]:
        return True, "no rounds"
    thr = np.where(a["stereo"], np.float64(CHI2_STEREO), np.float64(CHI2_MONO))
    spread = 0.0
    margin = np.inf
    for r in range(len(a["chi2"])):
        c = np.stack([v["chi2"][r] for v in vs])
        if not np.isfinite(c).all():
            return False, "non-finite chi2"
        spread = max(spread, float((c.max(axis=0) - c.min(axis=0)).max()))
        margin = min(margin, float(np.abs(c - thr).min()))
    if not margin > 1000.0 * spread:
        return False, f"chi2 margin {margin:g} within 1000 x spread {spread:g}"
    return True, f"margin {margin:g}, spread {spread:g}"


def decision_margin(vs):
    """How far the LM decisions are from rounding level: the smallest ratio, over every
    quantity whose sign decides a trial (chi - chi_trial) or the _nBad stop ((iniChi - chi)
    1e3 - iniChi), of its magnitude to its spread between the variants (inf: no spread).
    A converged iteration decides at rounding level, so agreement of the variants' traces
    can be luck; the seed search prefers scenes with a large ratio.  Needs guard(vs)."""
    worst = np.inf
    for r in range(len(vs[0]["decisions"])):
        d = np.array([v["decisions"][r] for v in vs])
        if d.size == 0:
            continue
        sp = d.max(axis=0) - d.min(axis=0)
        with np.errstate(all="ignore"):
            ratio = np.where(sp > 0, np.abs(d).min(axis=0) / sp, np.where(np.abs(d).min(axis=0) > 0, np.inf, 0.0))
        worst = min(worst, float(ratio.min()))
    return worst


# ---- the scenes of the GPU tests -------------------------------------------------------------
# Edge counts: the two early exits (0, 2, 3, 9, 10), the wave boundary (63, 64, 65), the
# workgroup stride (255, 256, 257), just under and just over the kernel's LDS staging
# capacity (ORBX_POSE_OPT_LDS_EDGES = 1984), and cap 5000 with about 2000 edges.
LDS_EDGES = 1984
COUNTS = (0, 2, 3, 9, 10, 63, 64, 65, 255, 256, 257, LDS_EDGES - 1, LDS_EDGES + 1)
KINDS = {"mono": dict(cam=TUM1, size=(640, 480)), "stereo": dict(cam=KITTI, size=(1241, 376)),
         "mixed": dict(cam=TUM1, size=(640, 480))}
# name -> make_scene arguments; the seeds are the first for which guard() holds, preferring
# those whose LM decisions are far above rounding level (python tests/pose_opt_spread.py
# --find prints them; the all-monocular scenes converge to rounding level in every seed)
SEEDS = {
    "mono-0": 0, "mono-2": 0, "mono-3": 12, "mono-9": 16, "mono-10": 16, "mono-63": 20, "mono-64": 5, "mono-65": 11,
    "mono-255": 16, "mono-256": 6, "mono-257": 17, "mono-1983": 116, "mono-1985": 81, "mono-cap5000": 108,
    "stereo-0": 0, "stereo-2": 0, "stereo-3": 0, "stereo-9": 0, "stereo-10": 0, "stereo-63": 1, "stereo-64": 2,
    "stereo-65": 1, "stereo-255": 3, "stereo-256": 4, "stereo-257": 2, "stereo-1983": 1, "stereo-1985": 12,
    "stereo-cap5000": 9,
    "mixed-0": 0, "mixed-2": 0, "mixed-3": 0, "mixed-9": 1, "mixed-10": 0, "mixed-63": 0, "mixed-64": 3, "mixed-65": 3,
    "mixed-255": 5, "mixed-256": 0, "mixed-257": 3, "mixed-1983": 1, "mixed-1985": 0, "mixed-cap5000": 0,
    "mixed-off3": 6, "mixed-out30": 7, "mono-out30": 11,
}


def scene_specs():
    specs = {}
    for kind in KINDS:
        for ne in COUNTS:
            specs[f"{kind}-{ne}"] = dict(nedges=ne, kind=kind)
        specs[f"{kind}-cap5000"] = dict(nedges=2000, kind=kind, cap=5000)
    specs["mixed-off3"] = dict(nedges=280, kind="mixed", off_deg=3.0, off_m=0.05)
    specs["mixed-out30"] = dict(nedges=300, kind="mixed", outlier_frac=0.3)
    specs["mono-out30"] = dict(nedges=200, kind="mono", outlier_frac=0.3)
    return specs


def scene(name, seed=None):
    spec = dict(scene_specs()[name])
    kind = spec["kind"]
    return make_scene(SEEDS[name] if seed is None else seed, **spec, **KINDS[kind])


# the B = 16 batch: one camera (mixed scenes), a different count in every frame, an empty
# frame and one with 2 edges among them
BATCH16 = tuple(f"mixed-{c}" for c in COUNTS) + ("mixed-off3", "mixed-out30", "mixed-cap5000")


def transitions(r):
    """(edges that turn outlier, edges that turn inlier again) between consecutive rounds."""
    thr = np.where(r["stereo"], CHI2_STEREO, CHI2_MONO)
    lv = [c.astype(np.float32) > thr for c in r["chi2"]]
    leave = sum(int((~lv[i] & lv[i + 1]).sum()) for i in range(len(lv) - 1))
    enter = sum(int((lv[i] & ~lv[i + 1]).sum()) for i in range(len(lv) - 1))
    return leave, enter


# scenes that must show something more than the guard: rejected trials in the trace, edges
# that leave and re-enter across rounds
def scene_extra(name, r):
    if name.endswith("off3"):
        return any(not a for acc in r["accepts"] for a in acc)
    if name.endswith("out30"):
        return min(transitions(r)) > 0
    return True


def pose_spread(vs):
    t = np.stack([v["Tcw64"] for v in vs])
    return float((t.max(axis=0) - t.min(axis=0)).max())
