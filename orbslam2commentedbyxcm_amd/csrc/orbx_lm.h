// orbx_lm.h -- device pieces shared by the Levenberg-Marquardt kernels (orbx_poseopt.hip,
// orbx_optsim3.hip, orbx_localba.hip, orbx_globalba.hip, orbx_essgraph.hip): Eigen's quaternion formulas, g2o's
// SE3Quat and Huber
// kernel, the fixed-shape workgroup sums and the dense LDL^T of linear_solver_dense.h, for a
// compile-time dimension per thread and for a run-time dimension per workgroup.  Everything is
// double and every function is inlined into its kernel.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace orbx {
namespace lm {

// Eigen::Quaterniond(Matrix3d)
__host__ __device__ __forceinline__ void quat_from_matrix(const double (&m)[3][3], double (&q)[4]) {
    double t = m[0][0] + m[1][1] + m[2][2];
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[2][1] - m[1][2]) * t;
        q[1] = (m[0][2] - m[2][0]) * t;
        q[2] = (m[1][0] - m[0][1]) * t;
    } else if (m[0][0] >= m[1][1] && m[0][0] >= m[2][2]) {  // i = 0 (the first largest diagonal entry)
        t = sqrt(m[0][0] - m[1][1] - m[2][2] + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[2][1] - m[1][2]) * t;
        q[1] = (m[1][0] + m[0][1]) * t;
        q[2] = (m[2][0] + m[0][2]) * t;
    } else if (m[1][1] >= m[2][2]) {  // i = 1
        t = sqrt(m[1][1] - m[2][2] - m[0][0] + 1.0);
        q[1] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[0][2] - m[2][0]) * t;
        q[2] = (m[2][1] + m[1][2]) * t;
        q[0] = (m[0][1] + m[1][0]) * t;
    } else {  // i = 2
        t = sqrt(m[2][2] - m[0][0] - m[1][1] + 1.0);
        q[2] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[1][0] - m[0][1]) * t;
        q[0] = (m[0][2] + m[2][0]) * t;
        q[1] = (m[1][2] + m[2][1]) * t;
    }
}

// Eigen's Quaternion * Vector3 (uv = 2 q.vec x v; v + w uv + q.vec x uv)
__device__ __forceinline__ void quat_rotate(double qx, double qy, double qz, double qw, double X, double Y, double Z,
                                            double& x, double& y, double& z) {
    double ux = qy * Z - qz * Y, uy = qz * X - qx * Z, uz = qx * Y - qy * X;
    ux += ux;
    uy += uy;
    uz += uz;
    x = X + qw * ux + (qy * uz - qz * uy);
    y = Y + qw * uy + (qz * ux - qx * uz);
    z = Z + qw * uz + (qx * uy - qy * ux);
}

// Eigen's toRotationMatrix
__device__ __forceinline__ void quat_to_matrix(double qx, double qy, double qz, double qw, double (&R)[3][3]) {
    const double tx = 2.0 * qx, ty = 2.0 * qy, tz = 2.0 * qz;
    const double twx = tx * qw, twy = ty * qw, twz = tz * qw;
    const double txx = tx * qx, txy = ty * qx, txz = tz * qx;
    const double tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
    R[0][0] = 1.0 - (tyy + tzz);
    R[0][1] = txy - twz;
    R[0][2] = txz + twy;
    R[1][0] = txy + twz;
    R[1][1] = 1.0 - (txx + tzz);
    R[1][2] = tyz - twx;
    R[2][0] = txz - twy;
    R[2][1] = tyz + twx;
    R[2][2] = 1.0 - (txx + tyy);
}

// g2o::SE3Quat: a unit quaternion and a translation
struct Pose {
    double qx, qy, qz, qw, tx, ty, tz;
};

// SE3Quat::normalizeRotation, se3quat.h:280-285
__device__ __forceinline__ void quat_normalize(double& x, double& y, double& z, double& w) {
    if (w < 0) {
        x = -x;
        y = -y;
        z = -z;
        w = -w;
    }
    const double n = sqrt(x * x + y * y + z * z + w * w);
    x = x / n;
    y = y / n;
    z = z / n;
    w = w / n;
}

// SE3Quat::map, se3quat.h:217-220
__device__ __forceinline__ void pose_map(const Pose& P, double X, double Y, double Z, double& x, double& y,
                                         double& z) {
    quat_rotate(P.qx, P.qy, P.qz, P.qw, X, Y, Z, x, y, z);
    x += P.tx;
    y += P.ty;
    z += P.tz;
}

// SE3Quat::exp(x) * P: types_six_dof_expmap.h:73-76 with se3quat.h:223-257 and 104-110
__device__ __forceinline__ Pose pose_update(const double (&x)[6], const Pose& P) {
    const double w0 = x[0], w1 = x[1], w2 = x[2];
    const double theta = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    const double O[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
    double O2[3][3], R[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) O2[i][j] = O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j];
    if (theta < 0.00001) {
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                R[i][j] = (i == j ? 1.0 : 0.0) + O[i][j] + O2[i][j];
                V[i][j] = R[i][j];
            }
    } else {
        const double s = sin(theta), c = cos(theta);
        const double a = s / theta, b = (1.0 - c) / (theta * theta), d = (theta - s) / (theta * theta * theta);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const double id = i == j ? 1.0 : 0.0;
                R[i][j] = id + a * O[i][j] + b * O2[i][j];
                V[i][j] = id + b * O[i][j] + d * O2[i][j];
            }
    }
    double q[4];
    quat_from_matrix(R, q);
    quat_normalize(q[0], q[1], q[2], q[3]);
    const double t0 = V[0][0] * x[3] + V[0][1] * x[4] + V[0][2] * x[5];
    const double t1 = V[1][0] * x[3] + V[1][1] * x[4] + V[1][2] * x[5];
    const double t2 = V[2][0] * x[3] + V[2][1] * x[4] + V[2][2] * x[5];
    Pose out;
    out.qx = q[3] * P.qx + q[0] * P.qw + q[1] * P.qz - q[2] * P.qy;
    out.qy = q[3] * P.qy + q[1] * P.qw + q[2] * P.qx - q[0] * P.qz;
    out.qz = q[3] * P.qz + q[2] * P.qw + q[0] * P.qy - q[1] * P.qx;
    out.qw = q[3] * P.qw - q[0] * P.qx - q[1] * P.qy - q[2] * P.qz;
    quat_normalize(out.qx, out.qy, out.qz, out.qw);
    double rx, ry, rz;
    quat_rotate(q[0], q[1], q[2], q[3], P.tx, P.ty, P.tz, rx, ry, rz);
    out.tx = rx + t0;
    out.ty = ry + t1;
    out.tz = rz + t2;
    return out;
}

// RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91): rho(e) returned, rho'(e) in rho1.
__device__ __forceinline__ double huber(double chi2, double delta, bool robust, double& rho1) {
    rho1 = 1.0;
    if (!robust) return chi2;
    const double dsqr = delta * delta;
    if (chi2 > dsqr) {
        const double sq = sqrt(chi2);
        rho1 = delta / sq;
        return 2.0 * sq * delta - dsqr;
    }
    return chi2;
}

// Sums over a workgroup of W waves.  All threads leave with the same sums: lanes by an xor
// butterfly (32, 16, ... 1), waves in wave order.  s_red: [W][N] doubles.
template <int N, int W>
__device__ __forceinline__ void block_sum(double (&v)[N], double* s_red) {
#pragma unroll
    for (int k = 0; k < N; k++)
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) v[k] += __shfl_xor(v[k], m, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < N; k++) s_red[wave * N + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; k++) {
        double s = s_red[k];
#pragma unroll
        for (int w = 1; w < W; w++) s += s_red[w * N + k];
        v[k] = s;
    }
    __syncthreads();
}

// The same order, the sums left in LDS (s_sum [N]) for every thread to read.
template <int N, int W>
__device__ __forceinline__ void block_sum_lds(double (&v)[N], double* s_red, double* s_sum) {
#pragma unroll
    for (int k = 0; k < N; k++)
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) v[k] += __shfl_xor(v[k], m, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < N; k++) s_red[wave * N + k] = v[k];
    }
    __syncthreads();
    for (int k = threadIdx.x; k < N; k += W * 64) {
        double s = s_red[k];
#pragma unroll
        for (int w = 1; w < W; w++) s += s_red[w * N + k];
        s_sum[k] = s;
    }
    __syncthreads();
}

template <int W>
__device__ __forceinline__ int block_sum_int(int v, int* s_cnt) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < W; w++) s += s_cnt[w];
    __syncthreads();
    return s;
}

// (H + lambda I) x = b by a dense LDL^T without pivoting; h: the upper triangle of H row by
// row.  A pivot that is not positive (or not finite) is a failed solve
// (linear_solver_dense.h:107-112) and leaves x as it was.
template <int D>
__device__ __forceinline__ bool ldlt_solve(const double* h, double lam, const double (&b)[D], double (&x)[D]) {
    double A[D][D], L[D][D], d[D], y[D];
    {
        int k = 0;
#pragma unroll
        for (int r = 0; r < D; r++)
#pragma unroll
            for (int c = r; c < D; c++, k++) A[r][c] = A[c][r] = h[k];
    }
#pragma unroll
    for (int j = 0; j < D; j++) A[j][j] = A[j][j] + lam;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < D; j++) {
        double s = A[j][j];
#pragma unroll
        for (int k = 0; k < j; k++) s = s - L[j][k] * L[j][k] * d[k];
        if (!(s > 0.0) || !isfinite(s)) ok = false;
        d[j] = s;
#pragma unroll
        for (int i = j + 1; i < D; i++) {
            double t = A[i][j];
#pragma unroll
            for (int k = 0; k < j; k++) t = t - L[i][k] * L[j][k] * d[k];
            L[i][j] = t / s;
        }
    }
    if (!ok) return false;
#pragma unroll
    for (int i = 0; i < D; i++) {
        double t = b[i];
#pragma unroll
        for (int k = 0; k < i; k++) t = t - L[i][k] * y[k];
        y[i] = t;
    }
#pragma unroll
    for (int i = D - 1; i >= 0; i--) {
        double t = y[i] / d[i];
#pragma unroll
        for (int k = i + 1; k < D; k++) t = t - L[k][i] * x[k];
        x[i] = t;
    }
    return true;
}

// The same factorisation for a run-time dimension n, worked by the whole workgroup of T
// threads: A [n][n] row-major in global memory, rows r <= c in use, is overwritten by D (the
// diagonal) and L^T (above it); x [n] in LDS holds b on entry and the solution on return.
// Every entry sees the terms of ldlt_solve in the same order (k ascending, (L L) d), the
// forward substitution likewise; the back substitution subtracts its terms k descending.
// Only a pivot that is exactly zero (or not finite) is a failed solve, as Eigen's
// SimplicialLDLT reports it; x is then left partly worked and the caller discards it.  All
// threads take the same path: the pivot is read by all after a barrier.
template <int T>
__device__ __forceinline__ bool ldlt_solve_block(double* A, int n, double* x) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int j = 0; j < n; j++) {
        double* rj = A + (size_t)j * n;
        const double d = rj[j];
        if (d == 0.0 || !isfinite(d)) return false;
        for (int i = j + 1 + tid; i < n; i += T) rj[i] = rj[i] / d;
        __syncthreads();
        for (int i = j + 1 + wave; i < n; i += T / 64) {
            const double li = rj[i];
            double* ri = A + (size_t)i * n;
            for (int k = i + lane; k < n; k += 64) ri[k] = ri[k] - li * rj[k] * d;
        }
        __syncthreads();
    }
    for (int k = 0; k + 1 < n; k++) {
        const double* rk = A + (size_t)k * n;
        const double xk = x[k];
        for (int i = k + 1 + tid; i < n; i += T) x[i] = x[i] - rk[i] * xk;
        __syncthreads();
    }
    for (int i = tid; i < n; i += T) x[i] = x[i] / A[(size_t)i * n + i];
    __syncthreads();
    for (int k = n - 1; k > 0; k--) {
        const double xk = x[k];
        for (int i = tid; i < k; i += T) x[i] = x[i] - A[(size_t)i * n + k] * xk;
        __syncthreads();
    }
    return true;
}

}  // namespace lm
}  // namespace orbx
