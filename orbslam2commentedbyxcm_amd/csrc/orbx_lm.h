// orbx_lm.h -- device pieces shared by the dense Levenberg-Marquardt kernels (orbx_poseopt.hip,
// orbx_optsim3.hip): Eigen's quaternion formulas, g2o's Huber kernel, the fixed-shape workgroup
// sums and the dense LDL^T of linear_solver_dense.h.  Everything is double and every function
// is inlined into its kernel.
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

}  // namespace lm
}  // namespace orbx
