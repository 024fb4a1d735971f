// orbx_sim3.h -- g2o::Sim3 (types/sim3.h) for the kernels that optimise over it
// (orbx_optsim3.hip, orbx_essgraph.hip): a quaternion that is never normalised, a translation
// and a scale, with operator*, inverse, the exponential map, the logarithm and the conversion
// to [R | t / s].  Everything is double and every function is inlined into its kernel.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "orbx_lm.h"

namespace orbx {

struct S3 {
    double qx, qy, qz, qw, tx, ty, tz, s;
};

// Sim3::operator*, sim3.h:266-272
__host__ __device__ __forceinline__ S3 s3_mul(const S3& a, const S3& b) {
    S3 o;
    o.qx = a.qw * b.qx + a.qx * b.qw + a.qy * b.qz - a.qz * b.qy;
    o.qy = a.qw * b.qy + a.qy * b.qw + a.qz * b.qx - a.qx * b.qz;
    o.qz = a.qw * b.qz + a.qz * b.qw + a.qx * b.qy - a.qy * b.qx;
    o.qw = a.qw * b.qw - a.qx * b.qx - a.qy * b.qy - a.qz * b.qz;
    double ux = a.qy * b.tz - a.qz * b.ty, uy = a.qz * b.tx - a.qx * b.tz, uz = a.qx * b.ty - a.qy * b.tx;
    ux += ux;
    uy += uy;
    uz += uz;
    const double rx = b.tx + a.qw * ux + (a.qy * uz - a.qz * uy);
    const double ry = b.ty + a.qw * uy + (a.qz * ux - a.qx * uz);
    const double rz = b.tz + a.qw * uz + (a.qx * uy - a.qy * ux);
    o.tx = a.s * rx + a.tx;
    o.ty = a.s * ry + a.ty;
    o.tz = a.s * rz + a.tz;
    o.s = a.s * b.s;
    return o;
}

// Sim3::inverse, sim3.h:233-236
__device__ __forceinline__ S3 s3_inverse(const S3& a) {
    S3 o;
    o.qx = -a.qx;
    o.qy = -a.qy;
    o.qz = -a.qz;
    o.qw = a.qw;
    const double k = -1. / a.s;
    lm::quat_rotate(o.qx, o.qy, o.qz, o.qw, k * a.tx, k * a.ty, k * a.tz, o.tx, o.ty, o.tz);
    o.s = 1. / a.s;
    return o;
}

// Sim3(const Vector7d& update), sim3.h:70-142: update = (omega, upsilon, sigma)
__host__ __device__ __forceinline__ S3 s3_exp(const double (&x)[7]) {
    const double w0 = x[0], w1 = x[1], w2 = x[2], sigma = x[6];
    const double theta = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
    const double O[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
    const double s = exp(sigma);
    double O2[3][3], R[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) O2[i][j] = O[i][0] * O[0][j] + O[i][1] * O[1][j] + O[i][2] * O[2][j];
    const double eps = 0.00001;
    double A, B, C;
    const bool small_theta = theta < eps;
    double ra = 1.0, rb = 1.0;  // R = I + ra Omega + rb Omega2
    if (!small_theta) {
        ra = sin(theta) / theta;
        rb = (1 - cos(theta)) / (theta * theta);
    }
    if (fabs(sigma) < eps) {
        C = 1;
        if (small_theta) {
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = (1 - cos(theta)) / (theta2);
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (small_theta) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sin(theta);
            const double b = s * cos(theta);
            const double theta2 = theta * theta;
            const double sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    double W[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double id = i == j ? 1.0 : 0.0;
            R[i][j] = small_theta ? id + O[i][j] + O2[i][j] : id + ra * O[i][j] + rb * O2[i][j];
            W[i][j] = A * O[i][j] + B * O2[i][j] + C * id;
        }
    double q[4];
    lm::quat_from_matrix(R, q);
    S3 o;
    o.qx = q[0];
    o.qy = q[1];
    o.qz = q[2];
    o.qw = q[3];
    o.tx = W[0][0] * x[3] + W[0][1] * x[4] + W[0][2] * x[5];
    o.ty = W[1][0] * x[3] + W[1][1] * x[4] + W[1][2] * x[5];
    o.tz = W[2][0] * x[3] + W[2][1] * x[4] + W[2][2] * x[5];
    o.s = s;
    return o;
}

__device__ __forceinline__ S3 s3_load(const double* p) {
    S3 o;
    o.qx = p[0];
    o.qy = p[1];
    o.qz = p[2];
    o.qw = p[3];
    o.tx = p[4];
    o.ty = p[5];
    o.tz = p[6];
    o.s = p[7];
    return o;
}

__device__ __forceinline__ void s3_store(double* p, const S3& a) {
    p[0] = a.qx;
    p[1] = a.qy;
    p[2] = a.qz;
    p[3] = a.qw;
    p[4] = a.tx;
    p[5] = a.ty;
    p[6] = a.tz;
    p[7] = a.s;
}

// Sim3::map, sim3.h:144-146
__device__ __forceinline__ void s3_map(const S3& a, double X, double Y, double Z, double& x, double& y, double& z) {
    double rx, ry, rz;
    lm::quat_rotate(a.qx, a.qy, a.qz, a.qw, X, Y, Z, rx, ry, rz);
    x = a.s * rx + a.tx;
    y = a.s * ry + a.ty;
    z = a.s * rz + a.tz;
}

// W x = t by Eigen's PartialPivLU (sim3.h:217): the pivot of a column is its entry of largest
// absolute value, the first on ties; unit-lower forward and upper back substitution, each
// row's products summed before they are subtracted
__device__ __forceinline__ void lu3_solve(double (&W)[3][3], const double (&t)[3], double (&x)[3]) {
    double b[3] = {t[0], t[1], t[2]};
#pragma unroll
    for (int k = 0; k < 2; k++) {
        int p = k;
        double best = fabs(W[k][k]);
#pragma unroll
        for (int i = k + 1; i < 3; i++)
            if (fabs(W[i][k]) > best) {
                best = fabs(W[i][k]);
                p = i;
            }
#pragma unroll
        for (int i = k + 1; i < 3; i++)
            if (p == i) {
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const double v = W[k][c];
                    W[k][c] = W[i][c];
                    W[i][c] = v;
                }
                const double v = b[k];
                b[k] = b[i];
                b[i] = v;
            }
#pragma unroll
        for (int i = k + 1; i < 3; i++) {
            W[i][k] = W[i][k] / W[k][k];
#pragma unroll
            for (int c = k + 1; c < 3; c++) W[i][c] = W[i][c] - W[i][k] * W[k][c];
        }
    }
    const double c0 = b[0];
    const double c1 = b[1] - W[1][0] * c0;
    const double c2 = b[2] - (W[2][0] * c0 + W[2][1] * c1);
    x[2] = c2 / W[2][2];
    x[1] = (c1 - W[1][2] * x[2]) / W[1][1];
    x[0] = (c0 - (W[0][1] * x[1] + W[0][2] * x[2])) / W[0][0];
}

// Sim3::log, sim3.h:148-230: res = (omega, upsilon, sigma)
__device__ __forceinline__ void s3_log(const S3& a, double (&res)[7]) {
    const double s = a.s;
    const double sigma = log(s);
    double R[3][3];
    lm::quat_to_matrix(a.qx, a.qy, a.qz, a.qw, R);
    const double d = 0.5 * (R[0][0] + R[1][1] + R[2][2] - 1);
    const double dR[3] = {R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]};  // deltaR, se3_ops.hpp:40-47
    const double eps = 0.00001;
    const bool small_rot = d > 1 - eps;
    double theta = 0.0, k = 0.5;
    if (!small_rot) {
        theta = acos(d);
        k = theta / (2 * sqrt(1 - d * d));
    }
    const double w0 = k * dR[0], w1 = k * dR[1], w2 = k * dR[2];
    double A, B, C;
    if (fabs(sigma) < eps) {
        C = 1;
        if (small_rot) {
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = (1 - cos(theta)) / (theta2);
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (small_rot) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / (sigma2);
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double theta2 = theta * theta;
            const double sa = s * sin(theta);
            const double sb = s * cos(theta);
            const double c = theta2 + sigma * sigma;
            A = (sa * sigma + (1 - sb) * theta) / (theta * c);
            B = (C - ((sb - 1) * sigma + sa * theta) / (c)) * 1. / (theta2);
        }
    }
    // W = A Omega + (B Omega) Omega + C I
    const double O[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
    double W[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double bo2 = (B * O[i][0]) * O[0][j] + (B * O[i][1]) * O[1][j] + (B * O[i][2]) * O[2][j];
            W[i][j] = A * O[i][j] + bo2 + (i == j ? C : 0.0);
        }
    const double t[3] = {a.tx, a.ty, a.tz};
    double u[3];
    lu3_solve(W, t, u);
    res[0] = w0;
    res[1] = w1;
    res[2] = w2;
    res[3] = u[0];
    res[4] = u[1];
    res[5] = u[2];
    res[6] = sigma;
}

// The Sim3 as the pose [R | t / s] (Optimizer.cc:1106-1112): toRotationMatrix, eigt *= 1. / s,
// Converter::toCvSE3's casts to float; T: rows 0..2 of Tcw
__device__ __forceinline__ void s3_to_tcw(const S3& a, float* T) {
    double R[3][3];
    lm::quat_to_matrix(a.qx, a.qy, a.qz, a.qw, R);
    const double k = 1. / a.s;
    const double t[3] = {a.tx * k, a.ty * k, a.tz * k};
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) T[4 * r + c] = (float)R[r][c];
        T[4 * r + 3] = (float)t[r];
    }
}

// g2o::Sim3(Rcw, tcw, 1.0) of a pose's rows 0..2 (Optimizer.cc:927-929): Quaterniond(R), not
// normalised
__device__ __forceinline__ S3 s3_from_tcw(const float* T) {
    double R[3][3], q[4];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) R[r][c] = (double)T[4 * r + c];
    lm::quat_from_matrix(R, q);
    S3 o;
    o.qx = q[0];
    o.qy = q[1];
    o.qz = q[2];
    o.qw = q[3];
    o.tx = (double)T[3];
    o.ty = (double)T[7];
    o.tz = (double)T[11];
    o.s = 1.0;
    return o;
}

// The 14 probe increments Sim3(+-1e-9 e_d) of g2o's central difference
// (base_binary_edge.hpp:147-196), index 2 d + (0: +delta, 1: -delta), as q xyzw, t, s, by the
// host's libm; with fix_scale oplusImpl zeroes the seventh entry, so both of its probes are
// Sim3(0)
inline void s3_probe_increments(bool fix_scale, double* out) {
    static_assert(sizeof(S3) == 8 * sizeof(double), "probe layout");
    for (int d = 0; d < 7; d++)
        for (int sgn = 0; sgn < 2; sgn++) {
            double x[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            x[d] = sgn ? -1e-9 : 1e-9;
            if (fix_scale) x[6] = 0;
            const S3 p = s3_exp(x);
            const double v[8] = {p.qx, p.qy, p.qz, p.qw, p.tx, p.ty, p.tz, p.s};
            for (int k = 0; k < 8; k++) out[(2 * d + sgn) * 8 + k] = v[k];
        }
}

}  // namespace orbx
