// orbx_epnp.h -- the small algebra of PnPsolver (src/PnPsolver.cc:381-418, 466-1345): EPnP on n
// correspondences and CheckInliers for one point, as plain functions of memory the caller
// provides.  Shared by orbx_pnp.hip (device) and by host builds that check it against the
// float64 model (tests/cpp/epnp_host.cpp): it needs nothing but <cmath>, and must be compiled
// with -ffp-contract=off.  DESIGN.md §4.21.
//
// Conventions (the reference leaves them to OpenCV's cvSVD / cvInvert / cvSolve):
//   * Every "SVD of a symmetric PSD matrix" (the 3x3 PW0^T PW0 and the 12x12 M^T M) is a
//     one-sided (Hestenes) cyclic Jacobi on the symmetric matrix itself, A V = B: pairs (p, q),
//     p < q, in lexicographic order, a pair is rotated unless gamma == 0 or |gamma| <=
//     8 eps sqrt(alpha beta), the sweeps end with the first that rotates nothing, at most 30
//     (orbx_jacobi4.h's constants).  The singular value of column j is |b_j|, its vector is
//     column j of V as the Jacobi leaves it: no sign normalisation.  Descending order; on a tie
//     the higher index is the smaller.  v[0..3] are the vectors of the four smallest values,
//     smallest first (cc:1008-1014).
//   * cvInvert(CC, CV_SVD) (cc:553): CC's columns are k_i u_i with orthonormal u_i, so the
//     inverse's rows are u_i^T / k_i, and a row is zero where k_i == 0.
//   * cvSolve(L, rho, CV_SVD) for the 6x4, 6x3 and 6x5 systems: the same Jacobi on L, L V = B,
//     x = sum_j v_j (b_j . rho) / |b_j|^2 over the columns with |b_j| > 2 eps sum_k |b_k|.
//   * qr_solve (cc:1211-1345) operation for operation, its pivot search that never looks at
//     the last row and its eta == 0 return included; the increment X starts as 0 (the
//     reference's is an uninitialised local before the first solve).
//   * The 3x3 SVD of estimate_R_and_t: one-sided Jacobi, w descending, u_0 and u_1 the
//     normalised columns of B, u_2 = u_0 x u_1 on b_2's side.
// Every sum runs in index order from 0.0; a + b + c is (a + b) + c.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ORBX_HD __host__ __device__ __forceinline__
#else
#define ORBX_HD inline
#endif

namespace orbx {
namespace epnp {

constexpr int kSweeps = 30;
constexpr double kEps = 2.220446049250313e-16;
constexpr double kTol = 8.0 * kEps;
constexpr int kWork = 288;  // doubles of work memory per solve: the 12x12 working matrix and V

// Element i of an array that lives in the caller's memory with a stride (1 on the host and for
// a single thread; the lane count for the lane-minor LDS layout of k_pnp_hyp).
struct Mem {
    double* p;
    int s;
    ORBX_HD double& operator()(int i) const { return p[i * s]; }
    ORBX_HD Mem at(int off) const { return Mem{p + off * s, s}; }
};

// One-sided Jacobi on the rows x n matrix a (row-major, overwritten by B = A V); v is n x n.
ORBX_HD void hestenes(const Mem& a, const Mem& v, int rows, int n) {
#pragma unroll 1
    for (int r = 0; r < n; r++)
#pragma unroll 1
        for (int c = 0; c < n; c++) v(r * n + c) = r == c ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < kSweeps; sweep++) {
        bool rot = false;
#pragma unroll 1
        for (int p = 0; p < n - 1; p++)
#pragma unroll 1
            for (int q = p + 1; q < n; q++) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll 1
                for (int r = 0; r < rows; r++) {
                    const double x = a(r * n + p), y = a(r * n + q);
                    alpha = alpha + x * x;
                    beta = beta + y * y;
                    gamma = gamma + x * y;
                }
                if (gamma == 0.0 || std::fabs(gamma) <= kTol * std::sqrt(alpha * beta)) continue;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = std::copysign(1.0, zeta) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t);
                const double sn = c * t;
#pragma unroll 1
                for (int r = 0; r < rows; r++) {
                    const double x = a(r * n + p), y = a(r * n + q);
                    a(r * n + p) = c * x - sn * y;
                    a(r * n + q) = sn * x + c * y;
                }
#pragma unroll 1
                for (int r = 0; r < n; r++) {
                    const double x = v(r * n + p), y = v(r * n + q);
                    v(r * n + p) = c * x - sn * y;
                    v(r * n + q) = sn * x + c * y;
                }
                rot = true;
            }
        if (!rot) break;
    }
}

// |b_c|^2 of hestenes' result
ORBX_HD double col_norm2(const Mem& a, int rows, int n, int c) {
    double w = 0.0;
#pragma unroll 1
    for (int r = 0; r < rows; r++) w = w + a(r * n + c) * a(r * n + c);
    return w;
}

// cvSolve(L, rho, x, CV_SVD) for the 6 x NC matrix in `a` (destroyed); v is NC x NC.
template <int NC>
ORBX_HD void lsq6(const Mem& a, const Mem& v, const double* rho, double* x) {
    hestenes(a, v, 6, NC);
    double sum = 0.0;
#pragma unroll 1
    for (int j = 0; j < NC; j++) sum = sum + std::sqrt(col_norm2(a, 6, NC, j));
    const double thr = 2.0 * kEps * sum;
#pragma unroll
    for (int i = 0; i < NC; i++) x[i] = 0.0;
#pragma unroll 1
    for (int j = 0; j < NC; j++) {
        const double w2 = col_norm2(a, 6, NC, j);
        if (!(std::sqrt(w2) > thr)) continue;
        double d = 0.0;
#pragma unroll
        for (int r = 0; r < 6; r++) d = d + a(r * NC + j) * rho[r];
        const double coef = d / w2;
#pragma unroll
        for (int i = 0; i < NC; i++) x[i] = x[i] + v(i * NC + j) * coef;
    }
}

// qr_solve (cc:1211-1345) for the 6x4 system of a Gauss-Newton step: a [6][4] and b [6] are
// destroyed, x [4] is left as it was when a pivot column is all zero.
ORBX_HD void qr_solve_6x4(double* a, double* b, double* x) {
    double A1[4], A2[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        double eta = std::fabs(a[4 * k + k]);
#pragma unroll
        for (int i = k; i < 5; i++) {  // cc:1242-1247: rows k .. nr - 2
            const double elt = std::fabs(a[4 * i + k]);
            if (eta < elt) eta = elt;
        }
        if (eta == 0.0) return;  // cc:1250-1255
        const double inv_eta = 1.0 / eta;
        double sum = 0.0;
#pragma unroll
        for (int i = k; i < 6; i++) {
            a[4 * i + k] = a[4 * i + k] * inv_eta;
            sum = sum + a[4 * i + k] * a[4 * i + k];
        }
        double sigma = std::sqrt(sum);
        if (a[4 * k + k] < 0.0) sigma = -sigma;
        a[4 * k + k] = a[4 * k + k] + sigma;
        A1[k] = sigma * a[4 * k + k];
        A2[k] = -eta * sigma;
#pragma unroll
        for (int j = k + 1; j < 4; j++) {
            double s2 = 0.0;
#pragma unroll
            for (int i = k; i < 6; i++) s2 = s2 + a[4 * i + k] * a[4 * i + j];
            const double tau = s2 / A1[k];
#pragma unroll
            for (int i = k; i < 6; i++) a[4 * i + j] = a[4 * i + j] - tau * a[4 * i + k];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {  // b <- Q^T b
        double tau = 0.0;
#pragma unroll
        for (int i = j; i < 6; i++) tau = tau + a[4 * i + j] * b[i];
        tau = tau / A1[j];
#pragma unroll
        for (int i = j; i < 6; i++) b[i] = b[i] - tau * a[4 * i + j];
    }
    x[3] = b[3] / A2[3];
#pragma unroll
    for (int i = 2; i >= 0; i--) {
        double sum = 0.0;
#pragma unroll
        for (int j = i + 1; j < 4; j++) sum = sum + a[4 * i + j] * x[j];
        x[i] = (b[i] - sum) / A2[i];
    }
}

// gauss_newton (cc:1173-1207) with compute_A_and_b_gauss_newton (cc:1076-1170); L is the 6x10
// matrix in memory.
ORBX_HD void gauss_newton(const Mem& L, const double* rho, double* betas) {
    double x[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int it = 0; it < 5; it++) {
        double a[24], b[6];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            double l[10];
#pragma unroll
            for (int c = 0; c < 10; c++) l[c] = L(10 * i + c);
            a[4 * i] = ((2.0 * l[0] * betas[0] + l[1] * betas[1]) + l[3] * betas[2]) + l[6] * betas[3];
            a[4 * i + 1] = ((l[1] * betas[0] + 2.0 * l[2] * betas[1]) + l[4] * betas[2]) + l[7] * betas[3];
            a[4 * i + 2] = ((l[3] * betas[0] + l[4] * betas[1]) + 2.0 * l[5] * betas[2]) + l[8] * betas[3];
            a[4 * i + 3] = ((l[6] * betas[0] + l[7] * betas[1]) + l[8] * betas[2]) + 2.0 * l[9] * betas[3];
            double s = l[0] * betas[0] * betas[0];
            s = s + l[1] * betas[0] * betas[1];
            s = s + l[2] * betas[1] * betas[1];
            s = s + l[3] * betas[0] * betas[2];
            s = s + l[4] * betas[1] * betas[2];
            s = s + l[5] * betas[2] * betas[2];
            s = s + l[6] * betas[0] * betas[3];
            s = s + l[7] * betas[1] * betas[3];
            s = s + l[8] * betas[2] * betas[3];
            s = s + l[9] * betas[3] * betas[3];
            b[i] = rho[i] - s;
        }
        qr_solve_6x4(a, b, x);
#pragma unroll
        for (int i = 0; i < 4; i++) betas[i] = betas[i] + x[i];
    }
}

ORBX_HD double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

template <int P, int Q>
ORBX_HD bool rot3(double* B, double* V) {
    const double alpha = (B[P] * B[P] + B[3 + P] * B[3 + P]) + B[6 + P] * B[6 + P];
    const double beta = (B[Q] * B[Q] + B[3 + Q] * B[3 + Q]) + B[6 + Q] * B[6 + Q];
    const double gamma = (B[P] * B[Q] + B[3 + P] * B[3 + Q]) + B[6 + P] * B[6 + Q];
    if (gamma == 0.0 || std::fabs(gamma) <= kTol * std::sqrt(alpha * beta)) return false;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = std::copysign(1.0, zeta) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / std::sqrt(1.0 + t * t);
    const double s = c * t;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        double x = B[3 * r + P];
        B[3 * r + P] = c * x - s * B[3 * r + Q];
        B[3 * r + Q] = s * x + c * B[3 * r + Q];
        x = V[3 * r + P];
        V[3 * r + P] = c * x - s * V[3 * r + Q];
        V[3 * r + Q] = s * x + c * V[3 * r + Q];
    }
    return true;
}

template <int P, int Q>
ORBX_HD void swap_cols3(double* B, double* V, double* w) {
    if (w[P] < w[Q]) {
        double x = w[P]; w[P] = w[Q]; w[Q] = x;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            x = B[3 * r + P]; B[3 * r + P] = B[3 * r + Q]; B[3 * r + Q] = x;
            x = V[3 * r + P]; V[3 * r + P] = V[3 * r + Q]; V[3 * r + Q] = x;
        }
    }
}

// R = U V^T of the 3x3 A = U diag(w) V^T (cc:824-829)
ORBX_HD void rotation_of(const double* A, double* R) {
    double B[9], V[9], w[3], U[9];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        B[i] = A[i];
        V[i] = (i % 4 == 0) ? 1.0 : 0.0;
    }
#pragma unroll 1
    for (int sweep = 0; sweep < kSweeps; sweep++) {
        bool rot = false;
        rot |= rot3<0, 1>(B, V);
        rot |= rot3<0, 2>(B, V);
        rot |= rot3<1, 2>(B, V);
        if (!rot) break;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) w[c] = std::sqrt((B[c] * B[c] + B[3 + c] * B[3 + c]) + B[6 + c] * B[6 + c]);
    swap_cols3<0, 1>(B, V, w);
    swap_cols3<1, 2>(B, V, w);
    swap_cols3<0, 1>(B, V, w);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        U[3 * r] = B[3 * r] / w[0];
        U[3 * r + 1] = B[3 * r + 1] / w[1];
    }
    double c0 = U[3] * U[7] - U[6] * U[4], c1 = U[6] * U[1] - U[0] * U[7], c2 = U[0] * U[4] - U[3] * U[1];
    if ((c0 * B[2] + c1 * B[5]) + c2 * B[8] < 0.0) {
        c0 = -c0;
        c1 = -c1;
        c2 = -c2;
    }
    U[2] = c0;
    U[5] = c1;
    U[8] = c2;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) R[3 * i + j] = dot3(U + 3 * i, V + 3 * j);
}

struct Camera {
    double fu, fv, uc, vc;
};

// compute_R_and_t (cc:877-892): compute_ccs, compute_pcs, solve_for_sign, estimate_R_and_t and
// reprojection_error for one set of betas.  V12 is the 12x12 V, vi the columns of v[0..3].
ORBX_HD double compute_R_and_t(int n, const Mem& pws, const Mem& us, const Mem& alphas, const Mem& pcs,
                               const Mem& V12, const int* vi, const double* betas, const Camera& K, double* R,
                               double* t) {
    double ccs[12];
#pragma unroll
    for (int i = 0; i < 12; i++) ccs[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 12; j++) ccs[j] = ccs[j] + betas[i] * V12(j * 12 + vi[i]);  // cc:609-625
#pragma unroll 1
    for (int i = 0; i < n; i++) {  // cc:629-641
#pragma unroll
        for (int j = 0; j < 3; j++)
            pcs(3 * i + j) = ((alphas(4 * i) * ccs[j] + alphas(4 * i + 1) * ccs[3 + j]) + alphas(4 * i + 2) * ccs[6 + j]) +
                             alphas(4 * i + 3) * ccs[9 + j];
    }
    if (pcs(2) < 0.0) {  // solve_for_sign (cc:857-874); ccs is not read again
#pragma unroll 1
        for (int i = 0; i < 3 * n; i++) pcs(i) = -pcs(i);
    }
    double pc0[3] = {0.0, 0.0, 0.0}, pw0[3] = {0.0, 0.0, 0.0};  // cc:776-846
#pragma unroll 1
    for (int i = 0; i < n; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            pc0[j] = pc0[j] + pcs(3 * i + j);
            pw0[j] = pw0[j] + pws(3 * i + j);
        }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        pc0[j] = pc0[j] / (double)n;
        pw0[j] = pw0[j] / (double)n;
    }
    double abt[9];
#pragma unroll
    for (int i = 0; i < 9; i++) abt[i] = 0.0;
#pragma unroll 1
    for (int i = 0; i < n; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int m = 0; m < 3; m++)
                abt[3 * j + m] = abt[3 * j + m] + (pcs(3 * i + j) - pc0[j]) * (pws(3 * i + m) - pw0[m]);
    rotation_of(abt, R);
    const double det = ((((R[0] * R[4] * R[8] + R[1] * R[5] * R[6]) + R[2] * R[3] * R[7]) - R[2] * R[4] * R[6]) -
                        R[1] * R[3] * R[8]) -
                       R[0] * R[5] * R[7];
    if (det < 0.0) {
        R[6] = -R[6];
        R[7] = -R[7];
        R[8] = -R[8];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) t[i] = pc0[i] - dot3(R + 3 * i, pw0);
    double sum2 = 0.0;  // cc:750-773: the mean of the distances
#pragma unroll 1
    for (int i = 0; i < n; i++) {
        const double pw[3] = {pws(3 * i), pws(3 * i + 1), pws(3 * i + 2)};
        const double Xc = dot3(R, pw) + t[0], Yc = dot3(R + 3, pw) + t[1];
        const double inv_Zc = 1.0 / (dot3(R + 6, pw) + t[2]);
        const double ue = K.uc + K.fu * Xc * inv_Zc, ve = K.vc + K.fv * Yc * inv_Zc;
        const double du = us(2 * i) - ue, dv = us(2 * i + 1) - ve;
        sum2 = sum2 + std::sqrt(du * du + dv * dv);
    }
    return sum2 / (double)n;
}

// compute_pose (cc:644-719) on the n correspondences pws [3n] / us [2n]; alphas [4n] and pcs
// [3n] are work arrays, W holds kWork doubles.  R [9], t [3] out; returns the reprojection error.
ORBX_HD double compute_pose(int n, const Mem& pws, const Mem& us, const Mem& alphas, const Mem& pcs, const Mem& W,
                            const Camera& K, double* R, double* t) {
    const Mem A = W, V = W.at(144);
    const double dn = (double)n;
    // choose_control_points (cc:467-522)
    double cws[12];
#pragma unroll
    for (int j = 0; j < 3; j++) cws[j] = 0.0;
#pragma unroll 1
    for (int i = 0; i < n; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) cws[j] = cws[j] + pws(3 * i + j);
#pragma unroll
    for (int j = 0; j < 3; j++) cws[j] = cws[j] / dn;
    {
        double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // xx xy xz yy yz zz
#pragma unroll 1
        for (int i = 0; i < n; i++) {
            const double x = pws(3 * i) - cws[0], y = pws(3 * i + 1) - cws[1], z = pws(3 * i + 2) - cws[2];
            m[0] = m[0] + x * x;
            m[1] = m[1] + x * y;
            m[2] = m[2] + x * z;
            m[3] = m[3] + y * y;
            m[4] = m[4] + y * z;
            m[5] = m[5] + z * z;
        }
        A(0) = m[0]; A(1) = m[1]; A(2) = m[2];
        A(3) = m[1]; A(4) = m[3]; A(5) = m[4];
        A(6) = m[2]; A(7) = m[4]; A(8) = m[5];
    }
    hestenes(A, V, 3, 3);
    double uct[9], kk[3];
    {
        const double w0 = std::sqrt(col_norm2(A, 3, 3, 0)), w1 = std::sqrt(col_norm2(A, 3, 3, 1)),
                     w2 = std::sqrt(col_norm2(A, 3, 3, 2));
        // descending, a tie keeps the lower index first
        int o0 = 0, o1 = 1, o2 = 2;
        double d0 = w0, d1 = w1, d2 = w2;
        if (d0 < d1) { double x = d0; d0 = d1; d1 = x; int y = o0; o0 = o1; o1 = y; }
        if (d1 < d2) { double x = d1; d1 = d2; d2 = x; int y = o1; o1 = o2; o2 = y; }
        if (d0 < d1) { double x = d0; d0 = d1; d1 = x; int y = o0; o0 = o1; o1 = y; }
        kk[0] = std::sqrt(d0 / dn);
        kk[1] = std::sqrt(d1 / dn);
        kk[2] = std::sqrt(d2 / dn);
#pragma unroll
        for (int j = 0; j < 3; j++) {
            uct[j] = V(3 * j + o0);
            uct[3 + j] = V(3 * j + o1);
            uct[6 + j] = V(3 * j + o2);
        }
    }
#pragma unroll
    for (int i = 1; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) cws[3 * i + j] = cws[j] + kk[i - 1] * uct[3 * (i - 1) + j];
    // compute_barycentric_coordinates (cc:532-576) with the closed-form inverse
    double ci[9];
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int m = 0; m < 3; m++) ci[3 * j + m] = kk[j] == 0.0 ? 0.0 : uct[3 * j + m] / kk[j];
#pragma unroll 1
    for (int i = 0; i < n; i++) {
        const double x = pws(3 * i) - cws[0], y = pws(3 * i + 1) - cws[1], z = pws(3 * i + 2) - cws[2];
        const double a1 = (ci[0] * x + ci[1] * y) + ci[2] * z;
        const double a2 = (ci[3] * x + ci[4] * y) + ci[5] * z;
        const double a3 = (ci[6] * x + ci[7] * y) + ci[8] * z;
        alphas(4 * i) = ((1.0 - a1) - a2) - a3;
        alphas(4 * i + 1) = a1;
        alphas(4 * i + 2) = a2;
        alphas(4 * i + 3) = a3;
    }
    // fill_M (cc:587-605) and M^T M (cc:667), point by point: the upper triangle, then mirrored
#pragma unroll 1
    for (int i = 0; i < 144; i++) A(i) = 0.0;
    const Mem M1 = V, M2 = V.at(12);  // the two rows of a point, in memory V does not use yet
#pragma unroll 1
    for (int i = 0; i < n; i++) {
        const double du = K.uc - us(2 * i), dv = K.vc - us(2 * i + 1);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const double a = alphas(4 * i + j);
            M1(3 * j) = a * K.fu;
            M1(3 * j + 1) = 0.0;
            M1(3 * j + 2) = a * du;
            M2(3 * j) = 0.0;
            M2(3 * j + 1) = a * K.fv;
            M2(3 * j + 2) = a * dv;
        }
#pragma unroll 1
        for (int a = 0; a < 12; a++) {
            const double m1 = M1(a), m2 = M2(a);
#pragma unroll 1
            for (int b = a; b < 12; b++) A(12 * a + b) = (A(12 * a + b) + m1 * M1(b)) + m2 * M2(b);
        }
    }
#pragma unroll 1
    for (int a = 1; a < 12; a++)
#pragma unroll 1
        for (int b = 0; b < a; b++) A(12 * a + b) = A(12 * b + a);
    hestenes(A, V, 12, 12);
    // the four smallest, smallest first; on a tie the higher index is the smaller
    int vi[4];
    {
        unsigned taken = 0u;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            int bc = -1;
            double best = 0.0;
#pragma unroll 1
            for (int c = 0; c < 12; c++) {
                if (taken & (1u << c)) continue;
                const double w = col_norm2(A, 12, 12, c);
                if (bc < 0 || w <= best) {
                    best = w;
                    bc = c;
                }
            }
            taken |= 1u << bc;
            vi[k] = bc;
        }
    }
    // compute_L_6x10 (cc:1002-1061) into the freed working matrix, compute_rho (cc:1064-1073)
    const Mem L = A;
    {
        const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {1, 2, 3, 2, 3, 3};
#pragma unroll
        for (int r = 0; r < 6; r++) {
            double dv[4][3];
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int c = 0; c < 3; c++) dv[i][c] = V((3 * pa[r] + c) * 12 + vi[i]) - V((3 * pb[r] + c) * 12 + vi[i]);
            L(10 * r) = dot3(dv[0], dv[0]);
            L(10 * r + 1) = 2.0 * dot3(dv[0], dv[1]);
            L(10 * r + 2) = dot3(dv[1], dv[1]);
            L(10 * r + 3) = 2.0 * dot3(dv[0], dv[2]);
            L(10 * r + 4) = 2.0 * dot3(dv[1], dv[2]);
            L(10 * r + 5) = dot3(dv[2], dv[2]);
            L(10 * r + 6) = 2.0 * dot3(dv[0], dv[3]);
            L(10 * r + 7) = 2.0 * dot3(dv[1], dv[3]);
            L(10 * r + 8) = 2.0 * dot3(dv[2], dv[3]);
            L(10 * r + 9) = dot3(dv[3], dv[3]);
        }
    }
    double rho[6];
    {
        const int pa[6] = {0, 0, 0, 1, 1, 2}, pb[6] = {1, 2, 3, 2, 3, 3};
#pragma unroll
        for (int r = 0; r < 6; r++) {
            const double dx = cws[3 * pa[r]] - cws[3 * pb[r]], dy = cws[3 * pa[r] + 1] - cws[3 * pb[r] + 1],
                         dz = cws[3 * pa[r] + 2] - cws[3 * pb[r] + 2];
            rho[r] = (dx * dx + dy * dy) + dz * dz;
        }
    }
    const Mem S = W.at(60), SV = W.at(90);  // the 6 x NC system and its V
    double betas[4], Rn[9], tn[3];
    // N = 4 (cc:897-926)
    {
        double b4[4];
#pragma unroll 1
        for (int r = 0; r < 6; r++) {
            S(4 * r) = L(10 * r);
            S(4 * r + 1) = L(10 * r + 1);
            S(4 * r + 2) = L(10 * r + 3);
            S(4 * r + 3) = L(10 * r + 6);
        }
        lsq6<4>(S, SV, rho, b4);
        if (b4[0] < 0.0) {
            betas[0] = std::sqrt(-b4[0]);
            betas[1] = -b4[1] / betas[0];
            betas[2] = -b4[2] / betas[0];
            betas[3] = -b4[3] / betas[0];
        } else {
            betas[0] = std::sqrt(b4[0]);
            betas[1] = b4[1] / betas[0];
            betas[2] = b4[2] / betas[0];
            betas[3] = b4[3] / betas[0];
        }
    }
    gauss_newton(L, rho, betas);
    double err = compute_R_and_t(n, pws, us, alphas, pcs, V, vi, betas, K, R, t);
    // N = 2 (cc:931-962)
    {
        double b3[3];
#pragma unroll 1
        for (int r = 0; r < 6; r++) {
            S(3 * r) = L(10 * r);
            S(3 * r + 1) = L(10 * r + 1);
            S(3 * r + 2) = L(10 * r + 2);
        }
        lsq6<3>(S, SV, rho, b3);
        if (b3[0] < 0.0) {
            betas[0] = std::sqrt(-b3[0]);
            betas[1] = (b3[2] < 0.0) ? std::sqrt(-b3[2]) : 0.0;
        } else {
            betas[0] = std::sqrt(b3[0]);
            betas[1] = (b3[2] > 0.0) ? std::sqrt(b3[2]) : 0.0;
        }
        if (b3[1] < 0.0) betas[0] = -betas[0];
        betas[2] = 0.0;
        betas[3] = 0.0;
    }
    gauss_newton(L, rho, betas);
    double e = compute_R_and_t(n, pws, us, alphas, pcs, V, vi, betas, K, Rn, tn);
    if (e < err) {  // cc:711
        err = e;
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = Rn[i];
#pragma unroll
        for (int i = 0; i < 3; i++) t[i] = tn[i];
    }
    // N = 3 (cc:967-999)
    {
        double b5[5];
#pragma unroll 1
        for (int r = 0; r < 6; r++)
#pragma unroll 1
            for (int c = 0; c < 5; c++) S(5 * r + c) = L(10 * r + c);
        lsq6<5>(S, SV, rho, b5);
        if (b5[0] < 0.0) {
            betas[0] = std::sqrt(-b5[0]);
            betas[1] = (b5[2] < 0.0) ? std::sqrt(-b5[2]) : 0.0;
        } else {
            betas[0] = std::sqrt(b5[0]);
            betas[1] = (b5[2] > 0.0) ? std::sqrt(b5[2]) : 0.0;
        }
        if (b5[1] < 0.0) betas[0] = -betas[0];
        betas[2] = b5[3] / betas[0];
        betas[3] = 0.0;
    }
    gauss_newton(L, rho, betas);
    e = compute_R_and_t(n, pws, us, alphas, pcs, V, vi, betas, K, Rn, tn);
    if (e < err) {  // cc:712
        err = e;
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = Rn[i];
#pragma unroll
        for (int i = 0; i < 3; i++) t[i] = tn[i];
    }
    return err;
}

// CheckInliers for one correspondence (cc:389-408) with its mixed precision: Xc, Yc, invZc and
// the two differences are floats, ue / ve doubles, error2 = distX * distX + distY * distY in
// float with two roundings (the pragma keeps the compiler from fusing them whatever the
// command line says), the comparison strict; a NaN error2 is an outlier.
ORBX_HD bool check_inlier(const double* R, const double* t, const Camera& K, float X, float Y, float Z, float u,
                          float v, float max_error) {
#pragma clang fp contract(off)
    const double x = (double)X, y = (double)Y, z = (double)Z;
    const float Xc = (float)((((R[0] * x + R[1] * y) + R[2] * z)) + t[0]);
    const float Yc = (float)((((R[3] * x + R[4] * y) + R[5] * z)) + t[1]);
    const float invZc = (float)(1.0 / ((((R[6] * x + R[7] * y) + R[8] * z)) + t[2]));
    const double ue = K.uc + K.fu * (double)Xc * (double)invZc;
    const double ve = K.vc + K.fv * (double)Yc * (double)invZc;
    const float distX = (float)((double)u - ue);
    const float distY = (float)((double)v - ve);
    const float xx = distX * distX, yy = distY * distY;
    const float error2 = xx + yy;
    return error2 < max_error;
}

}  // namespace epnp
}  // namespace orbx
