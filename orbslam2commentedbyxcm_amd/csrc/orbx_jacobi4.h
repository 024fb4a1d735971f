// orbx_jacobi4.h -- the 4x4 one-sided (Hestenes) Jacobi of the linear triangulation, shared by
// orbx_triangulate.hip (LocalMapping::CreateNewMapPoints) and orbx_initializer.hip
// (Initializer::Triangulate).  Fully unrolled over 32 named doubles (no runtime-indexed array,
// so nothing goes to scratch): a sweep visits the six column pairs in the order (0,1) (0,2)
// (0,3) (1,2) (1,3) (2,3), a pair is rotated unless |a_i . a_j| <= 8 eps |a_i| |a_j|, the sweeps
// end with the first one that rotates nothing or after kSweepCap.
#pragma once

#include <hip/hip_runtime.h>

namespace orbx {

constexpr int kSweepCap = 30;
constexpr double kJacobiTol = 8.0 * 2.220446049250313e-16;

// One Hestenes rotation of columns a, b of the working matrix and of V.  Returns whether it rotated.
__device__ __forceinline__ bool jacobi_pair(double& a0, double& a1, double& a2, double& a3, double& b0, double& b1,
                                            double& b2, double& b3, double& va0, double& va1, double& va2,
                                            double& va3, double& vb0, double& vb1, double& vb2, double& vb3) {
    const double alpha = ((a0 * a0 + a1 * a1) + a2 * a2) + a3 * a3;
    const double beta = ((b0 * b0 + b1 * b1) + b2 * b2) + b3 * b3;
    const double gamma = ((a0 * b0 + a1 * b1) + a2 * b2) + a3 * b3;
    if (gamma == 0.0 || fabs(gamma) <= kJacobiTol * sqrt(alpha * beta)) return false;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t);
    const double s = c * t;
    double x;
    x = a0; a0 = c * x - s * b0; b0 = s * x + c * b0;
    x = a1; a1 = c * x - s * b1; b1 = s * x + c * b1;
    x = a2; a2 = c * x - s * b2; b2 = s * x + c * b2;
    x = a3; a3 = c * x - s * b3; b3 = s * x + c * b3;
    x = va0; va0 = c * x - s * vb0; vb0 = s * x + c * vb0;
    x = va1; va1 = c * x - s * vb1; vb1 = s * x + c * vb1;
    x = va2; va2 = c * x - s * vb2; vb2 = s * x + c * vb2;
    x = va3; va3 = c * x - s * vb3; vb3 = s * x + c * vb3;
    return true;
}

// The right singular vector of the smallest singular value of the 4x4 matrix with rows r0..r3
// (each 4 doubles by value), as h0..h3.
__device__ __forceinline__ void smallest_right_singular_vector(
    double a00, double a01, double a02, double a03, double a10, double a11, double a12, double a13, double a20,
    double a21, double a22, double a23, double a30, double a31, double a32, double a33, double& h0, double& h1,
    double& h2, double& h3) {
    // column j of the working matrix: a0j a1j a2j a3j; column j of V: v0j v1j v2j v3j
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v03 = 0.0;
    double v10 = 0.0, v11 = 1.0, v12 = 0.0, v13 = 0.0;
    double v20 = 0.0, v21 = 0.0, v22 = 1.0, v23 = 0.0;
    double v30 = 0.0, v31 = 0.0, v32 = 0.0, v33 = 1.0;
    for (int sweep = 0; sweep < kSweepCap; sweep++) {
        bool rot = false;
        rot |= jacobi_pair(a00, a10, a20, a30, a01, a11, a21, a31, v00, v10, v20, v30, v01, v11, v21, v31);
        rot |= jacobi_pair(a00, a10, a20, a30, a02, a12, a22, a32, v00, v10, v20, v30, v02, v12, v22, v32);
        rot |= jacobi_pair(a00, a10, a20, a30, a03, a13, a23, a33, v00, v10, v20, v30, v03, v13, v23, v33);
        rot |= jacobi_pair(a01, a11, a21, a31, a02, a12, a22, a32, v01, v11, v21, v31, v02, v12, v22, v32);
        rot |= jacobi_pair(a01, a11, a21, a31, a03, a13, a23, a33, v01, v11, v21, v31, v03, v13, v23, v33);
        rot |= jacobi_pair(a02, a12, a22, a32, a03, a13, a23, a33, v02, v12, v22, v32, v03, v13, v23, v33);
        if (!rot) break;
    }
    const double n0 = ((a00 * a00 + a10 * a10) + a20 * a20) + a30 * a30;
    const double n1 = ((a01 * a01 + a11 * a11) + a21 * a21) + a31 * a31;
    const double n2 = ((a02 * a02 + a12 * a12) + a22 * a22) + a32 * a32;
    const double n3 = ((a03 * a03 + a13 * a13) + a23 * a23) + a33 * a33;
    double best = n0;
    h0 = v00; h1 = v10; h2 = v20; h3 = v30;
    if (n1 <= best) { best = n1; h0 = v01; h1 = v11; h2 = v21; h3 = v31; }
    if (n2 <= best) { best = n2; h0 = v02; h1 = v12; h2 = v22; h3 = v32; }
    if (n3 <= best) { best = n3; h0 = v03; h1 = v13; h2 = v23; h3 = v33; }
}

}  // namespace orbx
