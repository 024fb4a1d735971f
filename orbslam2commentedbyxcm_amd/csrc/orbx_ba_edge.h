// orbx_ba_edge.h -- the projection edges shared by the bundle-adjustment kernels
// (orbx_localba.hip, orbx_globalba.hip): EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ with their
// analytic Jacobians, and the pose record both kernels keep per keyframe.
//
// Reference, under Thirdparty/g2o/g2o:
//   types/types_six_dof_expmap.cpp:103-157, 188-234   Jacobians, cam_project (stereo: float
//                                                     invz and the float product bf * invz)
//   types/types_six_dof_expmap.h                      computeError
//   src/Converter.cc                                  toSE3Quat
// Everything is double but the two float intermediates of the stereo projection, and every
// function is inlined into its kernel.
#pragma once

#include <hip/hip_runtime.h>

#include "orbx_lm.h"

namespace orbx {
namespace ba {

constexpr int kValid = 1, kStereo = 2, kLevel1 = 4;  // an edge record's flags
constexpr int kPoseWords = 16;                       // q xyzw, t, R

struct Cam {
    double fx, fy, cx, cy, bf;
    float bf_f;
    double delta_mono, delta_stereo;  // the caller's float Huber deltas (Optimizer.cc:650-653, 115-116), widened
};

// Converter::toSE3Quat into a pose record
__device__ __forceinline__ void pose_from_tcw(const float* T, double* P) {
    double R[3][3], q[4];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) R[r][c] = (double)T[4 * r + c];
    lm::quat_from_matrix(R, q);
    lm::quat_normalize(q[0], q[1], q[2], q[3]);
    lm::quat_to_matrix(q[0], q[1], q[2], q[3], R);
#pragma unroll
    for (int k = 0; k < 4; k++) P[k] = q[k];
    P[4] = (double)T[3];
    P[5] = (double)T[7];
    P[6] = (double)T[11];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) P[7 + 3 * r + c] = R[r][c];
}

// computeError and chi2 of one edge (types_six_dof_expmap.h; cpp:141-157: the stereo projection
// rounds 1 / z to float and forms bf * invz in float; base_edge.h:59-61); x, y, z: the point
// in the camera frame.  A monocular edge has err[2] = 0.
__device__ __forceinline__ double edge_error(int flags, const float4 r, const double* P, const double (&X)[3],
                                             const Cam& C, double (&err)[3], double& x, double& y, double& z) {
    lm::quat_rotate(P[0], P[1], P[2], P[3], X[0], X[1], X[2], x, y, z);
    x += P[4];
    y += P[5];
    z += P[6];
    const double w = (double)r.w;
    if (flags & kStereo) {
        const float invz = (float)(1.0 / z);
        const float bfz = C.bf_f * invz;
        const double r0 = x * invz * C.fx + C.cx;
        const double r1 = y * invz * C.fy + C.cy;
        const double r2 = r0 - bfz;
        err[0] = (double)r.x - r0;
        err[1] = (double)r.y - r1;
        err[2] = (double)r.z - r2;
    } else {
        err[0] = (double)r.x - ((x / z) * C.fx + C.cx);
        err[1] = (double)r.y - ((y / z) * C.fy + C.cy);
        err[2] = 0.0;
    }
    double chi2 = err[0] * (w * err[0]) + err[1] * (w * err[1]);
    chi2 = chi2 + err[2] * (w * err[2]);
    return chi2;
}

// linearizeOplus of the pose (cpp:126-138, 214-233); row 2 is zero for a monocular edge
__device__ __forceinline__ void pose_jacobian(bool stereo, double x, double y, double z, const Cam& C,
                                              double (&J)[3][6]) {
    const double z_2 = z * z, fx = C.fx, fy = C.fy, bf = C.bf;
    J[0][0] = x * y / z_2 * fx;
    J[0][1] = -(1 + (x * x / z_2)) * fx;
    J[0][2] = y / z * fx;
    J[0][3] = -1. / z * fx;
    J[0][4] = 0;
    J[0][5] = x / z_2 * fx;
    J[1][0] = (1 + y * y / z_2) * fy;
    J[1][1] = -x * y / z_2 * fy;
    J[1][2] = -x / z * fy;
    J[1][3] = 0;
    J[1][4] = -1. / z * fy;
    J[1][5] = y / z_2 * fy;
    if (stereo) {
        J[2][0] = J[0][0] - bf * y / z_2;
        J[2][1] = J[0][1] + bf * x / z_2;
        J[2][2] = J[0][2];
        J[2][3] = J[0][3];
        J[2][4] = 0;
        J[2][5] = J[0][5] - bf / z_2;
    } else {
#pragma unroll
        for (int c = 0; c < 6; c++) J[2][c] = 0.0;
    }
}

// linearizeOplus of the point (cpp:115-124, 202-212); R = P + 7
__device__ __forceinline__ void point_jacobian(bool stereo, const double* R, double x, double y, double z,
                                               const Cam& C, double (&J)[3][3]) {
    const double z_2 = z * z, fx = C.fx, fy = C.fy, bf = C.bf;
    if (stereo) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            J[0][c] = -fx * R[c] / z + fx * x * R[6 + c] / z_2;
            J[1][c] = -fy * R[3 + c] / z + fy * y * R[6 + c] / z_2;
            J[2][c] = J[0][c] - bf * R[6 + c] / z_2;
        }
    } else {  // (-1. / z * tmp) * R, tmp = [fx 0 -x/z*fx; 0 fy -y/z*fy]
        const double s = -1. / z;
        const double t00 = s * fx, t02 = s * (-x / z * fx), t11 = s * fy, t12 = s * (-y / z * fy);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            J[0][c] = t00 * R[c] + t02 * R[6 + c];
            J[1][c] = t11 * R[3 + c] + t12 * R[6 + c];
            J[2][c] = 0.0;
        }
    }
}
}  // namespace ba
}  // namespace orbx
