// orbx_poseopt.hip -- Optimizer::PoseOptimization (motion-only bundle adjustment) for a batch
// of Frames in HBM: one persistent workgroup per frame runs all four rounds, every
// Levenberg-Marquardt iteration and every trial; the host reads nothing back in between.
//
// Reference: src/Optimizer.cc:299-502 and, under Thirdparty/g2o/g2o,
//   core/optimization_algorithm_levenberg.cpp:61-189  solve, computeLambdaInit, computeScale
//   core/sparse_optimizer.cpp:61-114, 354-419         computeActiveErrors, activeRobustChi2, optimize
//   core/base_unary_edge.hpp:43-72                    constructQuadraticForm
//   core/base_edge.h:59-61, 96-102                    chi2, robustInformation (no second-order term)
//   core/robust_kernel_impl.cpp:78-91                 RobustKernelHuber::robustify
//   solvers/linear_solver_dense.h:104-112             LDLT; not positive = failed solve
//   types/types_six_dof_expmap.h:73-76, 153-157, 184-188   oplusImpl, computeError
//   types/types_six_dof_expmap.cpp:266-306, 335-364   Jacobians, cam_project (stereo: float invz)
//   types/se3quat.h:104-110, 217-257, 280-285         operator*, map, exp, normalizeRotation
//   src/Converter.cc                                  toSE3Quat / toCvMat
// DESIGN.md §4.15.
//
// Float inputs are widened to double; everything after is double (the build keeps
// -ffp-contract=off).  The pose is g2o's SE3Quat: a unit quaternion and a translation, with
// Eigen's quaternion-from-matrix, product, vector rotation and toRotationMatrix formulas.
//
// Sums over edges (the 21 upper entries of H, the 6 of b, chi2) have a fixed shape: thread t
// adds its edges t, t + 256, ... in index order, the 64 lanes of a wave are combined by a
// __shfl_xor butterfly (32, 16, ... 1), the four waves are added in wave order from LDS.
// There are no floating-point atomics: a frame's result does not depend on scheduling, on the
// batch or on the compute unit.  After each reduction every thread holds the same sums and
// runs the scalar part (LDLT, exponential map, accept / reject) redundantly, so the control
// flow is uniform and needs no broadcast.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "orbx.h"
#include "orbx_kernels.h"
#include "orbx_lm.h"

namespace orbx {

namespace {

constexpr int kPoThreads = 256;
constexpr int kPoWaves = kPoThreads / 64;
constexpr int kRecWords = 8;  // Xw[3], u, v, u_right, invSigma2, flags
constexpr int kFlagStereo = 1, kFlagOutlier = 2;

using lm::huber;
using lm::Pose;
using lm::pose_map;
using lm::pose_update;
using lm::quat_from_matrix;
using lm::quat_normalize;
using lm::quat_rotate;

struct Cam {
    double fx, fy, cx, cy, bf;
    double delta_mono, delta_stereo;  // the float sqrt(5.991) and sqrt(7.815) of Optimizer.cc:332-334, widened
};

// Eigen's toRotationMatrix
__device__ __forceinline__ void quat_to_matrix(const Pose& P, double (&R)[3][3]) {
    lm::quat_to_matrix(P.qx, P.qy, P.qz, P.qw, R);
}

struct Edge {
    double X, Y, Z, u, v, ur, w;
    int flags;
};

__device__ __forceinline__ Edge load_edge(const float* rec, int stride, int e) {
    Edge E;
    E.X = (double)rec[e];
    E.Y = (double)rec[stride + e];
    E.Z = (double)rec[2 * stride + e];
    E.u = (double)rec[3 * stride + e];
    E.v = (double)rec[4 * stride + e];
    E.ur = (double)rec[5 * stride + e];
    E.w = (double)rec[6 * stride + e];
    E.flags = __float_as_int(rec[7 * stride + e]);
    return E;
}

// computeError and chi2 of one edge at pose P (types_six_dof_expmap.h:153-157, 184-188;
// cpp:290-306: the stereo projection rounds 1 / z to float; base_edge.h:59-61)
__device__ __forceinline__ double edge_error(const Edge& E, const Pose& P, const Cam& C, double (&err)[3],
                                             double& x, double& y, double& z) {
    pose_map(P, E.X, E.Y, E.Z, x, y, z);
    double chi2;
    if (E.flags & kFlagStereo) {
        const double invz = (double)(float)(1.0 / z);
        const double r0 = x * invz * C.fx + C.cx;
        const double r1 = y * invz * C.fy + C.cy;
        const double r2 = r0 - C.bf * invz;
        err[0] = E.u - r0;
        err[1] = E.v - r1;
        err[2] = E.ur - r2;
        chi2 = err[0] * (E.w * err[0]) + err[1] * (E.w * err[1]);
        chi2 = chi2 + err[2] * (E.w * err[2]);
    } else {
        err[0] = E.u - ((x / z) * C.fx + C.cx);
        err[1] = E.v - ((y / z) * C.fy + C.cy);
        err[2] = 0.0;
        chi2 = err[0] * (E.w * err[0]) + err[1] * (E.w * err[1]);
    }
    return chi2;
}

// computeActiveErrors + activeRobustChi2 + buildSystem over the active (level 0) edges:
// s_sum[0..20] the upper triangle of H row by row, s_sum[21..26] = -b, s_sum[27] = chi.
__device__ __forceinline__ void linearize(const float* rec, int stride, int ne, const Pose& P, const Cam& C,
                                          bool robust, double* s_red, double* s_sum) {
    double v[28];
#pragma unroll
    for (int k = 0; k < 28; k++) v[k] = 0.0;
    for (int e = threadIdx.x; e < ne; e += kPoThreads) {
        const Edge E = load_edge(rec, stride, e);
        if (E.flags & kFlagOutlier) continue;
        const bool stereo = E.flags & kFlagStereo;
        double err[3], x, y, z, rho1;
        const double chi2 = edge_error(E, P, C, err, x, y, z);
        v[27] += huber(chi2, stereo ? C.delta_stereo : C.delta_mono, robust, rho1);
        // linearizeOplus, types_six_dof_expmap.cpp:266-288, 335-364
        const double invz = 1.0 / z, invz_2 = invz * invz;
        double J[3][6];
        J[0][0] = x * y * invz_2 * C.fx;
        J[0][1] = -(1.0 + (x * x * invz_2)) * C.fx;
        J[0][2] = y * invz * C.fx;
        J[0][3] = -invz * C.fx;
        J[0][4] = 0.0;
        J[0][5] = x * invz_2 * C.fx;
        J[1][0] = (1.0 + y * y * invz_2) * C.fy;
        J[1][1] = -x * y * invz_2 * C.fy;
        J[1][2] = -x * invz * C.fy;
        J[1][3] = 0.0;
        J[1][4] = -invz * C.fy;
        J[1][5] = y * invz_2 * C.fy;
        // base_unary_edge.hpp:56-63: b -= rho' J^T Omega e, H += J^T (rho' Omega) J
        const double w = rho1 * E.w;
        const double we0 = w * err[0], we1 = w * err[1];
        if (stereo) {
            J[2][0] = J[0][0] - C.bf * y * invz_2;
            J[2][1] = J[0][1] + C.bf * x * invz_2;
            J[2][2] = J[0][2];
            J[2][3] = J[0][3];
            J[2][4] = 0.0;
            J[2][5] = J[0][5] - C.bf * invz_2;
            const double we2 = w * err[2];
            int k = 0;
#pragma unroll
            for (int r = 0; r < 6; r++) {
#pragma unroll
                for (int c = r; c < 6; c++, k++)
                    v[k] += J[0][r] * w * J[0][c] + J[1][r] * w * J[1][c] + J[2][r] * w * J[2][c];
                v[21 + r] += J[0][r] * we0 + J[1][r] * we1 + J[2][r] * we2;
            }
        } else {
            int k = 0;
#pragma unroll
            for (int r = 0; r < 6; r++) {
#pragma unroll
                for (int c = r; c < 6; c++, k++) v[k] += J[0][r] * w * J[0][c] + J[1][r] * w * J[1][c];
                v[21 + r] += J[0][r] * we0 + J[1][r] * we1;
            }
        }
    }
    lm::block_sum_lds<28, kPoWaves>(v, s_red, s_sum);
}

// computeActiveErrors + activeRobustChi2 at a trial pose
__device__ __forceinline__ double robust_chi(const float* rec, int stride, int ne, const Pose& P, const Cam& C,
                                             bool robust, double* s_red) {
    double v[1] = {0.0};
    for (int e = threadIdx.x; e < ne; e += kPoThreads) {
        const Edge E = load_edge(rec, stride, e);
        if (E.flags & kFlagOutlier) continue;
        double err[3], x, y, z, rho1;
        const double chi2 = edge_error(E, P, C, err, x, y, z);
        v[0] += huber(chi2, (E.flags & kFlagStereo) ? C.delta_stereo : C.delta_mono, robust, rho1);
    }
    lm::block_sum<1, kPoWaves>(v, s_red);
    return v[0];
}

// The four rounds (Optimizer.cc:440-493) over the frame's records at rec (LDS or the
// workspace).  Returns nBad; P is left at the recovered estimate.
__device__ __forceinline__ int optimize_frame(float* rec, int stride, int ne, const Pose& P0, const Cam& C, Pose& P,
                                              int32_t* trace, double* s_red, double* s_sum, int* s_cnt) {
    int nbad_edges = 0;
    for (int round = 0; round < 4; round++) {
        const bool robust = round < 3;  // cc:467-468: the kernel is dropped after round 2's classification
        Pose cur = P0, errp = P0;       // cc:441
        int its = 0, trials = 0;
        if (ne - nbad_edges > 0) {      // no active edge: no active vertex, optimize() returns at once
            double lam = 0.0, ni = 2.0, x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            int nbad = 0;
            for (int it = 0; it < 10; it++) {
                // the next linearize writes s_sum only after a barrier that follows this iteration's last read
                const double* h = s_sum;
                linearize(rec, stride, ne, cur, C, robust, s_red, s_sum);
                errp = cur;
                double b[6];
#pragma unroll
                for (int j = 0; j < 6; j++) b[j] = -h[21 + j];
                double chi = h[27];
                const double ini_chi = chi;
                if (it == 0) {  // computeLambdaInit: tau = 1e-5
                    double md = 0.0;
                    md = fmax(fabs(h[0]), md);
                    md = fmax(fabs(h[6]), md);
                    md = fmax(fabs(h[11]), md);
                    md = fmax(fabs(h[15]), md);
                    md = fmax(fabs(h[18]), md);
                    md = fmax(fabs(h[20]), md);
                    lam = 1e-5 * md;
                    ni = 2.0;
                    nbad = 0;
                }
                int qmax = 0;
                double rho = 0.0;
                do {
                    const bool ok = lm::ldlt_solve<6>(h, lam, b, x);
                    const Pose trial = pose_update(x, cur);
                    double temp = robust_chi(rec, stride, ne, trial, C, robust, s_red);
                    errp = trial;
                    if (!ok) temp = DBL_MAX;
                    rho = chi - temp;
                    double scale = 0.0;
#pragma unroll
                    for (int j = 0; j < 6; j++) scale += x[j] * (lam * x[j] + b[j]);
                    scale += 1e-3;
                    rho = rho / scale;
                    if (rho > 0 && isfinite(temp)) {
                        const double t = 2.0 * rho - 1.0;
                        double alpha = 1.0 - t * t * t;
                        alpha = fmin(alpha, 2.0 / 3.0);
                        lam *= fmax(1.0 / 3.0, alpha);
                        ni = 2.0;
                        chi = temp;
                        cur = trial;
                    } else {
                        lam *= ni;
                        ni *= 2.0;
                    }
                    qmax++;
                } while (rho < 0 && qmax < 10);
                trials += qmax;
                its++;
                if (qmax == 10 || rho == 0) break;
                if ((ini_chi - chi) * 1e3 < ini_chi)
                    nbad++;
                else
                    nbad = 0;
                if (nbad >= 3) break;
            }
        }
        if (threadIdx.x == 0 && trace) {
            trace[2 * round] = its;
            trace[2 * round + 1] = trials;
        }
        // cc:449-489: an active edge keeps the chi2 of the last computeActiveErrors (pose errp),
        // an outlier's is computed at the round's estimate
        int bad = 0;
        for (int e = threadIdx.x; e < ne; e += kPoThreads) {
            const Edge E = load_edge(rec, stride, e);
            double err[3], x, y, z;
            const double chi2 = edge_error(E, (E.flags & kFlagOutlier) ? cur : errp, C, err, x, y, z);
            const bool out = (float)chi2 > ((E.flags & kFlagStereo) ? 7.815f : 5.991f);
            rec[7 * stride + e] = __int_as_float((E.flags & kFlagStereo) | (out ? kFlagOutlier : 0));
            bad += out;
        }
        nbad_edges = lm::block_sum_int<kPoWaves>(bad, s_cnt);
        P = cur;
        if (ne < 10) break;  // cc:491
    }
    return nbad_edges;
}

__global__ __launch_bounds__(kPoThreads) void k_pose_opt(PoseOptArgs A) {
    extern __shared__ __attribute__((aligned(16))) double s_mem[];
    double* s_red = s_mem;                                   // [4][28]
    double* s_sum = s_red + kPoWaves * 28;                   // [28]
    int* s_cnt = (int*)(s_sum + 28);                         // [4] (+ 4 spare)
    float* s_rec = (float*)(s_cnt + 8);                      // [8][kPoseOptLdsEdges]
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cap = A.cap;
    int n = A.n[b];
    n = n < 0 ? 0 : (n > cap ? cap : n);
    const size_t row = (size_t)b * cap;
    float* g_rec = A.rec + row * kRecWords;
    int32_t* eidx = A.eidx + row;
    int32_t* frame_mp = A.frame_mp + row;
    uint8_t* outlier = A.outlier + row;
    const orbx_keypoint* kps = A.kps + row;
    const float* ur = A.u_right ? A.u_right + row : nullptr;
    int32_t* trace = A.trace ? A.trace + (size_t)b * 8 : nullptr;
    if (trace)
        for (int k = tid; k < 8; k += kPoThreads) trace[k] = 0;

    // The frame's edges in keypoint order (cc:340-425), compacted into SoA records
    int ne = 0;
    for (int c0 = 0; c0 < n; c0 += kPoThreads) {
        const int i = c0 + tid;
        int id = -1;
        if (i < n) id = frame_mp[i];
        const bool has = id >= 0 && id < A.n_mp;
        const unsigned long long m = __ballot(has);
        if (lane == 0) s_cnt[wave] = __popcll(m);
        __syncthreads();
        int off = ne, total = 0;
#pragma unroll
        for (int w = 0; w < kPoWaves; w++) {
            if (w < wave) off += s_cnt[w];
            total += s_cnt[w];
        }
        if (has) {
            const int e = off + __popcll(m & ((1ull << lane) - 1ull));
            const orbx_keypoint kp = kps[i];
            const float r = ur ? ur[i] : -1.0f;
            const bool stereo = !(r < 0);  // cc:346
            int oct = kp.octave;
            oct = oct < 0 ? 0 : (oct >= A.nlevels ? A.nlevels - 1 : oct);
            g_rec[e] = A.pos[(size_t)id * 3];
            g_rec[cap + e] = A.pos[(size_t)id * 3 + 1];
            g_rec[2 * cap + e] = A.pos[(size_t)id * 3 + 2];
            g_rec[3 * cap + e] = kp.x;
            g_rec[4 * cap + e] = kp.y;
            g_rec[5 * cap + e] = stereo ? r : 0.0f;
            g_rec[6 * cap + e] = A.inv_sigma2[oct];
            g_rec[7 * cap + e] = __int_as_float(stereo ? kFlagStereo : 0);
            eidx[e] = i;
            outlier[i] = 0;  // cc:349, 388
        }
        ne += total;
        __syncthreads();
    }

    Cam C;
    C.fx = (double)A.fx;
    C.fy = (double)A.fy;
    C.cx = (double)A.cx;
    C.cy = (double)A.cy;
    C.bf = (double)A.bf;
    C.delta_mono = (double)A.delta_mono;
    C.delta_stereo = (double)A.delta_stereo;
    const float* Tin = A.Tcw + (size_t)b * 12;
    float* Tout = A.Tcw_out + (size_t)b * 12;
    int nbad = 0;
    const bool lds = ne <= kPoseOptLdsEdges;
    if (ne < 3) {  // cc:428: return 0, the pose untouched
        for (int k = tid; k < 12; k += kPoThreads) Tout[k] = Tin[k];
    } else {
        // Converter::toSE3Quat
        double R[3][3], q[4];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) R[r][c] = (double)Tin[4 * r + c];
        quat_from_matrix(R, q);
        quat_normalize(q[0], q[1], q[2], q[3]);
        Pose P0, P;
        P0.qx = q[0];
        P0.qy = q[1];
        P0.qz = q[2];
        P0.qw = q[3];
        P0.tx = (double)Tin[3];
        P0.ty = (double)Tin[7];
        P0.tz = (double)Tin[11];
        P = P0;
        if (lds) {
            for (int k = 0; k < kRecWords; k++)
                for (int e = tid; e < ne; e += kPoThreads) s_rec[k * kPoseOptLdsEdges + e] = g_rec[k * cap + e];
            __syncthreads();
            nbad = optimize_frame(s_rec, kPoseOptLdsEdges, ne, P0, C, P, trace, s_red, s_sum, s_cnt);
        } else {
            nbad = optimize_frame(g_rec, cap, ne, P0, C, P, trace, s_red, s_sum, s_cnt);
        }
        // Converter::toCvMat(SE3Quat)
        if (tid == 0) {
            quat_to_matrix(P, R);
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) Tout[4 * r + c] = (float)R[r][c];
            Tout[3] = (float)P.tx;
            Tout[7] = (float)P.ty;
            Tout[11] = (float)P.tz;
        }
    }
    if (tid == 0) {
        A.ninit[b] = ne;
        A.ninliers[b] = ne < 3 ? 0 : ne - nbad;
    }
    // mvbOutlier, then what the callers do next (Tracking.cc:1004-1017)
    const float* flags = (ne >= 3 && lds) ? s_rec + 7 * kPoseOptLdsEdges : g_rec + 7 * (size_t)cap;
    int nmap = 0;
    for (int e = tid; e < ne; e += kPoThreads) {
        const bool out = ne >= 3 && (__float_as_int(flags[e]) & kFlagOutlier);
        const int i = eidx[e];
        if (out) {
            if (A.discard_outliers) {
                frame_mp[i] = -1;
                outlier[i] = 0;
            } else {
                outlier[i] = 1;
            }
        } else if (A.nmatches_map) {
            nmap += !A.mp_obs || A.mp_obs[frame_mp[i]] > 0;
        }
    }
    if (A.nmatches_map) {
        nmap = lm::block_sum_int<kPoWaves>(nmap, s_cnt);
        if (tid == 0) A.nmatches_map[b] = nmap;
    }
}

}  // namespace

size_t pose_opt_workspace_bytes(int batch, int cap) {
    return (size_t)batch * cap * (kRecWords + 1) * 4;
}

hipError_t launch_pose_opt(PoseOptArgs A, int batch, char* workspace, hipStream_t stream) {
    if (batch <= 0) return hipSuccess;
    A.rec = (float*)workspace;
    A.eidx = (int32_t*)(workspace + (size_t)batch * A.cap * kRecWords * 4);
    const size_t lds = (kPoWaves + 1) * 28 * 8 + 8 * 4 + (size_t)kRecWords * kPoseOptLdsEdges * 4;
    k_pose_opt<<<batch, kPoThreads, lds, stream>>>(A);
    return hipGetLastError();
}

}  // namespace orbx
