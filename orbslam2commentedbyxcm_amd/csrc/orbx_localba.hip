// orbx_localba.hip -- Optimizer::LocalBundleAdjustment for a batch of local maps in HBM: one
// persistent workgroup per problem runs optimize(5), the chi2 / depth test, optimize(10) on the
// edges that passed and the final test; the host reads nothing back in between.
//
// Reference: src/Optimizer.cc:586-853 and, under Thirdparty/g2o/g2o,
//   core/optimization_algorithm_levenberg.cpp:61-189  solve, computeLambdaInit, computeScale
//   core/block_solver.hpp:354-486, 502-560            the Schur complement, buildSystem
//   core/base_binary_edge.hpp:55-120                  constructQuadraticForm
//   core/robust_kernel_impl.cpp:78-91                 RobustKernelHuber::robustify
//   types/types_six_dof_expmap.cpp:103-157, 188-234   Jacobians, cam_project (stereo: float
//                                                     invz and the float product bf * invz)
//   types/types_six_dof_expmap.h                      computeError, isDepthPositive, oplusImpl
//   types/se3quat.h                                   operator*, map, exp, normalizeRotation
//   src/Converter.cc                                  toSE3Quat / toCvMat
// DESIGN.md §4.20.  The stop flag (pbStopFlag) is not supported: bDoMore is always true.
//
// Float inputs are widened to double; everything after is double (the build keeps
// -ffp-contract=off), except the two float intermediates of the stereo projection.
//
// No workgroup waits on another and no sum uses a floating-point atomic.  Every sum has one
// owner and a fixed shape:
//   a point's Hll, b_l and the blocks W = A^T (rho' Omega) B of its edges: the point's thread,
//     in edge order;
//   a free keyframe's Hpp block and b_p, and its part of B Dinv b_l: one wave; lane l adds the
//     keyframe's edges l, l + 64, ... of its edge list (edge order), the lanes are combined by
//     the xor butterfly of orbx_lm.h;
//   an entry of S: the wave that owns its block row (row mod 4), which walks the points in
//     order; within a point an entry belongs to one lane;
//   chi2 and computeScale: thread t adds its points (keyframes) t, t + 256, ..., then block_sum.
// The reduced system is factored by lm::ldlt_solve_block in natural order.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "orbx.h"
#include "orbx_ba_edge.h"
#include "orbx_kernels.h"
#include "orbx_layout.h"
#include "orbx_lm.h"

namespace orbx {

namespace {

constexpr int kLbThreads = 256;
constexpr int kLbWaves = kLbThreads / 64;
constexpr int kMaxFree = ORBX_LOCAL_BA_MAX_FREE_KF;
constexpr int kPtSys = 24;  // Hll (6), bl (3), Dinv (9), Dinv bl (3), xl (3)
using namespace ba;         // Cam, the pose record, the edges and their Jacobians (orbx_ba_edge.h)

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ double block_max(double v, double* s_red) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = s_red[0];
#pragma unroll
    for (int w = 1; w < kLbWaves; w++) s = fmax(s, s_red[w]);
    __syncthreads();
    return s;
}

struct Prob {
    int k0, K, p0, P, oA, oB;
};

__device__ __forceinline__ void point_range(const LocalBaArgs& A, const Prob& Q, int j, int& o0, int& o1) {
    o0 = clampi(A.obs_off[Q.p0 + j], Q.oA, Q.oB);
    o1 = clampi(A.obs_off[Q.p0 + j + 1], o0, Q.oB);
}

// computeActiveErrors + activeRobustChi2 at the estimates of `slot`; every active edge's chi2
// is left in A.chi2
__device__ __forceinline__ double active_chi(const LocalBaArgs& A, const Prob& Q, const Cam& C, int slot,
                                             bool robust, double* s_red) {
    double v[1] = {0.0};
    for (int j = threadIdx.x; j < Q.P; j += kLbThreads) {
        if (!A.pt_active[Q.p0 + j]) continue;
        int o0, o1;
        point_range(A, Q, j, o0, o1);
        const double* pp = A.pt + ((size_t)(Q.p0 + j) * 2 + slot) * 3;
        const double X[3] = {pp[0], pp[1], pp[2]};
        for (int e = o0; e < o1; e++) {
            const int fl = A.rec_flags[e];
            if ((fl & (kValid | kLevel1)) != kValid || A.rec_pt[e] != j) continue;
            const double* Pk = A.pose + ((size_t)(Q.k0 + A.rec_kf[e]) * 2 + slot) * kPoseWords;
            double err[3], x, y, z, rho1;
            const double chi2 = edge_error(fl, ((const float4*)A.rec)[e], Pk, X, C, err, x, y, z);
            A.chi2[e] = chi2;
            v[0] += lm::huber(chi2, (fl & kStereo) ? C.delta_stereo : C.delta_mono, robust, rho1);
        }
    }
    lm::block_sum<1, kLbWaves>(v, s_red);
    return v[0];
}

__global__ __launch_bounds__(kLbThreads) void k_local_ba(LocalBaArgs A) {
    __shared__ double s_red[kLbWaves * 28];
    __shared__ double s_hpp[kMaxFree * 21];
    __shared__ double s_bp[kMaxFree * 6], s_bs[kMaxFree * 6], s_xp[kMaxFree * 6];
    __shared__ int s_fk[kMaxFree], s_cand[kMaxFree], s_ccnt[kMaxFree], s_eoff[kMaxFree + 1];
    __shared__ int s_cnt[8], s_misc[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    Prob Q;
    Q.k0 = clampi(A.kf_off[b], 0, A.n_kf);
    Q.K = clampi(A.kf_off[b + 1], Q.k0, A.n_kf) - Q.k0;
    Q.p0 = clampi(A.pt_off[b], 0, A.n_pt);
    Q.P = clampi(A.pt_off[b + 1], Q.p0, A.n_pt) - Q.p0;
    Q.oA = clampi(A.obs_off[Q.p0], 0, A.n_obs);
    Q.oB = clampi(A.obs_off[Q.p0 + Q.P], Q.oA, A.n_obs);
    const int k0 = Q.k0, K = Q.K, p0 = Q.p0, P = Q.P, oA = Q.oA, oB = Q.oB;
    int32_t* trace = A.trace ? A.trace + (size_t)b * 4 : nullptr;

    // outputs that hold whatever happens: nothing to erase, the trace at zero
    for (int e = oA + tid; e < oB; e += kLbThreads) {
        A.erase[e] = 0;
        if (A.level1) A.level1[e] = 0;
    }
    if (trace && tid < 4) trace[tid] = 0;
    int nfree = 0;
    for (int k = tid; k < K; k += kLbThreads) nfree += A.kf_fixed[k0 + k] ? 0 : 1;
    nfree = lm::block_sum_int<kLbWaves>(nfree, s_cnt);
    const int cap_free = A.max_free < kMaxFree ? A.max_free : kMaxFree;
    if (nfree == 0 || nfree > cap_free) {  // the inputs come back
        for (int i = tid; i < K * 12; i += kLbThreads) A.kf_Tcw_out[(size_t)k0 * 12 + i] = A.kf_Tcw[(size_t)k0 * 12 + i];
        for (int i = tid; i < P * 3; i += kLbThreads) A.pt_pos_out[(size_t)p0 * 3 + i] = A.pt_pos[(size_t)p0 * 3 + i];
        if (tid == 0) {
            A.n_erase[b] = 0;
            A.status[b] = nfree == 0 ? ORBX_LOCAL_BA_STATUS_NO_FREE_KF : ORBX_LOCAL_BA_STATUS_CAPACITY;
        }
        return;
    }

    Cam C;
    C.fx = (double)A.fx;
    C.fy = (double)A.fy;
    C.cx = (double)A.cx;
    C.cy = (double)A.cy;
    C.bf = (double)A.bf;
    C.bf_f = A.bf;
    C.delta_mono = (double)A.delta_mono;
    C.delta_stereo = (double)A.delta_stereo;

    // ---- vertices and edge records (cc:601-735) ----
    for (int k = tid; k < K; k += kLbThreads) {
        double Pk[kPoseWords];
        pose_from_tcw(A.kf_Tcw + (size_t)(k0 + k) * 12, Pk);
        double* d = A.pose + (size_t)(k0 + k) * 2 * kPoseWords;
#pragma unroll
        for (int i = 0; i < kPoseWords; i++) d[i] = d[kPoseWords + i] = Pk[i];
    }
    for (int i = tid; i < P * 3; i += kLbThreads) {
        const int j = i / 3, c = i - 3 * j;
        const double v = (double)A.pt_pos[(size_t)p0 * 3 + i];
        A.pt[((size_t)(p0 + j) * 2) * 3 + c] = v;
        A.pt[((size_t)(p0 + j) * 2 + 1) * 3 + c] = v;
    }
    for (int e = oA + tid; e < oB; e += kLbThreads) {
        A.rec_kf[e] = -1;
        A.rec_pt[e] = -1;
        A.rec_flags[e] = 0;
        A.rec_free[e] = -1;
        A.chi2[e] = 0.0;
    }
    __syncthreads();
    int nbadidx = 0;
    for (int j = tid; j < P; j += kLbThreads) {
        int o0, o1;
        point_range(A, Q, j, o0, o1);
        for (int e = o0; e < o1; e++) {
            const int kf = A.obs_kf[e], kp = A.obs_kp[e];
            bool ok = kf >= 0 && kf < K && kp >= 0 && kp < A.cap;
            int slot = -1;
            if (ok) {
                slot = A.kf_slot[k0 + kf];
                ok = slot >= 0 && slot < A.n_slots;
            }
            for (int e2 = o0; ok && e2 < e; e2++) ok = A.obs_kf[e2] != kf;  // one observation per keyframe
            if (!ok) {
                nbadidx++;
                continue;
            }
            const size_t at = (size_t)slot * A.cap + kp;
            const orbx_keypoint kpt = A.kps[at];
            const float ur = A.u_right ? A.u_right[at] : -1.0f;
            const bool stereo = !(ur < 0);  // cc:679
            int oct = kpt.octave;
            oct = oct < 0 ? 0 : (oct >= A.nlevels ? A.nlevels - 1 : oct);
            ((float4*)A.rec)[e] = make_float4(kpt.x, kpt.y, stereo ? ur : 0.0f, A.inv_sigma2[oct]);
            A.rec_kf[e] = kf;
            A.rec_pt[e] = j;
            A.rec_flags[e] = kValid | (stereo ? kStereo : 0);
        }
    }
    nbadidx = lm::block_sum_int<kLbWaves>(nbadidx, s_cnt);
    // the keyframes that may move, in table order
    if (tid == 0) {
        int c = 0;
        for (int k = 0; k < K; k++)
            if (!A.kf_fixed[k0 + k]) s_cand[c++] = k;
    }
    __syncthreads();

    double* S = A.S + (size_t)b * (6 * (size_t)A.max_free) * (6 * (size_t)A.max_free);
    int nerase = 0;
    for (int phase = 0; phase < 2; phase++) {
        const bool robust = phase == 0;  // cc:768, 781
        // ---- initializeOptimization(0): the active edges, vertices and the order of S ----
        for (int k = tid; k < K; k += kLbThreads) A.kf_free[k0 + k] = -1;
        for (int i = tid; i < kMaxFree * 6; i += kLbThreads) s_xp[i] = 0.0;  // the solver's x starts at zero
        for (int i = tid; i < P * 3; i += kLbThreads) A.pt_sys[(size_t)(p0 + i / 3) * kPtSys + 21 + i % 3] = 0.0;
        for (int c = wave; c < nfree; c += kLbWaves) {
            const int k = s_cand[c];
            int n = 0;
            for (int e = oA + lane; e < oB; e += 64)
                n += A.rec_kf[e] == k && (A.rec_flags[e] & (kValid | kLevel1)) == kValid;
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) n += __shfl_xor(n, m, 64);
            if (lane == 0) s_ccnt[c] = n;
        }
        __syncthreads();
        if (tid == 0) {
            int f = 0, run = 0;
            for (int c = 0; c < nfree; c++) {
                if (s_ccnt[c] <= 0) continue;
                s_fk[f] = s_cand[c];
                s_eoff[f] = run;
                run += s_ccnt[c];
                A.kf_free[k0 + s_cand[c]] = f++;
            }
            s_eoff[f] = run;
            s_misc[0] = f;
        }
        __syncthreads();
        const int F = s_misc[0], n = 6 * F;
        for (int f = wave; f < F; f += kLbWaves) {
            const int k = s_fk[f];
            int pos = oA + s_eoff[f];
            for (int base = oA; base < oB; base += 64) {
                const int e = base + lane;
                const bool hit = e < oB && A.rec_kf[e] == k && (A.rec_flags[e] & (kValid | kLevel1)) == kValid;
                const unsigned long long m = __ballot(hit);
                if (hit) A.kf_elist[pos + __popcll(m & ((1ull << lane) - 1ull))] = e;
                pos += __popcll(m);
            }
        }
        int nact = 0;
        for (int e = oA + tid; e < oB; e += kLbThreads) {
            const bool act = (A.rec_flags[e] & (kValid | kLevel1)) == kValid;
            A.rec_free[e] = act ? A.kf_free[k0 + A.rec_kf[e]] : -1;
            nact += act;
        }
        for (int j = tid; j < P; j += kLbThreads) {
            int o0, o1, any = 0;
            point_range(A, Q, j, o0, o1);
            for (int e = o0; e < o1; e++) any |= (A.rec_flags[e] & (kValid | kLevel1)) == kValid && A.rec_pt[e] == j;
            A.pt_active[p0 + j] = any;
        }
        nact = lm::block_sum_int<kLbWaves>(nact, s_cnt);

        // ---- optimize(5) / optimize(10) ----
        int its = 0, trials = 0;
        if (nact > 0 && F > 0) {
            const int max_it = phase == 0 ? 5 : 10;
            double lam = 0.0, ni = 2.0;
            int nbad = 0;
            for (int it = 0; it < max_it; it++) {
                // computeActiveErrors, activeRobustChi2, buildSystem: the points' side
                double v[1] = {0.0};
                double md = 0.0;
                for (int j = tid; j < P; j += kLbThreads) {
                    if (!A.pt_active[p0 + j]) continue;
                    int o0, o1;
                    point_range(A, Q, j, o0, o1);
                    const double* pp = A.pt + ((size_t)(p0 + j) * 2) * 3;
                    const double X[3] = {pp[0], pp[1], pp[2]};
                    double h[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, bl[3] = {0.0, 0.0, 0.0};
                    for (int e = o0; e < o1; e++) {
                        const int fl = A.rec_flags[e];
                        if ((fl & (kValid | kLevel1)) != kValid || A.rec_pt[e] != j) continue;
                        const bool stereo = fl & kStereo;
                        const float4 r = ((const float4*)A.rec)[e];
                        const double* Pk = A.pose + ((size_t)(k0 + A.rec_kf[e]) * 2) * kPoseWords;
                        double err[3], x, y, z, rho1;
                        const double chi2 = edge_error(fl, r, Pk, X, C, err, x, y, z);
                        A.chi2[e] = chi2;
                        v[0] += lm::huber(chi2, stereo ? C.delta_stereo : C.delta_mono, robust, rho1);
                        double Ja[3][3];
                        point_jacobian(stereo, Pk + 7, x, y, z, C, Ja);
                        // base_binary_edge.hpp:73-113
                        const double w0 = (double)r.w, w = rho1 * w0;
                        double wr[3];
#pragma unroll
                        for (int i = 0; i < 3; i++) wr[i] = -(w0 * err[i]) * rho1;
                        int q = 0;
#pragma unroll
                        for (int a = 0; a < 3; a++) {
#pragma unroll
                            for (int c = a; c < 3; c++, q++)
                                h[q] += Ja[0][a] * w * Ja[0][c] + Ja[1][a] * w * Ja[1][c] + Ja[2][a] * w * Ja[2][c];
                            bl[a] += Ja[0][a] * wr[0] + Ja[1][a] * wr[1] + Ja[2][a] * wr[2];
                        }
                        if (A.rec_free[e] >= 0) {
                            double Jb[3][6];
                            pose_jacobian(stereo, x, y, z, C, Jb);
                            double* W = A.W + (size_t)e * 18;
#pragma unroll
                            for (int a = 0; a < 3; a++)
#pragma unroll
                                for (int c = 0; c < 6; c++)
                                    W[a * 6 + c] = Ja[0][a] * w * Jb[0][c] + Ja[1][a] * w * Jb[1][c] + Ja[2][a] * w * Jb[2][c];
                        }
                    }
                    double* ps = A.pt_sys + (size_t)(p0 + j) * kPtSys;
#pragma unroll
                    for (int i = 0; i < 6; i++) ps[i] = h[i];
#pragma unroll
                    for (int i = 0; i < 3; i++) ps[6 + i] = bl[i];
                    md = fmax(fmax(fabs(h[0]), fabs(h[3])), fmax(fabs(h[5]), md));
                }
                lm::block_sum<1, kLbWaves>(v, s_red);
                double chi = v[0];
                const double ini_chi = chi;
                // the keyframes' side: Hpp and b_p of every free keyframe, by its wave
                for (int f = wave; f < F; f += kLbWaves) {
                    const double* Pk = A.pose + ((size_t)(k0 + s_fk[f]) * 2) * kPoseWords;
                    double acc[27];
#pragma unroll
                    for (int i = 0; i < 27; i++) acc[i] = 0.0;
                    for (int i = s_eoff[f] + lane; i < s_eoff[f + 1]; i += 64) {
                        const int e = A.kf_elist[oA + i];
                        const int fl = A.rec_flags[e];
                        const bool stereo = fl & kStereo;
                        const float4 r = ((const float4*)A.rec)[e];
                        const double* pp = A.pt + ((size_t)(p0 + A.rec_pt[e]) * 2) * 3;
                        const double X[3] = {pp[0], pp[1], pp[2]};
                        double err[3], x, y, z, rho1;
                        const double chi2 = edge_error(fl, r, Pk, X, C, err, x, y, z);
                        (void)lm::huber(chi2, stereo ? C.delta_stereo : C.delta_mono, robust, rho1);
                        double Jb[3][6];
                        pose_jacobian(stereo, x, y, z, C, Jb);
                        const double w0 = (double)r.w, w = rho1 * w0;
                        double wr[3];
#pragma unroll
                        for (int q = 0; q < 3; q++) wr[q] = -(w0 * err[q]) * rho1;
                        int q = 0;
#pragma unroll
                        for (int a = 0; a < 6; a++) {
#pragma unroll
                            for (int c = a; c < 6; c++, q++)
                                acc[q] += Jb[0][a] * w * Jb[0][c] + Jb[1][a] * w * Jb[1][c] + Jb[2][a] * w * Jb[2][c];
                            acc[21 + a] += Jb[0][a] * wr[0] + Jb[1][a] * wr[1] + Jb[2][a] * wr[2];
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 27; i++)
#pragma unroll
                        for (int m = 32; m > 0; m >>= 1) acc[i] += __shfl_xor(acc[i], m, 64);
                    if (lane == 0) {
#pragma unroll
                        for (int i = 0; i < 21; i++) s_hpp[f * 21 + i] = acc[i];
#pragma unroll
                        for (int i = 0; i < 6; i++) s_bp[f * 6 + i] = acc[21 + i];
                    }
                }
                __syncthreads();
                if (it == 0) {  // computeLambdaInit: tau = 1e-5 over every active free vertex
                    for (int i = tid; i < n; i += kLbThreads) {
                        const int f = i / 6, r = i - 6 * f;
                        md = fmax(fabs(s_hpp[f * 21 + r * 6 - (r * (r - 1)) / 2]), md);
                    }
                    md = block_max(md, s_red);
                    lam = 1e-5 * md;
                    ni = 2.0;
                    nbad = 0;
                }
                int qmax = 0;
                double rho = 0.0;
                do {
                    // setLambda, the landmark inverses (block_solver.hpp:381-395; Eigen's 3x3 inverse by cofactors)
                    for (int j = tid; j < P; j += kLbThreads) {
                        if (!A.pt_active[p0 + j]) continue;
                        double* ps = A.pt_sys + (size_t)(p0 + j) * kPtSys;
                        const double m00 = ps[0] + lam, m01 = ps[1], m02 = ps[2], m11 = ps[3] + lam, m12 = ps[4],
                                     m22 = ps[5] + lam;
                        const double c00 = m11 * m22 - m12 * m12, c10 = m12 * m02 - m22 * m01, c20 = m01 * m12 - m02 * m11;
                        const double det = (c00 * m00 + c10 * m01) + c20 * m02;
                        const double invdet = 1.0 / det;
                        double D[9];
                        D[0] = c00 * invdet;
                        D[1] = c10 * invdet;
                        D[2] = c20 * invdet;
                        D[3] = (m12 * m02 - m01 * m22) * invdet;
                        D[4] = (m22 * m00 - m02 * m02) * invdet;
                        D[5] = (m02 * m01 - m00 * m12) * invdet;
                        D[6] = (m01 * m12 - m11 * m02) * invdet;
                        D[7] = (m02 * m01 - m12 * m00) * invdet;
                        D[8] = (m00 * m11 - m01 * m01) * invdet;
#pragma unroll
                        for (int i = 0; i < 9; i++) ps[9 + i] = D[i];
#pragma unroll
                        for (int a = 0; a < 3; a++) ps[18 + a] = D[3 * a] * ps[6] + D[3 * a + 1] * ps[7] + D[3 * a + 2] * ps[8];
                    }
                    // S = Hpp + lambda I (upper triangle)
                    for (int i = tid; i < n * n; i += kLbThreads) {
                        const int r = i / n, c = i - r * n, fr = r / 6, fc = c / 6, a = r - 6 * fr, d = c - 6 * fc;
                        double val = 0.0;
                        if (fr == fc && a <= d) val = s_hpp[fr * 21 + a * 6 - (a * (a - 1)) / 2 + (d - a)] + (a == d ? lam : 0.0);
                        S[i] = val;
                    }
                    __syncthreads();
                    // S -= B Dinv B^T (block_solver.hpp:400-431), block rows by wave, points in order
                    for (int j = 0; j < P; j++) {
                        if (!A.pt_active[p0 + j]) continue;
                        int o0, o1;
                        point_range(A, Q, j, o0, o1);
                        const double* D = A.pt_sys + (size_t)(p0 + j) * kPtSys + 9;
                        const int items = (o1 - o0) * 36;
                        for (int e1 = o0; e1 < o1; e1++) {
                            const int f1 = A.rec_free[e1];
                            if (f1 < 0 || (f1 & (kLbWaves - 1)) != wave || A.rec_pt[e1] != j) continue;
                            const double* W1 = A.W + (size_t)e1 * 18;
                            for (int i = lane; i < items; i += 64) {
                                const int e2 = o0 + i / 36, ent = i % 36, r = ent / 6, c = ent - 6 * r;
                                const int f2 = A.rec_free[e2];
                                if (f2 < f1 || A.rec_pt[e2] != j) continue;
                                if (f2 == f1 && (e2 != e1 || r > c)) continue;
                                const double* W2 = A.W + (size_t)e2 * 18;
                                const double w0 = W1[r], w1 = W1[6 + r], w2 = W1[12 + r];
                                const double bd0 = w0 * D[0] + w1 * D[3] + w2 * D[6];
                                const double bd1 = w0 * D[1] + w1 * D[4] + w2 * D[7];
                                const double bd2 = w0 * D[2] + w1 * D[5] + w2 * D[8];
                                double* s = S + (size_t)(6 * f1 + r) * n + 6 * f2 + c;
                                *s = *s - (bd0 * W2[c] + bd1 * W2[6 + c] + bd2 * W2[12 + c]);
                            }
                        }
                        // the next point's updates of an entry follow this point's, whichever lane makes them
                        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    }
                    // b_s = b_p - B Dinv b_l (block_solver.hpp:413, 436-439)
                    for (int f = wave; f < F; f += kLbWaves) {
                        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                        for (int i = s_eoff[f] + lane; i < s_eoff[f + 1]; i += 64) {
                            const int e = A.kf_elist[oA + i];
                            const double* W = A.W + (size_t)e * 18;
                            const double* db = A.pt_sys + (size_t)(p0 + A.rec_pt[e]) * kPtSys + 18;
#pragma unroll
                            for (int r = 0; r < 6; r++) acc[r] += W[r] * db[0] + W[6 + r] * db[1] + W[12 + r] * db[2];
                        }
#pragma unroll
                        for (int r = 0; r < 6; r++)
#pragma unroll
                            for (int m = 32; m > 0; m >>= 1) acc[r] += __shfl_xor(acc[r], m, 64);
                        if (lane == 0) {
#pragma unroll
                            for (int r = 0; r < 6; r++) s_bs[f * 6 + r] = s_bp[f * 6 + r] - acc[r];
                        }
                    }
                    __syncthreads();
                    const bool ok = lm::ldlt_solve_block<kLbThreads>(S, n, s_bs);
                    __syncthreads();
                    if (ok) {  // a failed solve leaves x as it was
                        for (int i = tid; i < n; i += kLbThreads) s_xp[i] = s_bs[i];
                        __syncthreads();
                        // x_l = Dinv (b_l - B^T x_p) (block_solver.hpp:468-481)
                        for (int j = tid; j < P; j += kLbThreads) {
                            if (!A.pt_active[p0 + j]) continue;
                            int o0, o1;
                            point_range(A, Q, j, o0, o1);
                            double* ps = A.pt_sys + (size_t)(p0 + j) * kPtSys;
                            double cl[3] = {ps[6], ps[7], ps[8]};
                            for (int e = o0; e < o1; e++) {
                                const int f = A.rec_free[e];
                                if (f < 0 || A.rec_pt[e] != j) continue;
                                const double* W = A.W + (size_t)e * 18;
                                const double* xp = s_xp + 6 * f;
#pragma unroll
                                for (int a = 0; a < 3; a++) {
                                    double t = W[a * 6] * -xp[0];
#pragma unroll
                                    for (int c = 1; c < 6; c++) t += W[a * 6 + c] * -xp[c];
                                    cl[a] += t;
                                }
                            }
#pragma unroll
                            for (int a = 0; a < 3; a++)
                                ps[21 + a] = ps[9 + 3 * a] * cl[0] + ps[10 + 3 * a] * cl[1] + ps[11 + 3 * a] * cl[2];
                        }
                    }
                    // update (push is the current slot): exp(x) * estimate, += for the points
                    for (int f = tid; f < F; f += kLbThreads) {
                        double* d = A.pose + (size_t)(k0 + s_fk[f]) * 2 * kPoseWords;
                        lm::Pose cur = {d[0], d[1], d[2], d[3], d[4], d[5], d[6]};
                        const double x[6] = {s_xp[6 * f], s_xp[6 * f + 1], s_xp[6 * f + 2], s_xp[6 * f + 3], s_xp[6 * f + 4],
                                             s_xp[6 * f + 5]};
                        const lm::Pose t = lm::pose_update(x, cur);
                        double R[3][3];
                        lm::quat_to_matrix(t.qx, t.qy, t.qz, t.qw, R);
                        double* o = d + kPoseWords;
                        o[0] = t.qx;
                        o[1] = t.qy;
                        o[2] = t.qz;
                        o[3] = t.qw;
                        o[4] = t.tx;
                        o[5] = t.ty;
                        o[6] = t.tz;
#pragma unroll
                        for (int r = 0; r < 3; r++)
#pragma unroll
                            for (int c = 0; c < 3; c++) o[7 + 3 * r + c] = R[r][c];
                    }
                    double sc[1] = {0.0};
                    for (int f = tid; f < F; f += kLbThreads)
#pragma unroll
                        for (int r = 0; r < 6; r++) sc[0] += s_xp[6 * f + r] * (lam * s_xp[6 * f + r] + s_bp[6 * f + r]);
                    for (int j = tid; j < P; j += kLbThreads) {
                        if (!A.pt_active[p0 + j]) continue;
                        const double* ps = A.pt_sys + (size_t)(p0 + j) * kPtSys;
                        double* pp = A.pt + ((size_t)(p0 + j) * 2) * 3;
#pragma unroll
                        for (int a = 0; a < 3; a++) {
                            pp[3 + a] = pp[a] + ps[21 + a];
                            sc[0] += ps[21 + a] * (lam * ps[21 + a] + ps[6 + a]);
                        }
                    }
                    __syncthreads();
                    double temp = active_chi(A, Q, C, 1, robust, s_red);
                    if (!ok) temp = DBL_MAX;
                    lm::block_sum<1, kLbWaves>(sc, s_red);
                    rho = chi - temp;
                    const double scale = sc[0] + 1e-3;
                    rho = rho / scale;
                    if (rho > 0 && isfinite(temp)) {
                        const double t = 2.0 * rho - 1.0;
                        double alpha = 1.0 - t * t * t;
                        alpha = fmin(alpha, 2.0 / 3.0);
                        lam *= fmax(1.0 / 3.0, alpha);
                        ni = 2.0;
                        chi = temp;
                        // discardTop: the trial becomes the estimate
                        for (int i = tid; i < F * kPoseWords; i += kLbThreads) {
                            double* d = A.pose + (size_t)(k0 + s_fk[i / kPoseWords]) * 2 * kPoseWords + i % kPoseWords;
                            d[0] = d[kPoseWords];
                        }
                        for (int j = tid; j < P; j += kLbThreads) {
                            if (!A.pt_active[p0 + j]) continue;
                            double* pp = A.pt + ((size_t)(p0 + j) * 2) * 3;
#pragma unroll
                            for (int a = 0; a < 3; a++) pp[a] = pp[3 + a];
                        }
                    } else {
                        lam *= ni;
                        ni *= 2.0;
                    }
                    __syncthreads();
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
        if (tid == 0 && trace) {
            trace[2 * phase] = its;
            trace[2 * phase + 1] = trials;
        }
        // ---- cc:756-782, 794-821: chi2 of the last computeActiveErrors, the depth now ----
        int bad = 0;
        for (int e = oA + tid; e < oB; e += kLbThreads) {
            const int fl = A.rec_flags[e];
            if (!(fl & kValid)) continue;
            const int j = A.rec_pt[e];
            const double* pp = A.pt + ((size_t)(p0 + j) * 2) * 3;
            const double* Pk = A.pose + ((size_t)(k0 + A.rec_kf[e]) * 2) * kPoseWords;
            double x, y, z;
            lm::quat_rotate(Pk[0], Pk[1], Pk[2], Pk[3], pp[0], pp[1], pp[2], x, y, z);
            z += Pk[6];
            const bool out = A.chi2[e] > ((fl & kStereo) ? 7.815 : 5.991) || !(z > 0.0);
            if (phase == 0) {
                if (out) A.rec_flags[e] = fl | kLevel1;
                if (A.level1) A.level1[e] = out;
            } else {
                A.erase[e] = out;
                bad += out;
            }
        }
        nerase = lm::block_sum_int<kLbWaves>(bad, s_cnt);
        // trial slots of vertices that leave the system follow their estimates
        for (int i = tid; i < K * kPoseWords; i += kLbThreads) {
            double* d = A.pose + (size_t)(k0 + i / kPoseWords) * 2 * kPoseWords + i % kPoseWords;
            d[kPoseWords] = d[0];
        }
        for (int i = tid; i < P * 3; i += kLbThreads) {
            double* pp = A.pt + ((size_t)(p0 + i / 3) * 2) * 3 + i % 3;
            pp[3] = pp[0];
        }
        __syncthreads();
    }

    // ---- cc:838-853: Converter::toCvMat(SE3Quat), positions; fixed keyframes as they came ----
    for (int k = tid; k < K; k += kLbThreads) {
        const float* Tin = A.kf_Tcw + (size_t)(k0 + k) * 12;
        float* To = A.kf_Tcw_out + (size_t)(k0 + k) * 12;
        if (A.kf_fixed[k0 + k]) {
#pragma unroll
            for (int i = 0; i < 12; i++) To[i] = Tin[i];
        } else {
            const double* Pk = A.pose + (size_t)(k0 + k) * 2 * kPoseWords;
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int c = 0; c < 3; c++) To[4 * r + c] = (float)Pk[7 + 3 * r + c];
                To[4 * r + 3] = (float)Pk[4 + r];
            }
        }
    }
    for (int i = tid; i < P * 3; i += kLbThreads)
        A.pt_pos_out[(size_t)p0 * 3 + i] = (float)A.pt[((size_t)(p0 + i / 3) * 2) * 3 + i % 3];
    if (tid == 0) {
        A.n_erase[b] = nerase;
        A.status[b] = nbadidx > 0 ? ORBX_LOCAL_BA_STATUS_BAD_INDEX : 0;
    }
}

// the workspace's regions, in order; returns its size
size_t carve(LocalBaArgs& A, int batch, char* base) {
    const size_t nk = (size_t)A.n_kf, np = (size_t)A.n_pt, no = (size_t)A.n_obs, n = 6 * (size_t)A.max_free;
    Layout L(up256);
    auto take = [&](auto*& field, size_t count) {
        using T = std::remove_reference_t<decltype(*field)>;
        field = (T*)(base + L.take(count * sizeof(T)));
    };
    take(A.pose, nk * 2 * kPoseWords);
    take(A.pt, np * 6);
    take(A.pt_sys, np * kPtSys);
    take(A.W, no * 18);
    take(A.chi2, no);
    take(A.S, (size_t)batch * n * n);
    take(A.rec, no * 4);
    take(A.rec_kf, no);
    take(A.rec_pt, no);
    take(A.rec_flags, no);
    take(A.rec_free, no);
    take(A.kf_free, nk);
    take(A.kf_elist, no);
    take(A.pt_active, np);
    return L.total();
}

}  // namespace

size_t local_ba_workspace_bytes(int batch, int n_kf, int n_pt, int n_obs, int max_free) {
    LocalBaArgs A{};
    A.n_kf = n_kf;
    A.n_pt = n_pt;
    A.n_obs = n_obs;
    A.max_free = max_free;
    return carve(A, batch, nullptr);
}

hipError_t launch_local_ba(LocalBaArgs A, int batch, char* workspace, hipStream_t stream) {
    if (batch <= 0) return hipSuccess;
    carve(A, batch, workspace);
    k_local_ba<<<batch, kLbThreads, 0, stream>>>(A);
    return hipGetLastError();
}

}  // namespace orbx
