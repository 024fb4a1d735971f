// orbx_globalba.hip -- Optimizer::BundleAdjustment / GlobalBundleAdjustemnt for a batch of maps
// in HBM: one persistent workgroup per problem builds the graph, runs one optimize(nIterations)
// and recovers every keyframe and every included point; the host reads nothing back in between.
//
// Reference: src/Optimizer.cc:41-281 and the g2o files that orbx_localba.hip lists (the same
// edges, quadratic form, Huber kernel, Schur complement and Levenberg-Marquardt).
// DESIGN.md §4.23.  The stop flag (pbStopFlag) is not supported: the iteration count is the
// caller's lever.
//
// This is k_local_ba's phase loop with one phase and without its cap: nothing sized by the
// keyframes stays in LDS, the per-keyframe edge lists come from integer counters, a workgroup
// scan and an owner's sort (as orbx_essgraph.hip builds its adjacency), and the reduced system
// S is a block envelope of 6 x 6 blocks factored by env::solve<6> (orbx_envelope.h).
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
//   an entry of S: the wave that owns its block row (row mod 4), which walks the row's edge
//     list -- one edge per point, in point order; within a point an entry belongs to one lane;
//   chi2 and computeScale: thread t adds its points (keyframes) t, t + 256, ..., then block_sum.
// The integer atomics only count and take minima: the lists they fill are sorted into edge
// order, and first[] is a minimum of integers.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "orbx.h"
#include "orbx_ba_edge.h"
#include "orbx_envelope.h"
#include "orbx_kernels.h"
#include "orbx_layout.h"
#include "orbx_lm.h"

namespace orbx {

namespace {

constexpr int kGbThreads = env::kThreads;
constexpr int kGbWaves = env::kWaves;
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
    for (int w = 1; w < kGbWaves; w++) s = fmax(s, s_red[w]);
    __syncthreads();
    return s;
}

// One problem's rows and its regions of the workspace; S, b_s, x and the solver's work
// vectors are env::Envelope's (H == L: S is rebuilt for every trial and factored in place).
struct Prob : env::Envelope {
    int k0, K, p0, P, oA, oB;
    double *hpp, *bp;   // [F][21], [F][6]
    int32_t *free_kf;   // [F] keyframe row of a block column
    int32_t *eoff;      // [F + 1] a block column's edges in kf_elist (from oA)
    int32_t *deg;       // [K] counters
};

__device__ __forceinline__ void point_range(const GlobalBaArgs& A, const Prob& Q, int j, int& o0, int& o1) {
    o0 = clampi(A.obs_off[Q.p0 + j], Q.oA, Q.oB);
    o1 = clampi(A.obs_off[Q.p0 + j + 1], o0, Q.oB);
}

// computeActiveErrors + activeRobustChi2 at the estimates of `slot`
__device__ __forceinline__ double active_chi(const GlobalBaArgs& A, const Prob& Q, const Cam& C, int slot,
                                             bool robust, double* s_red) {
    double v[1] = {0.0};
    for (int j = threadIdx.x; j < Q.P; j += kGbThreads) {
        if (!A.pt_active[Q.p0 + j]) continue;
        int o0, o1;
        point_range(A, Q, j, o0, o1);
        const double* pp = A.pt + ((size_t)(Q.p0 + j) * 2 + slot) * 3;
        const double X[3] = {pp[0], pp[1], pp[2]};
        for (int e = o0; e < o1; e++) {
            const int fl = A.rec_flags[e];
            if (!(fl & kValid)) continue;
            const double* Pk = A.pose + ((size_t)(Q.k0 + A.rec_kf[e]) * 2 + slot) * kPoseWords;
            double err[3], x, y, z, rho1;
            const double chi2 = edge_error(fl, ((const float4*)A.rec)[e], Pk, X, C, err, x, y, z);
            v[0] += lm::huber(chi2, (fl & kStereo) ? C.delta_stereo : C.delta_mono, robust, rho1);
        }
    }
    lm::block_sum<1, kGbWaves>(v, s_red);
    return v[0];
}

__device__ __forceinline__ void return_inputs(const GlobalBaArgs& A, const Prob& Q, int b, int status) {
    const int tid = threadIdx.x;
    for (int i = tid; i < Q.K * 12; i += kGbThreads) A.kf_Tcw_out[(size_t)Q.k0 * 12 + i] = A.kf_Tcw[(size_t)Q.k0 * 12 + i];
    for (int i = tid; i < Q.P * 3; i += kGbThreads) A.pt_pos_out[(size_t)Q.p0 * 3 + i] = A.pt_pos[(size_t)Q.p0 * 3 + i];
    for (int j = tid; j < Q.P; j += kGbThreads) A.pt_included[Q.p0 + j] = 0;
    if (tid == 0) {
        if (A.trace) A.trace[2 * b] = A.trace[2 * b + 1] = 0;
        if (A.chi2) A.chi2[2 * b] = A.chi2[2 * b + 1] = 0.0;
        A.status[b] = status;
    }
}

__global__ __launch_bounds__(kGbThreads) void k_global_ba(GlobalBaArgs A) {
    __shared__ double s_red[kGbWaves];
    __shared__ long long s_scan[kGbWaves];
    __shared__ int s_cnt[8];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    Prob Q;
    Q.k0 = clampi(A.kf_off[b], 0, A.n_kf);
    Q.K = clampi(A.kf_off[b + 1], Q.k0, A.n_kf) - Q.k0;
    Q.p0 = clampi(A.pt_off[b], 0, A.n_pt);
    Q.P = clampi(A.pt_off[b + 1], Q.p0, A.n_pt) - Q.p0;
    Q.oA = clampi(A.obs_off[Q.p0], 0, A.n_obs);
    Q.oB = clampi(A.obs_off[Q.p0 + Q.P], Q.oA, A.n_obs);
    const int k0 = Q.k0, K = Q.K, p0 = Q.p0, P = Q.P, oA = Q.oA, oB = Q.oB;
    Q.F = 0;
    Q.L = Q.H = A.L + (size_t)b * (size_t)A.max_env_blocks * 36;
    Q.bp = A.vec + (size_t)k0 * 30;
    Q.b = Q.bp + (size_t)K * 6;
    Q.x = Q.b + (size_t)K * 6;
    Q.xs = Q.x + (size_t)K * 6;
    Q.ys = Q.xs + (size_t)K * 6;
    Q.hpp = A.hpp + (size_t)k0 * 21;
    Q.first = A.first + k0 + b;  // K + 1 entries per problem, as eoff, col_off and row_off
    Q.eoff = A.eoff + k0 + b;
    Q.col_off = A.col_off + k0 + b;
    Q.row_off = A.row_off + k0 + b;
    Q.rows = A.rows + (size_t)b * (size_t)A.max_env_blocks;
    Q.free_kf = A.free_kf + k0;
    Q.deg = A.deg + k0;

    int nfree = 0;
    for (int k = tid; k < K; k += kGbThreads) nfree += A.kf_fixed[k0 + k] ? 0 : 1;
    nfree = lm::block_sum_int<kGbWaves>(nfree, s_cnt);
    if (nfree == 0) {  // the reference is undefined here: the inputs come back
        return_inputs(A, Q, b, ORBX_GLOBAL_BA_STATUS_NO_FREE_KF);
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
    const bool robust = A.robust != 0;

    // ---- vertices and edge records (cc:79-221) ----
    for (int k = tid; k < K; k += kGbThreads) {
        double Pk[kPoseWords];
        pose_from_tcw(A.kf_Tcw + (size_t)(k0 + k) * 12, Pk);
        double* d = A.pose + (size_t)(k0 + k) * 2 * kPoseWords;
#pragma unroll
        for (int i = 0; i < kPoseWords; i++) d[i] = d[kPoseWords + i] = Pk[i];
        Q.deg[k] = 0;
        A.kf_free[k0 + k] = -1;
#pragma unroll
        for (int i = 0; i < 6; i++) Q.x[6 * k + i] = 0.0;  // the solver's x starts at zero
    }
    for (int i = tid; i < P * 3; i += kGbThreads) {
        const int j = i / 3, c = i - 3 * j;
        const double v = (double)A.pt_pos[(size_t)p0 * 3 + i];
        A.pt[((size_t)(p0 + j) * 2) * 3 + c] = v;
        A.pt[((size_t)(p0 + j) * 2 + 1) * 3 + c] = v;
        A.pt_sys[(size_t)(p0 + j) * kPtSys + 21 + c] = 0.0;
    }
    for (int e = oA + tid; e < oB; e += kGbThreads) {
        A.rec_kf[e] = -1;
        A.rec_pt[e] = -1;
        A.rec_flags[e] = 0;
        A.rec_free[e] = -1;
    }
    __syncthreads();
    int nbadidx = 0, nact = 0;
    for (int j = tid; j < P; j += kGbThreads) {
        int o0, o1, any = 0;
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
            const bool stereo = !(ur < 0);  // cc:160
            int oct = kpt.octave;
            oct = oct < 0 ? 0 : (oct >= A.nlevels ? A.nlevels - 1 : oct);
            ((float4*)A.rec)[e] = make_float4(kpt.x, kpt.y, stereo ? ur : 0.0f, A.inv_sigma2[oct]);
            A.rec_kf[e] = kf;
            A.rec_pt[e] = j;
            A.rec_flags[e] = kValid | (stereo ? kStereo : 0);
            atomicAdd(&Q.deg[kf], 1);
            any = 1;
            nact++;
        }
        A.pt_active[p0 + j] = any;  // cc:223-228: a point without an edge is not included
    }
    nbadidx = lm::block_sum_int<kGbWaves>(nbadidx, s_cnt);
    nact = lm::block_sum_int<kGbWaves>(nact, s_cnt);
    auto degree = [&](int v) { return __hip_atomic_load(&Q.deg[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };

    // ---- the keyframes that may move and have an edge, in table order; their edge lists ----
    const int F = env::block_scan<int>([&](int k) { return !A.kf_fixed[k0 + k] && degree(k) > 0 ? 1 : 0; },
                                       (int*)Q.first, K, (int*)s_scan);
    Q.F = F;
    __syncthreads();
    for (int k = tid; k < K; k += kGbThreads)
        if (!A.kf_fixed[k0 + k] && degree(k) > 0) {
            A.kf_free[k0 + k] = Q.first[k];
            Q.free_kf[Q.first[k]] = k;
        }
    __syncthreads();
    env::block_scan<int>([&](int f) { return degree(Q.free_kf[f]); }, (int*)Q.eoff, F, (int*)s_scan);
    __syncthreads();
    for (int k = tid; k < K; k += kGbThreads) Q.deg[k] = 0;
    __syncthreads();
    for (int e = oA + tid; e < oB; e += kGbThreads) {
        if (!(A.rec_flags[e] & kValid)) continue;
        const int f = A.kf_free[k0 + A.rec_kf[e]];
        A.rec_free[e] = f;
        if (f >= 0) A.kf_elist[oA + Q.eoff[f] + atomicAdd(&Q.deg[f], 1)] = e;
    }
    __syncthreads();
    for (int f = tid; f < F; f += kGbThreads) {  // into edge order
        env::sort_ascending(A.kf_elist + oA + Q.eoff[f], Q.eoff[f + 1] - Q.eoff[f]);
        Q.deg[f] = f;
    }
    __syncthreads();

    // ---- the envelope of S: first[f] is the smallest block column that shares a point with f
    // (an integer minimum per block column, taken in the counters) ----
    for (int j = tid; j < P; j += kGbThreads) {
        int o0, o1, m = F;
        point_range(A, Q, j, o0, o1);
        for (int e = o0; e < o1; e++) {
            const int f = A.rec_free[e];
            if (f >= 0 && f < m) m = f;
        }
        for (int e = o0; e < o1; e++) {
            const int f = A.rec_free[e];
            if (f > m) atomicMin(&Q.deg[f], m);
        }
    }
    __syncthreads();
    for (int f = tid; f < F; f += kGbThreads) Q.first[f] = A.dense ? 0 : degree(f);
    __syncthreads();
    const long long blocks =
        env::block_scan<long long>([&](int f) { return (long long)(f - Q.first[f] + 1); }, Q.col_off, F, s_scan);
    const int bad_bit = nbadidx > 0 ? ORBX_GLOBAL_BA_STATUS_BAD_INDEX : 0;
    if (blocks > A.max_env_blocks) {
        return_inputs(A, Q, b, ORBX_GLOBAL_BA_STATUS_CAPACITY | bad_bit);
        return;
    }
    env::row_lists(Q, Q.deg, s_scan);
    const int n = 6 * F;
    const size_t env_words = (size_t)blocks * 36;

    // ---- optimize(nIterations) (cc:231-233) ----
    const int max_it = A.iterations > 0 ? A.iterations : 10;
    int its = 0, trials = 0;
    double chi0 = 0.0, chi = 0.0;
    if (nact == 0 || F == 0) {
        chi0 = chi = active_chi(A, Q, C, 0, robust, s_red);
    } else {
        double lam = 0.0, ni = 2.0;
        int nbad = 0;
        for (int it = 0; it < max_it; it++) {
            // computeActiveErrors, activeRobustChi2, buildSystem: the points' side
            double v[1] = {0.0};
            double md = 0.0;
            for (int j = tid; j < P; j += kGbThreads) {
                if (!A.pt_active[p0 + j]) continue;
                int o0, o1;
                point_range(A, Q, j, o0, o1);
                const double* pp = A.pt + ((size_t)(p0 + j) * 2) * 3;
                const double X[3] = {pp[0], pp[1], pp[2]};
                double h[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, bl[3] = {0.0, 0.0, 0.0};
                for (int e = o0; e < o1; e++) {
                    const int fl = A.rec_flags[e];
                    if (!(fl & kValid)) continue;
                    const bool stereo = fl & kStereo;
                    const float4 r = ((const float4*)A.rec)[e];
                    const double* Pk = A.pose + ((size_t)(k0 + A.rec_kf[e]) * 2) * kPoseWords;
                    double err[3], x, y, z, rho1;
                    const double chi2 = edge_error(fl, r, Pk, X, C, err, x, y, z);
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
            lm::block_sum<1, kGbWaves>(v, s_red);
            chi = v[0];
            const double ini_chi = chi;
            // the keyframes' side: Hpp and b_p of every block column, by its wave
            for (int f = wave; f < F; f += kGbWaves) {
                const double* Pk = A.pose + ((size_t)(k0 + Q.free_kf[f]) * 2) * kPoseWords;
                double acc[27];
#pragma unroll
                for (int i = 0; i < 27; i++) acc[i] = 0.0;
                for (int i = Q.eoff[f] + lane; i < Q.eoff[f + 1]; i += 64) {
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
                    for (int i = 0; i < 21; i++) Q.hpp[f * 21 + i] = acc[i];
#pragma unroll
                    for (int i = 0; i < 6; i++) Q.bp[f * 6 + i] = acc[21 + i];
                }
            }
            __syncthreads();
            if (it == 0) {  // computeLambdaInit: tau = 1e-5 over every active vertex
                for (int i = tid; i < n; i += kGbThreads) {
                    const int f = i / 6, r = i - 6 * f;
                    md = fmax(fabs(Q.hpp[f * 21 + r * 6 - (r * (r - 1)) / 2]), md);
                }
                md = block_max(md, s_red);
                lam = 1e-5 * md;
                ni = 2.0;
                nbad = 0;
                chi0 = chi;
            }
            int qmax = 0;
            double rho = 0.0;
            do {
                // setLambda, the landmark inverses (block_solver.hpp:381-395; Eigen's 3x3 inverse by cofactors)
                for (int j = tid; j < P; j += kGbThreads) {
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
                // S = Hpp + lambda I (upper triangles of the diagonal blocks), zero elsewhere
                for (size_t i = tid; i < env_words; i += kGbThreads) Q.L[i] = 0.0;
                __syncthreads();
                for (int i = tid; i < F * 36; i += kGbThreads) {
                    const int f = i / 36, ent = i - 36 * f, a = ent / 6, d = ent - 6 * a;
                    if (a <= d)
                        env::diag_block<6>(Q, Q.L, f)[ent] =
                            Q.hpp[f * 21 + a * 6 - (a * (a - 1)) / 2 + (d - a)] + (a == d ? lam : 0.0);
                }
                __syncthreads();
                // S -= B Dinv B^T (block_solver.hpp:400-431): block row f1 by its wave, over its edge list,
                // which holds one edge per point in point order; block (f1, f2), f1 <= f2, lies in column f2
                for (int f1 = wave; f1 < F; f1 += kGbWaves) {
                    for (int t = Q.eoff[f1]; t < Q.eoff[f1 + 1]; t++) {
                        const int e1 = A.kf_elist[oA + t], j = A.rec_pt[e1];
                        int o0, o1;
                        point_range(A, Q, j, o0, o1);
                        const double* D = A.pt_sys + (size_t)(p0 + j) * kPtSys + 9;
                        const double* W1 = A.W + (size_t)e1 * 18;
                        const int items = (o1 - o0) * 36;
                        for (int i = lane; i < items; i += 64) {
                            const int e2 = o0 + i / 36, ent = i % 36, r = ent / 6, c = ent - 6 * r;
                            const int f2 = A.rec_free[e2];
                            if (f2 < f1) continue;
                            if (f2 == f1 && (e2 != e1 || r > c)) continue;
                            const double* W2 = A.W + (size_t)e2 * 18;
                            const double w0 = W1[r], w1 = W1[6 + r], w2 = W1[12 + r];
                            const double bd0 = w0 * D[0] + w1 * D[3] + w2 * D[6];
                            const double bd1 = w0 * D[1] + w1 * D[4] + w2 * D[7];
                            const double bd2 = w0 * D[2] + w1 * D[5] + w2 * D[8];
                            double* s = Q.L + (size_t)(Q.col_off[f2] + f1 - Q.first[f2]) * 36 + ent;
                            *s = *s - (bd0 * W2[c] + bd1 * W2[6 + c] + bd2 * W2[12 + c]);
                        }
                        // the next point's updates of an entry follow this point's, whichever lane makes them
                        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    }
                }
                // b_s = b_p - B Dinv b_l (block_solver.hpp:413, 436-439)
                for (int f = wave; f < F; f += kGbWaves) {
                    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                    for (int i = Q.eoff[f] + lane; i < Q.eoff[f + 1]; i += 64) {
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
                        for (int r = 0; r < 6; r++) Q.b[f * 6 + r] = Q.bp[f * 6 + r] - acc[r];
                    }
                }
                __syncthreads();
                const bool ok = env::solve<6, false>(Q, 0.0);  // lambda is in S; a failed solve leaves x as it was
                __syncthreads();
                if (ok) {
                    // x_l = Dinv (b_l - B^T x_p) (block_solver.hpp:468-481)
                    for (int j = tid; j < P; j += kGbThreads) {
                        if (!A.pt_active[p0 + j]) continue;
                        int o0, o1;
                        point_range(A, Q, j, o0, o1);
                        double* ps = A.pt_sys + (size_t)(p0 + j) * kPtSys;
                        double cl[3] = {ps[6], ps[7], ps[8]};
                        for (int e = o0; e < o1; e++) {
                            const int f = A.rec_free[e];
                            if (f < 0) continue;
                            const double* W = A.W + (size_t)e * 18;
                            const double* xp = Q.x + 6 * f;
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
                double sc[1] = {0.0};
                for (int f = tid; f < F; f += kGbThreads) {
                    double* d = A.pose + (size_t)(k0 + Q.free_kf[f]) * 2 * kPoseWords;
                    lm::Pose cur = {d[0], d[1], d[2], d[3], d[4], d[5], d[6]};
                    const double* xp = Q.x + 6 * f;
                    const double x[6] = {xp[0], xp[1], xp[2], xp[3], xp[4], xp[5]};
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
#pragma unroll
                    for (int r = 0; r < 6; r++) sc[0] += x[r] * (lam * x[r] + Q.bp[6 * f + r]);
                }
                for (int j = tid; j < P; j += kGbThreads) {
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
                lm::block_sum<1, kGbWaves>(sc, s_red);
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
                    for (int i = tid; i < F * kPoseWords; i += kGbThreads) {
                        double* d = A.pose + (size_t)(k0 + Q.free_kf[i / kPoseWords]) * 2 * kPoseWords + i % kPoseWords;
                        d[0] = d[kPoseWords];
                    }
                    for (int j = tid; j < P; j += kGbThreads) {
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

    // ---- cc:236-280: Converter::toCvMat(SE3Quat) of every keyframe, the fixed ones too; positions ----
    for (int k = tid; k < K; k += kGbThreads) {
        float* To = A.kf_Tcw_out + (size_t)(k0 + k) * 12;
        const double* Pk = A.pose + (size_t)(k0 + k) * 2 * kPoseWords;
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) To[4 * r + c] = (float)Pk[7 + 3 * r + c];
            To[4 * r + 3] = (float)Pk[4 + r];
        }
    }
    for (int i = tid; i < P * 3; i += kGbThreads) {
        const int j = i / 3;
        A.pt_pos_out[(size_t)p0 * 3 + i] = A.pt_active[p0 + j] ? (float)A.pt[((size_t)(p0 + j) * 2) * 3 + i % 3]
                                                               : A.pt_pos[(size_t)p0 * 3 + i];
    }
    for (int j = tid; j < P; j += kGbThreads) A.pt_included[p0 + j] = A.pt_active[p0 + j] ? 1 : 0;
    if (tid == 0) {
        if (A.trace) {
            A.trace[2 * b] = its;
            A.trace[2 * b + 1] = trials;
        }
        if (A.chi2) {
            A.chi2[2 * b] = chi0;
            A.chi2[2 * b + 1] = chi;
        }
        A.status[b] = bad_bit;
    }
}

// the workspace's regions, in order; returns its size
size_t carve(GlobalBaArgs& A, int batch, char* base) {
    const size_t nk = (size_t)A.n_kf, np = (size_t)A.n_pt, no = (size_t)A.n_obs,
                 nb = (size_t)batch * (size_t)A.max_env_blocks;
    Layout L(up256);
    auto take = [&](auto*& field, size_t count) {
        using T = std::remove_reference_t<decltype(*field)>;
        field = (T*)(base + L.take(count * sizeof(T)));
    };
    take(A.pose, nk * 2 * kPoseWords);
    take(A.pt, np * 6);
    take(A.pt_sys, np * kPtSys);
    take(A.W, no * 18);
    take(A.L, nb * 36);
    take(A.hpp, nk * 21);
    take(A.vec, nk * 30);
    take(A.col_off, nk + batch);
    take(A.row_off, nk + batch);
    take(A.rec, no * 4);
    take(A.rows, nb);
    take(A.rec_kf, no);
    take(A.rec_pt, no);
    take(A.rec_flags, no);
    take(A.rec_free, no);
    take(A.kf_elist, no);
    take(A.kf_free, nk);
    take(A.free_kf, nk);
    take(A.deg, nk);
    take(A.first, nk + batch);
    take(A.eoff, nk + batch);
    take(A.pt_active, np);
    return L.total();
}

}  // namespace

size_t global_ba_workspace_bytes(int batch, int n_kf, int n_pt, int n_obs, long long max_env_blocks) {
    GlobalBaArgs A{};
    A.n_kf = n_kf;
    A.n_pt = n_pt;
    A.n_obs = n_obs;
    A.max_env_blocks = max_env_blocks;
    return carve(A, batch, nullptr);
}

hipError_t launch_global_ba(GlobalBaArgs A, int batch, char* workspace, hipStream_t stream) {
    if (batch <= 0) return hipSuccess;
    carve(A, batch, workspace);
    k_global_ba<<<batch, kGbThreads, 0, stream>>>(A);
    return hipGetLastError();
}

}  // namespace orbx
