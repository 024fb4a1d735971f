// orbx_optsim3.hip -- Optimizer::OptimizeSim3 (the Sim3 refinement of a loop candidate) for a
// batch of candidates in HBM: one persistent workgroup per candidate builds the edge pairs,
// runs both Levenberg-Marquardt optimisations and both classifications; the host reads
// nothing back in between.
//
// Reference: src/Optimizer.cc:1173-1358 and, under Thirdparty/g2o/g2o,
//   types/types_seven_dof_expmap.h:48-171             oplusImpl, cam_map1 / cam_map2, computeError
//   types/sim3.h:64-142, 144, 233, 266                Sim3(R, t, s), exp, map, inverse, operator*
//   core/base_binary_edge.hpp:55-120, 131-205         constructQuadraticForm, numeric linearizeOplus
//   core/optimization_algorithm_levenberg.cpp:61-189  solve, computeLambdaInit, computeScale
//   core/sparse_optimizer.cpp:61-114, 354-419         computeActiveErrors, activeRobustChi2, optimize
//   core/base_edge.h:59-61, 96-102                    chi2, robustInformation (no second-order term)
//   core/robust_kernel_impl.cpp:78-91                 RobustKernelHuber::robustify
//   solvers/linear_solver_dense.h:104-112             LDLT; not positive = failed solve
// DESIGN.md §4.17.
//
// Float inputs are widened to double; everything after is double (the build keeps
// -ffp-contract=off), except the fixed points P3D1c / P3D2c, which the reference computes as
// CV_32F matrices: float products and sums (r0 x + r1 y) + r2 z, the translation added in
// double and the result rounded to float once.  The vertex is g2o's Sim3: a quaternion that
// is never normalised, a translation and a scale.
//
// Both edge classes leave linearizeOplus to g2o's central difference, so a linearisation
// needs the estimate and the 14 probes Sim3(+-1e-9 e_d) * estimate, and their inverses for
// the inverse edge: 30 transforms, the same for every edge, built once per linearisation by
// 15 threads and kept in LDS.  The 14 probe increments do not depend on the data: the host
// builds them (launch_opt_sim3) and passes them in the kernel arguments.
//
// Sums over edges (the 28 upper entries of H, the 7 of b, chi2) have a fixed shape: thread t
// adds its pairs t, t + 256, ... in index order, the forward edge before the inverse one as
// g2o's active-edge order has them, the 64 lanes of a wave are combined by a __shfl_xor
// butterfly, the four waves are added in wave order from LDS.  There are no floating-point
// atomics.  After each reduction every thread holds the same sums and runs the scalar part
// (LDLT, exponential map, accept / reject) redundantly, so the control flow is uniform.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "orbx.h"
#include "orbx_kernels.h"
#include "orbx_lm.h"
#include "orbx_sim3.h"

namespace orbx {

namespace {

constexpr int kOsThreads = 256;
constexpr int kOsWaves = kOsThreads / 64;
constexpr int kOsSums = 36;      // H upper [28], -b [7], chi
constexpr int kOsRecWords = 12;  // P3D1c[3], P3D2c[3], obs1[2], obs2[2], invSigma2 of either keyframe
constexpr int kOsXf = 15;        // transforms per direction: 14 probes and the estimate

struct Cam2 {
    double fx, fy, cx, cy;
};

// computeError of one edge (types_seven_dof_expmap.h:138-145, 160-167): obs - cam_map(project(
// T.map(X))), T the estimate for the forward edge and its inverse for the inverse edge
__device__ __forceinline__ void edge_error(const S3& T, double X, double Y, double Z, double u, double v,
                                           const Cam2& C, double& e0, double& e1) {
    double rx, ry, rz;
    lm::quat_rotate(T.qx, T.qy, T.qz, T.qw, X, Y, Z, rx, ry, rz);
    const double x = T.s * rx + T.tx, y = T.s * ry + T.ty, z = T.s * rz + T.tz;
    e0 = u - ((x / z) * C.fx + C.cx);
    e1 = v - ((y / z) * C.fy + C.cy);
}

__device__ __forceinline__ double edge_chi2(double e0, double e1, double w) {
    return e0 * (w * e0) + e1 * (w * e1);  // base_edge.h:59-61
}

struct Pair {
    double X1[3], X2[3], u1, v1, u2, v2, w1, w2;
};

__device__ __forceinline__ Pair load_pair(const float* rec, int stride, int e) {
    Pair P;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        P.X1[k] = (double)rec[k * stride + e];
        P.X2[k] = (double)rec[(3 + k) * stride + e];
    }
    P.u1 = (double)rec[6 * stride + e];
    P.v1 = (double)rec[7 * stride + e];
    P.u2 = (double)rec[8 * stride + e];
    P.v2 = (double)rec[9 * stride + e];
    P.w1 = (double)rec[10 * stride + e];
    P.w2 = (double)rec[11 * stride + e];
    return P;
}

// One edge's share of chi, H and b: computeError, robustify, the central-difference Jacobian
// over the 14 probes at xf (base_binary_edge.hpp:147-196) and the robust branch of
// constructQuadraticForm (91-113) for the free `to` vertex.
__device__ __forceinline__ void add_edge(const double* xf, double* s_j, double X, double Y, double Z, double u,
                                         double v, double w, const Cam2& C, double delta, double (&acc)[kOsSums]) {
    double e0, e1;
    edge_error(s3_load(xf + 14 * 8), X, Y, Z, u, v, C, e0, e1);
    double rho1;
    acc[35] += lm::huber(edge_chi2(e0, e1, w), delta, true, rho1);
    const double scalar = 1.0 / (2 * 1e-9);
    // the columns go through the thread's own LDS words (s_j[k * kOsThreads]) so that this loop
    // stays rolled: unrolled, the 30 transforms are hoisted into registers and spill
#pragma unroll 1
    for (int d = 0; d < 7; d++) {
        double p0, p1, m0, m1;
        edge_error(s3_load(xf + (2 * d) * 8), X, Y, Z, u, v, C, p0, p1);
        edge_error(s3_load(xf + (2 * d + 1) * 8), X, Y, Z, u, v, C, m0, m1);
        s_j[(2 * d) * kOsThreads] = scalar * (p0 - m0);
        s_j[(2 * d + 1) * kOsThreads] = scalar * (p1 - m1);
    }
    double J[2][7];
#pragma unroll
    for (int d = 0; d < 7; d++) {
        J[0][d] = s_j[(2 * d) * kOsThreads];
        J[1][d] = s_j[(2 * d + 1) * kOsThreads];
    }
    // omega_r = -(Omega e) rho'; the sign is taken after the sum.  weightedOmega = rho' Omega
    const double r0 = (w * e0) * rho1, r1 = (w * e1) * rho1;
    const double ww = rho1 * w;
    int k = 0;
#pragma unroll
    for (int r = 0; r < 7; r++) {
#pragma unroll
        for (int c = r; c < 7; c++, k++) acc[k] += J[0][r] * ww * J[0][c] + J[1][r] * ww * J[1][c];
        acc[28 + r] += J[0][r] * r0 + J[1][r] * r1;
    }
}

struct Ctx {
    const float* rec;
    const int32_t* active;
    int stride, ne;
    Cam2 C1, C2;
    double delta;
    const S3* probes;  // [14] kernel arguments
    double *s_red, *s_sum, *s_xf, *s_j;
    int* s_cnt;
};

// computeActiveErrors + activeRobustChi2 + buildSystem at estimate P: s_sum[0..27] the upper
// triangle of H row by row, s_sum[28..34] = -b, s_sum[35] = chi.
__device__ __forceinline__ void linearize(const Ctx& K, const S3& P) {
    if (threadIdx.x < kOsXf) {
        const S3 T = threadIdx.x < 14 ? s3_mul(K.probes[threadIdx.x], P) : P;
        s3_store(K.s_xf + threadIdx.x * 8, T);
        s3_store(K.s_xf + (kOsXf + threadIdx.x) * 8, s3_inverse(T));
    }
    __syncthreads();
    double v[kOsSums];
#pragma unroll
    for (int k = 0; k < kOsSums; k++) v[k] = 0.0;
    for (int e = threadIdx.x; e < K.ne; e += kOsThreads) {
        if (!K.active[e]) continue;
        const Pair Q = load_pair(K.rec, K.stride, e);
        add_edge(K.s_xf, K.s_j, Q.X2[0], Q.X2[1], Q.X2[2], Q.u1, Q.v1, Q.w1, K.C1, K.delta, v);               // e12
        add_edge(K.s_xf + kOsXf * 8, K.s_j, Q.X1[0], Q.X1[1], Q.X1[2], Q.u2, Q.v2, Q.w2, K.C2, K.delta, v);  // e21
    }
    lm::block_sum_lds<kOsSums, kOsWaves>(v, K.s_red, K.s_sum);
}

// computeActiveErrors + activeRobustChi2 at a trial estimate
__device__ __forceinline__ double robust_chi(const Ctx& K, const S3& P) {
    const S3 Pi = s3_inverse(P);
    double v[1] = {0.0};
    for (int e = threadIdx.x; e < K.ne; e += kOsThreads) {
        if (!K.active[e]) continue;
        const Pair Q = load_pair(K.rec, K.stride, e);
        double e0, e1, rho1;
        edge_error(P, Q.X2[0], Q.X2[1], Q.X2[2], Q.u1, Q.v1, K.C1, e0, e1);
        v[0] += lm::huber(edge_chi2(e0, e1, Q.w1), K.delta, true, rho1);
        edge_error(Pi, Q.X1[0], Q.X1[1], Q.X1[2], Q.u2, Q.v2, K.C2, e0, e1);
        v[0] += lm::huber(edge_chi2(e0, e1, Q.w2), K.delta, true, rho1);
    }
    lm::block_sum<1, kOsWaves>(v, K.s_red);
    return v[0];
}

// SparseOptimizer::optimize(max_its) with OptimizationAlgorithmLevenberg from estimate `cur`
// (lambda initialised at iteration 0); errp is left at the estimate of the last
// computeActiveErrors.  The caller has at least one active edge.
__device__ __forceinline__ void optimize(const Ctx& K, int max_its, bool fix_scale, S3& cur, S3& errp, int& its,
                                         int& trials) {
    double lam = 0.0, ni = 2.0, x[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int nbad = 0;
    its = 0;
    trials = 0;
    errp = cur;
    for (int it = 0; it < max_its; it++) {
        // the next linearize writes s_sum only after a barrier that follows this iteration's last read
        const double* h = K.s_sum;
        linearize(K, cur);
        errp = cur;
        double b[7];
#pragma unroll
        for (int j = 0; j < 7; j++) b[j] = -h[28 + j];
        double chi = h[35];
        const double ini_chi = chi;
        if (it == 0) {  // computeLambdaInit: tau = 1e-5
            double md = 0.0;
            md = fmax(fabs(h[0]), md);
            md = fmax(fabs(h[7]), md);
            md = fmax(fabs(h[13]), md);
            md = fmax(fabs(h[18]), md);
            md = fmax(fabs(h[22]), md);
            md = fmax(fabs(h[25]), md);
            md = fmax(fabs(h[27]), md);
            lam = 1e-5 * md;
            ni = 2.0;
            nbad = 0;
        }
        int qmax = 0;
        double rho = 0.0;
        do {
            const bool ok = lm::ldlt_solve<7>(h, lam, b, x);
            if (fix_scale) x[6] = 0;  // oplusImpl zeroes the solver's entry in place
            const S3 trial = s3_mul(s3_exp(x), cur);
            double temp = robust_chi(K, trial);
            errp = trial;
            if (!ok) temp = DBL_MAX;
            rho = chi - temp;
            double scale = 0.0;
#pragma unroll
            for (int j = 0; j < 7; j++) scale += x[j] * (lam * x[j] + b[j]);
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

// cc:1306-1321 / 1340-1352 over the active pairs: chi2 of the last computeActiveErrors
// (estimate errp) against th2 in double; a rejected pair leaves the graph and its matches12
// entry becomes -1.  Returns the pairs rejected by this pass.
__device__ __forceinline__ int classify(const Ctx& K, const S3& errp, double th2, int32_t* active,
                                        const int32_t* eidx, int32_t* matches12) {
    const S3 Pi = s3_inverse(errp);
    int bad = 0;
    for (int e = threadIdx.x; e < K.ne; e += kOsThreads) {
        if (!active[e]) continue;
        const Pair Q = load_pair(K.rec, K.stride, e);
        double a0, a1, b0, b1;
        edge_error(errp, Q.X2[0], Q.X2[1], Q.X2[2], Q.u1, Q.v1, K.C1, a0, a1);
        edge_error(Pi, Q.X1[0], Q.X1[1], Q.X1[2], Q.u2, Q.v2, K.C2, b0, b1);
        if (edge_chi2(a0, a1, Q.w1) > th2 || edge_chi2(b0, b1, Q.w2) > th2) {
            active[e] = 0;
            matches12[eidx[e]] = -1;
            bad++;
        }
    }
    return lm::block_sum_int<kOsWaves>(bad, K.s_cnt);
}

// Rcw * Xw + tcw as the reference's CV_32F expression (cc:1240, 1250), DESIGN.md App. B:
// float products and sums (r0 x + r1 y) + r2 z, then the translation added in double and
// rounded to float once
__device__ __forceinline__ float cam_coord(const float* T, int r, float x, float y, float z) {
    const float s = (T[4 * r] * x + T[4 * r + 1] * y) + T[4 * r + 2] * z;
    return (float)((double)s + (double)T[4 * r + 3]);
}

__global__ __launch_bounds__(kOsThreads) void k_opt_sim3(OptSim3Args A) {
    __shared__ double s_red[kOsWaves * kOsSums];
    __shared__ double s_sum[kOsSums];
    __shared__ double s_xf[2 * kOsXf * 8];
    __shared__ double s_jac[14 * kOsThreads];
    __shared__ int s_cnt[8];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cap1 = A.cap1, cap2 = A.cap2;
    int n1 = A.n1[b], n2 = A.n2[b];
    n1 = n1 < 0 ? 0 : (n1 > cap1 ? cap1 : n1);
    n2 = n2 < 0 ? 0 : (n2 > cap2 ? cap2 : n2);
    const size_t row1 = (size_t)b * cap1, row2 = (size_t)b * cap2;
    float* rec = A.rec + row1 * kOsRecWords;
    int32_t* eidx = A.eidx + row1;
    int32_t* active = A.active + row1;
    const orbx_keypoint* kps1 = A.kps1 + row1;
    const orbx_keypoint* kps2 = A.kps2 + row2;
    const int32_t* mp1 = A.mp1 + row1;
    const int32_t* idx2 = A.idx2 + row1;
    int32_t* matches12 = A.matches12 + row1;
    const float* T1 = A.Tcw1 + (size_t)b * 12;
    const float* T2 = A.Tcw2 + (size_t)b * 12;
    int32_t* trace = A.trace ? A.trace + (size_t)b * 4 : nullptr;

    // The pairs in slot order (cc:1224-1298), compacted into SoA records
    int ne = 0;
    for (int c0 = 0; c0 < n1; c0 += kOsThreads) {
        const int i = c0 + tid;
        int id1 = -1, id2 = -1, i2 = -1;
        if (i < n1) {
            id1 = mp1[i];
            id2 = matches12[i];
            i2 = idx2[i];
        }
        const bool has = id1 >= 0 && id1 < A.n_mp && id2 >= 0 && id2 < A.n_mp && i2 >= 0 && i2 < n2;
        const unsigned long long m = __ballot(has);
        if (lane == 0) s_cnt[wave] = __popcll(m);
        __syncthreads();
        int off = ne, total = 0;
#pragma unroll
        for (int w = 0; w < kOsWaves; w++) {
            if (w < wave) off += s_cnt[w];
            total += s_cnt[w];
        }
        if (has) {
            const int e = off + __popcll(m & ((1ull << lane) - 1ull));
            const orbx_keypoint k1 = kps1[i], k2 = kps2[i2];
            int o1 = k1.octave, o2 = k2.octave;
            o1 = o1 < 0 ? 0 : (o1 >= A.nlevels ? A.nlevels - 1 : o1);
            o2 = o2 < 0 ? 0 : (o2 >= A.nlevels ? A.nlevels - 1 : o2);
            const float* p1 = A.pos + (size_t)id1 * 3;
            const float* p2 = A.pos + (size_t)id2 * 3;
#pragma unroll
            for (int r = 0; r < 3; r++) {
                rec[r * cap1 + e] = cam_coord(T1, r, p1[0], p1[1], p1[2]);
                rec[(3 + r) * cap1 + e] = cam_coord(T2, r, p2[0], p2[1], p2[2]);
            }
            rec[6 * cap1 + e] = k1.x;
            rec[7 * cap1 + e] = k1.y;
            rec[8 * cap1 + e] = k2.x;
            rec[9 * cap1 + e] = k2.y;
            rec[10 * cap1 + e] = A.inv_sigma2_1[o1];
            rec[11 * cap1 + e] = A.inv_sigma2_2[o2];
            eidx[e] = i;
            active[e] = 1;
        }
        ne += total;
        __syncthreads();
    }

    Ctx K;
    K.rec = rec;
    K.active = active;
    K.stride = cap1;
    K.ne = ne;
    K.C1 = {(double)A.K1[0], (double)A.K1[1], (double)A.K1[2], (double)A.K1[3]};
    K.C2 = {(double)A.K2[0], (double)A.K2[1], (double)A.K2[2], (double)A.K2[3]};
    K.delta = (double)A.delta;
    K.probes = (const S3*)A.probes;
    K.s_red = s_red;
    K.s_sum = s_sum;
    K.s_xf = s_xf;
    K.s_j = s_jac + tid;
    K.s_cnt = s_cnt;
    const double th2 = (double)A.th2;

    // g2o::Sim3(R, t, s): Quaterniond(R), not normalised
    const float* Rin = A.R12 + (size_t)b * 9;
    const float* tin = A.t12 + (size_t)b * 3;
    double R[3][3], q[4];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) R[r][c] = (double)Rin[3 * r + c];
    lm::quat_from_matrix(R, q);
    S3 cur;
    cur.qx = q[0];
    cur.qy = q[1];
    cur.qz = q[2];
    cur.qw = q[3];
    cur.tx = (double)tin[0];
    cur.ty = (double)tin[1];
    cur.tz = (double)tin[2];
    cur.s = (double)A.s12[b];
    S3 errp = cur;

    int its[2] = {0, 0}, trials[2] = {0, 0};
    int nbad = 0, nin = 0;
    bool done = false;
    if (ne > 0) {  // with zero edges optimize() runs no iteration
        optimize(K, 5, A.fix_scale != 0, cur, errp, its[0], trials[0]);
        nbad = classify(K, errp, th2, active, eidx, matches12);
    }
    if (ne - nbad >= 10) {  // cc:1331
        optimize(K, nbad > 0 ? 10 : 5, A.fix_scale != 0, cur, errp, its[1], trials[1]);
        const int more = classify(K, errp, th2, active, eidx, matches12);
        nin = ne - nbad - more;
        done = true;
    }
    if (tid == 0) {
        float* Ro = A.R12_opt + (size_t)b * 9;
        float* to = A.t12_opt + (size_t)b * 3;
        if (done) {
            lm::quat_to_matrix(cur.qx, cur.qy, cur.qz, cur.qw, R);
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) Ro[3 * r + c] = (float)R[r][c];
            to[0] = (float)cur.tx;
            to[1] = (float)cur.ty;
            to[2] = (float)cur.tz;
            A.s12_opt[b] = (float)cur.s;
        } else {  // return 0: g2oS12 is left at its input
            for (int k = 0; k < 9; k++) Ro[k] = Rin[k];
            for (int k = 0; k < 3; k++) to[k] = tin[k];
            A.s12_opt[b] = A.s12[b];
        }
        if (A.ninliers) A.ninliers[b] = nin;
        if (A.ncorr) A.ncorr[b] = ne;
        if (A.nbad) A.nbad[b] = nbad;
        if (trace) {
            trace[0] = its[0];
            trace[1] = trials[0];
            trace[2] = its[1];
            trace[3] = trials[1];
        }
    }
}

}  // namespace

size_t opt_sim3_workspace_bytes(int batch, int cap1) {
    return (size_t)batch * cap1 * (kOsRecWords + 2) * 4;
}

hipError_t launch_opt_sim3(OptSim3Args A, int batch, char* workspace, hipStream_t stream) {
    if (batch <= 0) return hipSuccess;
    const size_t rows = (size_t)batch * A.cap1;
    A.rec = (float*)workspace;
    A.eidx = (int32_t*)(workspace + rows * kOsRecWords * 4);
    A.active = A.eidx + rows;
    s3_probe_increments(A.fix_scale != 0, A.probes);
    k_opt_sim3<<<batch, kOsThreads, 0, stream>>>(A);
    return hipGetLastError();
}

}  // namespace orbx
