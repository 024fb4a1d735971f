// orbx_sim3.hip -- device Sim3Solver: Horn's closed form under RANSAC for a batch of loop
// candidates in HBM.
//
// Reference: include/Sim3Solver.h, src/Sim3Solver.cc:37-534 (constructor 37-129,
// SetRansacParameters 132-185, iterate 188-274, find 277-281, ComputeSim3 298-437,
// CheckInliers 440-468, Project 488-512, FromCameraToImage 515-534), as driven by
// LoopClosing::ComputeSim3 (LoopClosing.cc:243-377).  DESIGN.md §4.16.
//
// Three kernels per solver:
//   k_sim3_setup   one workgroup per candidate: the constructor.  Slots whose two MapPoint ids
//                  are valid are compacted in slot order (ballot + wave counts: the order is
//                  mvnIndices1), their camera coordinates, own projections and truncated
//                  thresholds go to the workspace as structure-of-arrays, and the iteration
//                  cap is looked up in the host's table at N.
//   k_sim3_score   one wave per (candidate, iteration of this call): every lane solves Horn for
//                  the iteration's three pairs (the same instructions on the same data, so the
//                  control flow is uniform), then the lanes stride over the N pairs and count
//                  the inliers with ballot + popcount.  One count per (candidate, iteration).
//   k_sim3_select  one workgroup per candidate: one thread walks the call's counts in order and
//                  applies the stopping rule of cc:212-273; the workgroup recomputes the flags
//                  of the returned iteration with the scoring code and scatters them through
//                  mvnIndices1, writes the outputs and the persistent state.
//
// Float inputs are widened to double; everything after is double under -ffp-contract=off;
// outputs are rounded to float once.  There are no floating-point sums across lanes: a
// candidate's bytes depend neither on the batch around it nor on how its iterations are cut
// into calls.  The host reads nothing back between setup and the end of a call.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "orbx.h"
#include "orbx_host.h"

namespace orbx {


constexpr int kSim3Threads = 256;
constexpr int kSim3Waves = kSim3Threads / 64;
constexpr int kSim3State = 8;  // ints per candidate
enum { kStN = 0, kStMaxIts, kStIterations, kStBestInliers, kStBestIteration, kStStatus, kStN1 };
constexpr int kSim3Planes = 10;  // doubles per pair: X3Dc1 xyz, X3Dc2 xyz, P1im1 uv, P2im2 uv

struct Sim3Work {
    double* pts;      // [B][10][cap]
    float* thr;       // [B][2][cap]  mvnMaxError1 / 2 as the float they are compared as
    int32_t* idx;     // [B][cap]     mvnIndices1
    int32_t* state;   // [B][8]
    int32_t* counts;  // [B][max_iterations] of the running call; -1: a draw out of range
    int cap, max_iterations;
};

struct Sim3SetupArgs {
    const int32_t* n1;    // [B]
    const int32_t* mp1;   // [B][cap]
    const int32_t* mp2;
    const int32_t* oct1;
    const int32_t* oct2;
    const float* pos;     // [n_mp][3]
    int n_mp;
    const float* Tcw1;    // [B][12]
    const float* Tcw2;
    float K1[4], K2[4];
    float thr[ORBX_MAX_LEVELS];
    int nlevels, cap, min_inliers;
    const int32_t* its;   // [cap + 1] mRansacMaxIts by N
    Sim3Work W;
};

struct Sim3RunArgs {
    Sim3Work W;
    const int32_t* draws;  // [B][draw_stride][3]
    int draw_stride;
    float K1[4], K2[4];
    int fix_scale, min_inliers, n_iterations, out_cap;
    orbx_sim3_result out;
};

struct Sim3Hyp {
    double R[9], t[3], s;
    double T12[12], T21[12];  // rows 0..2 of [sR | t] and of [(1/s)R^T | -(1/s)R^T t]
};

// Rcw * X + tcw: ((r0 x + r1 y) + r2 z) + t
__device__ __forceinline__ void transform(const double* T, double x, double y, double z, double* o) {
#pragma unroll
    for (int r = 0; r < 3; r++) o[r] = ((T[4 * r] * x + T[4 * r + 1] * y) + T[4 * r + 2] * z) + T[4 * r + 3];
}

// FromCameraToImage / the tail of Project (cc:506-510, 527-532): no depth check
__device__ __forceinline__ void to_image(const double* X, const float* K, double* u, double* v) {
    const double invz = 1.0 / X[2];
    *u = (double)K[0] * (X[0] * invz) + (double)K[2];
    *v = (double)K[1] * (X[1] * invz) + (double)K[3];
}

__global__ __launch_bounds__(kSim3Threads) void k_sim3_setup(Sim3SetupArgs A) {
    __shared__ int s_cnt[kSim3Waves];
    __shared__ double s_T[24];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cap = A.cap;
    int n1 = A.n1[b];
    n1 = n1 < 0 ? 0 : (n1 > cap ? cap : n1);
    if (tid < 12) s_T[tid] = (double)A.Tcw1[(size_t)b * 12 + tid];
    else if (tid < 24) s_T[tid] = (double)A.Tcw2[(size_t)b * 12 + tid - 12];
    const size_t row = (size_t)b * cap;
    double* pts = A.W.pts + (size_t)b * kSim3Planes * A.W.cap;
    float* thr = A.W.thr + (size_t)b * 2 * A.W.cap;
    int32_t* idx = A.W.idx + (size_t)b * A.W.cap;
    const int wcap = A.W.cap;
    int total = 0;
    __syncthreads();
    for (int base = 0; base < n1; base += kSim3Threads) {
        const int i = base + tid;
        int a = -1, c = -1;
        if (i < n1) {
            a = A.mp1[row + i];
            c = A.mp2[row + i];
        }
        const bool keep = a >= 0 && a < A.n_mp && c >= 0 && c < A.n_mp;  // cc:70-87 through the caller's ids
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_cnt[wave] = __popcll(m);
        __syncthreads();
        int off = total;
        for (int w = 0; w < wave; w++) off += s_cnt[w];
        int all = 0;
        for (int w = 0; w < kSim3Waves; w++) all += s_cnt[w];
        if (keep) {
            const int e = off + __popcll(m & ((1ull << lane) - 1ull));  // e <= i < cap
            int o1 = A.oct1[row + i], o2 = A.oct2[row + i];
            o1 = o1 < 0 ? 0 : (o1 >= A.nlevels ? A.nlevels - 1 : o1);
            o2 = o2 < 0 ? 0 : (o2 >= A.nlevels ? A.nlevels - 1 : o2);
            const float* p1 = A.pos + (size_t)a * 3;
            const float* p2 = A.pos + (size_t)c * 3;
            double X1[3], X2[3], u, v;
            transform(s_T, (double)p1[0], (double)p1[1], (double)p1[2], X1);       // cc:107-108
            transform(s_T + 12, (double)p2[0], (double)p2[1], (double)p2[2], X2);  // cc:110-111
#pragma unroll
            for (int k = 0; k < 3; k++) {
                pts[(size_t)k * wcap + e] = X1[k];
                pts[(size_t)(3 + k) * wcap + e] = X2[k];
            }
            to_image(X1, A.K1, &u, &v);  // cc:124
            pts[(size_t)6 * wcap + e] = u;
            pts[(size_t)7 * wcap + e] = v;
            to_image(X2, A.K2, &u, &v);  // cc:125
            pts[(size_t)8 * wcap + e] = u;
            pts[(size_t)9 * wcap + e] = v;
            thr[e] = A.thr[o1];          // cc:98-99
            thr[wcap + e] = A.thr[o2];
            idx[e] = i;                  // cc:104
        }
        total += all;
        __syncthreads();
    }
    if (tid == 0) {
        int32_t* st = A.W.state + (size_t)b * kSim3State;
        st[kStN] = total;
        st[kStMaxIts] = A.its[total];  // total <= n1 <= cap
        st[kStIterations] = 0;         // cc:184
        st[kStBestInliers] = 0;        // cc:38
        st[kStBestIteration] = -1;
        st[kStStatus] = 0;
        st[kStN1] = n1;
        st[7] = 0;
    }
}

// The eigenvector of the largest eigenvalue of the symmetric 4x4 a (destroyed): cyclic Jacobi,
// a rotation skipped where a_pq is exactly 0, at most 30 sweeps, stops when the off-diagonal
// is exactly 0.  Ties between eigenvalues go to the first.
__device__ void jacobi4(double a[4][4], double q[4]) {
    double v[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; sweep++) {
        double off = 0.0;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int r = p + 1; r < 4; r++) off = off + fabs(a[p][r]);
        if (!(off > 0.0)) break;  // 0, or NaN
#pragma unroll
        for (int p = 0; p < 3; p++) {
#pragma unroll
            for (int r = p + 1; r < 4; r++) {
                const double apq = a[p][r];
                if (apq == 0.0) continue;
                const double theta = (a[r][r] - a[p][p]) / (2.0 * apq);
                double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                if (theta < 0.0) t = -t;
                const double c = 1.0 / sqrt(t * t + 1.0);
                const double s = t * c;
#pragma unroll
                for (int k = 0; k < 4; k++) {  // A <- A J
                    const double akp = a[k][p], akq = a[k][r];
                    a[k][p] = c * akp - s * akq;
                    a[k][r] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {  // A <- J^T A
                    const double apk = a[p][k], aqk = a[r][k];
                    a[p][k] = c * apk - s * aqk;
                    a[r][k] = s * apk + c * aqk;
                }
                a[p][r] = 0.0;
                a[r][p] = 0.0;
#pragma unroll
                for (int k = 0; k < 4; k++) {  // V <- V J
                    const double vkp = v[k][p], vkq = v[k][r];
                    v[k][p] = c * vkp - s * vkq;
                    v[k][r] = s * vkp + c * vkq;
                }
            }
        }
    }
    double best = a[0][0];
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = v[k][0];
#pragma unroll
    for (int j = 1; j < 4; j++)
        if (a[j][j] > best) {
            best = a[j][j];
#pragma unroll
            for (int k = 0; k < 4; k++) q[k] = v[k][j];
        }
}

__device__ void nan_hypothesis(Sim3Hyp& h) {
    const double n = __builtin_nan("");
    for (int i = 0; i < 9; i++) h.R[i] = n;
    for (int i = 0; i < 3; i++) h.t[i] = n;
    h.s = n;
    for (int i = 0; i < 12; i++) h.T12[i] = h.T21[i] = n;
}

// Sim3Solver::ComputeSim3 (cc:298-437) on three pairs: P1[k], P2[k] are point k in camera 1 / 2.
__device__ void horn(const double P1[3][3], const double P2[3][3], int fix_scale, Sim3Hyp& h) {
    double O1[3], O2[3], Pr1[3][3], Pr2[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++) {  // cc:284-294
        O1[i] = ((P1[0][i] + P1[1][i]) + P1[2][i]) / 3.0;
        O2[i] = ((P2[0][i] + P2[1][i]) + P2[2][i]) / 3.0;
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int i = 0; i < 3; i++) {
            Pr1[k][i] = P1[k][i] - O1[i];
            Pr2[k][i] = P2[k][i] - O2[i];
        }
    double M[3][3];  // cc:318 M = Pr2 * Pr1^T
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            M[i][j] = (Pr2[0][i] * Pr1[0][j] + Pr2[1][i] * Pr1[1][j]) + Pr2[2][i] * Pr1[2][j];
    double N[4][4];  // cc:326-340
    N[0][0] = (M[0][0] + M[1][1]) + M[2][2];
    N[0][1] = M[1][2] - M[2][1];
    N[0][2] = M[2][0] - M[0][2];
    N[0][3] = M[0][1] - M[1][0];
    N[1][1] = (M[0][0] - M[1][1]) - M[2][2];
    N[1][2] = M[0][1] + M[1][0];
    N[1][3] = M[2][0] + M[0][2];
    N[2][2] = (-M[0][0] + M[1][1]) - M[2][2];
    N[2][3] = M[1][2] + M[2][1];
    N[3][3] = (-M[0][0] - M[1][1]) + M[2][2];
    N[1][0] = N[0][1];
    N[2][0] = N[0][2];
    N[3][0] = N[0][3];
    N[2][1] = N[1][2];
    N[3][1] = N[1][3];
    N[3][2] = N[2][3];
    double q[4];
    jacobi4(N, q);  // cc:347
    const double nv = sqrt((q[1] * q[1] + q[2] * q[2]) + q[3] * q[3]);  // cc:368
    const double ang = atan2(nv, q[0]);
    double rv[3];
#pragma unroll
    for (int i = 0; i < 3; i++) rv[i] = (2.0 * ang * q[1 + i]) / nv;    // cc:371: 0/0 when |v| is 0
    // cv::Rodrigues (cc:375)
    const double theta = sqrt((rv[0] * rv[0] + rv[1] * rv[1]) + rv[2] * rv[2]);
    double* R = h.R;
    if (theta < 2.220446049250313e-16) {
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    } else {
        const double c = cos(theta), s = sin(theta), c1 = 1.0 - c, it = 1.0 / theta;
        const double rx = rv[0] * it, ry = rv[1] * it, rz = rv[2] * it;
        const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
        const double r_x[9] = {0.0, -rz, ry, rz, 0.0, -rx, -ry, rx, 0.0};
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = (c * ((i % 4 == 0) ? 1.0 : 0.0) + c1 * rrt[i]) + s * r_x[i];
    }
    double P3[3][3];  // cc:379
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int i = 0; i < 3; i++)
            P3[k][i] = (R[3 * i] * Pr2[k][0] + R[3 * i + 1] * Pr2[k][1]) + R[3 * i + 2] * Pr2[k][2];
    double sc = 1.0;  // cc:383-407
    if (!fix_scale) {
        double nom = 0.0, den = 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int k = 0; k < 3; k++) {
                nom = nom + Pr1[k][i] * P3[k][i];
                den = den + P3[k][i] * P3[k][i];
            }
        sc = nom / den;
    }
    h.s = sc;
    const double inv = 1.0 / sc;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            h.T12[4 * i + j] = sc * R[3 * i + j];   // cc:421
            h.T21[4 * i + j] = inv * R[3 * j + i];  // cc:432
        }
        h.t[i] = O1[i] - ((h.T12[4 * i] * O2[0] + h.T12[4 * i + 1] * O2[1]) + h.T12[4 * i + 2] * O2[2]);  // cc:413
        h.T12[4 * i + 3] = h.t[i];
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
        h.T21[4 * i + 3] = -((h.T21[4 * i] * h.t[0] + h.T21[4 * i + 1] * h.t[1]) + h.T21[4 * i + 2] * h.t[2]);  // cc:435
}

// Iteration k's hypothesis of candidate b (cc:217-241).  False, and NaN everywhere, when a draw
// lies outside [0, N - j).
__device__ bool hypothesis(const Sim3RunArgs& A, int b, int N, int k, Sim3Hyp& h) {
    const int32_t* d = A.draws + ((size_t)b * A.draw_stride + k) * 3;
    const int r0 = d[0], r1 = d[1], r2 = d[2];
    if (r0 < 0 || r0 >= N || r1 < 0 || r1 >= N - 1 || r2 < 0 || r2 >= N - 2) {
        nan_hypothesis(h);
        return false;
    }
    // vAvailableIndices after one and two swap-with-back removals, in closed form
    const int i0 = r0;
    const int i1 = r1 == r0 ? N - 1 : r1;
    const int back = (N - 2) == r0 ? N - 1 : N - 2;
    const int i2 = r2 == r1 ? back : (r2 == r0 ? N - 1 : r2);
    const int id[3] = {i0, i1, i2};
    const double* pts = A.W.pts + (size_t)b * kSim3Planes * A.W.cap;
    double P1[3][3], P2[3][3];
#pragma unroll
    for (int p = 0; p < 3; p++)
#pragma unroll
        for (int a = 0; a < 3; a++) {
            P1[p][a] = pts[(size_t)a * A.W.cap + id[p]];
            P2[p][a] = pts[(size_t)(3 + a) * A.W.cap + id[p]];
        }
    horn(P1, P2, A.fix_scale, h);
    return true;
}

// CheckInliers for pair i (cc:443-466): both reprojection errors under their thresholds, strictly
__device__ __forceinline__ bool pair_inlier(const Sim3RunArgs& A, const double* pts, const float* thr, int i,
                                            const Sim3Hyp& h) {
    const size_t c = (size_t)A.W.cap;
    double X[3], u, v;
    transform(h.T12, pts[3 * c + i], pts[4 * c + i], pts[5 * c + i], X);  // vP2im1
    to_image(X, A.K1, &u, &v);
    const double d1x = pts[6 * c + i] - u, d1y = pts[7 * c + i] - v;
    transform(h.T21, pts[i], pts[c + i], pts[2 * c + i], X);              // vP1im2
    to_image(X, A.K2, &u, &v);
    const double d2x = u - pts[8 * c + i], d2y = v - pts[9 * c + i];
    const double e1 = d1x * d1x + d1y * d1y, e2 = d2x * d2x + d2y * d2y;
    return e1 < (double)thr[i] && e2 < (double)thr[c + i];
}

__device__ __forceinline__ bool runnable(int N, int min_inliers) { return N >= min_inliers && N >= 3; }  // cc:195

__global__ __launch_bounds__(kSim3Threads) void k_sim3_score(Sim3RunArgs A) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int j = blockIdx.x * kSim3Waves + (threadIdx.x >> 6);
    if (j >= A.n_iterations) return;
    const int32_t* st = A.W.state + (size_t)b * kSim3State;
    const int N = st[kStN];
    if (!runnable(N, A.min_inliers)) return;
    const int k = st[kStIterations] + j;
    if (k >= st[kStMaxIts]) return;  // cc:212
    Sim3Hyp h;
    const bool ok = hypothesis(A, b, N, k, h);
    const double* pts = A.W.pts + (size_t)b * kSim3Planes * A.W.cap;
    const float* thr = A.W.thr + (size_t)b * 2 * A.W.cap;
    int count = 0;
    for (int base = 0; base < N; base += 64) {
        const int i = base + lane;
        const bool in = i < N && pair_inlier(A, pts, thr, i, h);
        count += __popcll(__ballot(in));
    }
    if (lane == 0) A.W.counts[(size_t)b * A.W.max_iterations + j] = ok ? count : -1;
}

__global__ __launch_bounds__(kSim3Threads) void k_sim3_select(Sim3RunArgs A) {
    extern __shared__ int s_counts[];
    __shared__ int s_res[8];  // found, returned iteration, its count, iterations, best count, best iteration, status, no_more
    const int b = blockIdx.x, tid = threadIdx.x;
    int32_t* st = A.W.state + (size_t)b * kSim3State;
    const int N = st[kStN], max_its = st[kStMaxIts], it0 = st[kStIterations], n1 = st[kStN1];
    const bool run = runnable(N, A.min_inliers);
    int avail = max_its - it0;  // iterations the scoring kernel wrote
    avail = !run || avail < 0 ? 0 : (avail > A.n_iterations ? A.n_iterations : avail);
    for (int j = tid; j < avail; j += kSim3Threads) s_counts[j] = A.W.counts[(size_t)b * A.W.max_iterations + j];
    __syncthreads();
    if (tid == 0) {
        int found = 0, ret = -1, ret_count = 0, it = it0, best = st[kStBestInliers], best_it = st[kStBestIteration],
            status = st[kStStatus], no_more = 0;
        if (!run) {
            no_more = 1;  // cc:195-199
        } else {
            for (int j = 0; j < avail; j++) {  // cc:212-267
                const int k = it++;
                int inl = s_counts[j];
                if (inl < 0) {
                    status |= ORBX_SIM3_STATUS_BAD_DRAW;
                    inl = 0;
                }
                if (inl >= best) {             // cc:247: a tie goes to the later iteration
                    best = inl;
                    best_it = k;
                    if (inl > A.min_inliers) {  // cc:256
                        found = 1;
                        ret = k;  // == best_it
                        ret_count = inl;
                        break;
                    }
                }
            }
            if (!found && it >= max_its) no_more = 1;  // cc:270
        }
        s_res[0] = found;
        s_res[1] = ret;
        s_res[2] = ret_count;
        s_res[3] = it;
        s_res[4] = best;
        s_res[5] = best_it;
        s_res[6] = status;
        s_res[7] = no_more;
    }
    __syncthreads();
    const int found = s_res[0], best_it = s_res[5];
    const orbx_sim3_result& o = A.out;
    if (o.inliers)
        for (int i = tid; i < n1; i += kSim3Threads) o.inliers[(size_t)b * A.out_cap + i] = 0;  // cc:191
    __syncthreads();
    Sim3Hyp h;
    if (best_it >= 0) hypothesis(A, b, N, best_it, h);  // the returned iteration is the best one (cc:249-264)
    else nan_hypothesis(h);
    if (found && o.inliers) {
        const double* pts = A.W.pts + (size_t)b * kSim3Planes * A.W.cap;
        const float* thr = A.W.thr + (size_t)b * 2 * A.W.cap;
        const int32_t* idx = A.W.idx + (size_t)b * A.W.cap;
        for (int i = tid; i < N; i += kSim3Threads)
            if (pair_inlier(A, pts, thr, i, h)) o.inliers[(size_t)b * A.out_cap + idx[i]] = 1;  // cc:260-263
    }
    if (tid == 0) {
        if (o.found) o.found[b] = found;
        if (o.no_more) o.no_more[b] = s_res[7];
        if (o.n_inliers) o.n_inliers[b] = s_res[2];
        if (o.T12) {
            float* T = o.T12 + (size_t)b * 16;
            for (int i = 0; i < 12; i++) T[i] = found ? (float)h.T12[i] : 0.0f;
            T[12] = T[13] = T[14] = 0.0f;
            T[15] = found ? 1.0f : 0.0f;
        }
        if (o.best_R)
            for (int i = 0; i < 9; i++) o.best_R[(size_t)b * 9 + i] = (float)h.R[i];
        if (o.best_t)
            for (int i = 0; i < 3; i++) o.best_t[(size_t)b * 3 + i] = (float)h.t[i];
        if (o.best_s) o.best_s[b] = (float)h.s;
        if (o.best_inliers) o.best_inliers[b] = s_res[4];
        if (o.best_iteration) o.best_iteration[b] = best_it;
        if (o.iterations) o.iterations[b] = s_res[3];
        if (o.n_pairs) o.n_pairs[b] = N;
        if (o.status) o.status[b] = s_res[6];
        st[kStIterations] = s_res[3];
        st[kStBestInliers] = s_res[4];
        st[kStBestIteration] = best_it;
        st[kStStatus] = s_res[6];
    }
}

}  // namespace orbx

// ---------------------------------------------------------------------------------------
// Host side

struct orbx_sim3 {
    orbx_matcher* matcher = nullptr;
    int device = 0, max_batch = 0, cap = 0, max_iterations = 0;
    hipStream_t stream = nullptr;  // the matcher's
    char* work = nullptr;          // Sim3Work arrays
    int32_t* its = nullptr;        // [cap + 1]
    orbx::DeviceBuffer stage;      // the single host form's candidate and results
    orbx::Sim3Work W{};
    std::vector<int32_t> h_its;
    // the batch in force (set): what iterate needs
    bool is_set = false;
    int batch = 0, batch_cap = 0, draw_stride = 0, fix_scale = 0, min_inliers = 0;
    float K1[4] = {}, K2[4] = {};
    const int32_t* draws = nullptr;
    // the single host form's candidate (set): its result block, the device addresses in it,
    // and iterate's destinations
    orbx::HostStage host{orbx::up256};
    orbx_sim3_result host_dev{}, host_out{};
};

namespace {

using namespace orbx;

// SetRansacParameters (cc:145-181) for N = n, with the host's libm
int ransac_iterations(int n, int min_inliers, double probability, int max_iterations) {
    if (n < min_inliers || n <= 0) return 1;  // never used: iterate answers "no more" first
    int its;
    if (min_inliers == n) {
        its = 1;
    } else {
        const float epsilon = (float)min_inliers / n;
        const double v = std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3.0));
        its = !(v <= (double)max_iterations) ? max_iterations : (int)std::ceil(v);
    }
    return std::max(1, std::min(its, max_iterations));
}

// the argument checks of orbx_sim3_set_batch_device and orbx_sim3_set, before any GPU work
int check_batch(const orbx_sim3* s, const orbx_sim3_batch* in) {
    const int B = in->batch, cap = in->cap;
    if (B < 0 || B > s->max_batch || cap < 1 || cap > s->cap || in->n_mp < 0 || in->nlevels < 1 ||
        in->nlevels > ORBX_MAX_LEVELS || in->min_inliers < 0 || in->max_iterations < 1 ||
        in->max_iterations > s->max_iterations || !(in->probability > 0.0 && in->probability < 1.0))
        return fail(ORBX_ERR_ARG, "bad argument");
    if (!in->level_sigma2 || !in->K1 || !in->K2) return fail(ORBX_ERR_ARG, "null host array");
    if (B > 0 && (!in->n1 || !in->mp1 || !in->mp2 || !in->oct1 || !in->oct2 || !in->Tcw1 || !in->Tcw2 || !in->draws ||
                  (in->n_mp > 0 && !in->mp_pos)))
        return fail(ORBX_ERR_ARG, "null buffer");
    for (int l = 0; l < in->nlevels; l++)
        if (!(in->level_sigma2[l] >= 0.0f) || 9.210 * (double)in->level_sigma2[l] >= 16777216.0)
            return fail(ORBX_ERR_ARG, "level_sigma2 outside [0, 2^24 / 9.21)");
    return ORBX_OK;
}

}  // namespace

extern "C" {

int orbx_sim3_create(orbx_matcher* m, int max_batch, int cap, int max_iterations, orbx_sim3** out) {
    if (!out) return fail(ORBX_ERR_ARG, "null argument");
    *out = nullptr;
    if (!m) return fail(ORBX_ERR_ARG, "null matcher");
    if (max_batch < 1 || cap < 1 || max_iterations < 1 || max_iterations > ORBX_SIM3_MAX_ITERATIONS)
        return fail(ORBX_ERR_ARG, "bad argument");
    if ((size_t)max_batch * (size_t)cap >= ((size_t)1 << 31) ||
        (size_t)max_batch * (size_t)max_iterations >= ((size_t)1 << 31))
        return fail(ORBX_ERR_ARG, "max_batch x cap or x max_iterations of 2^31 or more");
    orbx_sim3* s = new (std::nothrow) orbx_sim3();
    if (!s) return fail(ORBX_ERR_ARG, "out of host memory");
    s->matcher = m;
    s->device = matcher_device(m);
    s->stream = matcher_stream(m);
    s->max_batch = max_batch;
    s->cap = cap;
    s->max_iterations = max_iterations;
    const size_t slots = (size_t)max_batch * cap;
    Layout L(up256);
    const size_t o_pts = L.take(slots * kSim3Planes * 8), o_thr = L.take(slots * 2 * 4), o_idx = L.take(slots * 4),
                 o_state = L.take((size_t)max_batch * kSim3State * 4),
                 o_counts = L.take((size_t)max_batch * max_iterations * 4);
    hipError_t e = hipSetDevice(s->device);
    if (e == hipSuccess) e = hipMalloc((void**)&s->work, L.total());
    if (e == hipSuccess) e = hipMalloc((void**)&s->its, ((size_t)cap + 1) * 4);
    if (e != hipSuccess) {
        if (s->work) (void)hipFree(s->work);
        if (s->its) (void)hipFree(s->its);
        delete s;
        set_last_error(std::string("orbx_sim3_create: ") + hipGetErrorString(e));
        return ORBX_ERR_HIP;
    }
    s->W.pts = (double*)(s->work + o_pts);
    s->W.thr = (float*)(s->work + o_thr);
    s->W.idx = (int32_t*)(s->work + o_idx);
    s->W.state = (int32_t*)(s->work + o_state);
    s->W.counts = (int32_t*)(s->work + o_counts);
    s->W.cap = cap;
    s->W.max_iterations = max_iterations;
    *out = s;
    return ORBX_OK;
}

void orbx_sim3_destroy(orbx_sim3* s) {
    if (!s || orbx::unloading()) return;  // DESIGN.md §1 "Teardown"
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    if (s->work) (void)hipFree(s->work);
    if (s->its) (void)hipFree(s->its);
    s->stage.release();
    delete s;
}

int orbx_sim3_set_batch_device(orbx_sim3* s, const orbx_sim3_batch* in, void* stream) {
    if (!s || !in) return fail(ORBX_ERR_ARG, "null argument");
    int rc = check_batch(s, in);
    if (rc) return rc;
    const int B = in->batch, cap = in->cap;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = stream ? (hipStream_t)stream : s->stream;
    s->is_set = false;
    s->host = HostStage(up256);
    if (B == 0) {
        s->batch = 0;
        s->is_set = true;
        return ORBX_OK;
    }
    Sim3SetupArgs A{};
    A.n1 = in->n1;
    A.mp1 = in->mp1;
    A.mp2 = in->mp2;
    A.oct1 = in->oct1;
    A.oct2 = in->oct2;
    A.pos = in->mp_pos;
    A.n_mp = in->n_mp;
    A.Tcw1 = in->Tcw1;
    A.Tcw2 = in->Tcw2;
    for (int i = 0; i < 4; i++) {
        A.K1[i] = s->K1[i] = in->K1[i];
        A.K2[i] = s->K2[i] = in->K2[i];
    }
    // mvnMaxError is a std::vector<size_t> (Sim3Solver.h:143-144): the double product truncated
    for (int l = 0; l < in->nlevels; l++) A.thr[l] = (float)(size_t)(9.210 * (double)in->level_sigma2[l]);
    A.nlevels = in->nlevels;
    A.cap = cap;
    A.min_inliers = in->min_inliers;
    s->h_its.resize((size_t)cap + 1);
    for (int n = 0; n <= cap; n++)
        s->h_its[n] = ransac_iterations(n, in->min_inliers, in->probability, in->max_iterations);
    HIP_TRY(hipMemcpyAsync(s->its, s->h_its.data(), ((size_t)cap + 1) * 4, hipMemcpyHostToDevice, st));
    A.its = s->its;
    A.W = s->W;
    k_sim3_setup<<<B, kSim3Threads, 0, st>>>(A);
    HIP_TRY(hipGetLastError());
    s->batch = B;
    s->batch_cap = cap;
    s->draw_stride = in->max_iterations;
    s->fix_scale = in->fix_scale ? 1 : 0;
    s->min_inliers = in->min_inliers;
    s->draws = in->draws;
    s->is_set = true;
    return ORBX_OK;
}

int orbx_sim3_iterate_device(orbx_sim3* s, int n_iterations, const orbx_sim3_result* out, void* stream) {
    if (!s || !out || n_iterations < 0) return fail(ORBX_ERR_ARG, "bad argument");
    if (!s->is_set) return fail(ORBX_ERR_STATE, "orbx_sim3_iterate before orbx_sim3_set");
    if (s->batch == 0) return ORBX_OK;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = stream ? (hipStream_t)stream : s->stream;
    Sim3RunArgs A{};
    A.W = s->W;
    A.draws = s->draws;
    A.draw_stride = s->draw_stride;
    for (int i = 0; i < 4; i++) {
        A.K1[i] = s->K1[i];
        A.K2[i] = s->K2[i];
    }
    A.fix_scale = s->fix_scale;
    A.min_inliers = s->min_inliers;
    A.n_iterations = n_iterations < s->draw_stride ? n_iterations : s->draw_stride;  // the cap is at most that
    A.out_cap = s->batch_cap;
    A.out = *out;
    if (A.n_iterations > 0) {
        dim3 grid((unsigned)((A.n_iterations + kSim3Waves - 1) / kSim3Waves), (unsigned)s->batch);
        k_sim3_score<<<grid, kSim3Threads, 0, st>>>(A);
        HIP_TRY(hipGetLastError());
    }
    k_sim3_select<<<s->batch, kSim3Threads, (size_t)(A.n_iterations > 0 ? A.n_iterations : 1) * 4, st>>>(A);
    HIP_TRY(hipGetLastError());
    return ORBX_OK;
}

int orbx_sim3_set(orbx_sim3* s, const orbx_sim3_batch* in) {
    if (!s || !in) return fail(ORBX_ERR_ARG, "null argument");
    if (in->batch != 1) return fail(ORBX_ERR_ARG, "the host form takes one candidate");
    int rc = check_batch(s, in);
    if (rc) return rc;
    const int cap = in->cap;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    int n1 = in->n1[0];
    n1 = n1 < 0 ? 0 : (n1 > cap ? cap : n1);
    const size_t N = (size_t)n1, C = (size_t)cap, its = (size_t)in->max_iterations;
    struct {
        float Tcw1[12], Tcw2[12];
    } T, *d_T = nullptr;
    std::memcpy(T.Tcw1, in->Tcw1, sizeof(T.Tcw1));
    std::memcpy(T.Tcw2, in->Tcw2, sizeof(T.Tcw2));
    orbx_sim3_batch d = *in;
    HostStage h(up256);
    h.in(&d.n1, in->n1, 1, 1);
    h.in(&d.mp1, in->mp1, N, C);
    h.in(&d.mp2, in->mp2, N, C);
    h.in(&d.oct1, in->oct1, N, C);
    h.in(&d.oct2, in->oct2, N, C);
    h.in(&d_T, &T, 1, 1);
    h.in(&d.mp_pos, in->mp_pos, 3 * (size_t)in->n_mp, 3 * (size_t)(in->n_mp > 0 ? in->n_mp : 1));
    h.in(&d.draws, in->draws, 3 * its, 3 * its);
    orbx_sim3_result& r = s->host_dev;
    const orbx_sim3_result& o = s->host_out;
    h.out(&r.found, &o.found, 1, 1);
    h.out(&r.no_more, &o.no_more, 1, 1);
    h.out(&r.n_inliers, &o.n_inliers, 1, 1);
    h.out(&r.best_inliers, &o.best_inliers, 1, 1);
    h.out(&r.best_iteration, &o.best_iteration, 1, 1);
    h.out(&r.iterations, &o.iterations, 1, 1);
    h.out(&r.n_pairs, &o.n_pairs, 1, 1);
    h.out(&r.status, &o.status, 1, 1);
    h.out(&r.T12, &o.T12, 16, 16);
    h.out(&r.best_R, &o.best_R, 9, 9);
    h.out(&r.best_t, &o.best_t, 3, 3);
    h.out(&r.best_s, &o.best_s, 1, 1);
    h.out(&r.inliers, &o.inliers, N, C);  // last: iterate downloads up to the n1 in use
    HIP_TRY(h.stage(s->stage, st));
    d.Tcw1 = d_T->Tcw1;
    d.Tcw2 = d_T->Tcw2;
    rc = orbx_sim3_set_batch_device(s, &d, st);
    if (rc) return rc;
    s->host = std::move(h);  // iterate reads the result entries only: they point into the handle
    return ORBX_OK;
}

int orbx_sim3_iterate(orbx_sim3* s, int n_iterations, const orbx_sim3_result* out) {
    if (!s || !out || n_iterations < 0) return fail(ORBX_ERR_ARG, "bad argument");
    if (!s->host.staged()) return fail(ORBX_ERR_STATE, "orbx_sim3_iterate before orbx_sim3_set");
    CallClock clock(s->matcher);
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    const int rc = orbx_sim3_iterate_device(s, n_iterations, &s->host_dev, st);
    if (rc) return rc;
    s->host_out = *out;
    HIP_TRY(s->host.download(st, s->host.results_in_use()));
    return ORBX_OK;
}

int orbx_sim3_draws(int32_t* draws, int n, int iterations) {
    if (!draws || n < 0 || iterations < 0) return fail(ORBX_ERR_ARG, "bad argument");
    for (int k = 0; k < iterations; k++)
        for (int j = 0; j < 3; j++) {
            const int d = n - j;  // RandomInt(0, vAvailableIndices.size() - 1), DUtils/Random.cpp:47-49
            draws[(size_t)k * 3 + j] = d > 0 ? (int)(((double)rand() / ((double)RAND_MAX + 1.0)) * d) : 0;
        }
    return ORBX_OK;
}

}  // extern "C"
