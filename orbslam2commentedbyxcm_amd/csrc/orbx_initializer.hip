// orbx_initializer.hip -- device Initializer: the H / F RANSAC and the two-view reconstruction
// of monocular initialisation for a batch of frame pairs in HBM.
//
// Reference: include/Initializer.h, src/Initializer.cc:64-1415 (Initialize 64-165,
// FindHomography 179-244, FindFundamental 257-309, ComputeH21 318-385, ComputeF21 394-440,
// CheckHomography 450-590, CheckFundamental 597-735, ReconstructF 749-890, ReconstructH
// 905-1097, Triangulate 1107-1125, Normalize 1138-1200, CheckRT 1215-1379, DecomposeE
// 1391-1415).  DESIGN.md §4.19.
//
// Six kernels per call:
//   k_init_normalize   one workgroup per pair: the means and mean absolute deviations of all
//                      n1 / n2 keypoints (a thread sums its slots i = tid, tid + 256, ... in
//                      that order, then a fixed halving tree over the 256 partial sums), the
//                      correspondences compacted in slot order (ballot + wave counts).
//   k_init_hyp<ROWS>   one lane per (pair, iteration), H (ROWS = 16) and F (ROWS = 8) as two
//                      grids of 32-lane workgroups: the lane builds the ROWS x 9 matrix A and
//                      V = I in LDS, element (r, c) of lane l at [(r * 9 + c) * 32 + l] (the
//                      lanes of an access are 8 bytes apart: no bank conflict), and runs the
//                      one-sided Jacobi below; F adds the 3x3 SVD and the rank-2 recomposition.
//                      H21i, H12i and F21i of every iteration go to the workspace.
//   k_init_score       one wave per (pair, model, iteration): the lanes stride over the N
//                      correspondences, a lane adds its terms in that order, and the 64 lane
//                      sums meet in a xor butterfly (32, 16, ..., 1).  Only the score is stored.
//   k_init_select      one workgroup per pair: one thread walks the scores (strict `>`, the
//                      earlier iteration keeps a tie), the workgroup recomputes the winners'
//                      flags with the scoring code, then one thread does the small algebra:
//                      RH, K^-1 H K or K^T F K, the 3x3 SVD, the 8 or 4 (R, t).
//   k_init_checkrt     one workgroup per (pair, motion hypothesis): CheckRT over the inliers,
//                      the count by ballot / popcount, the min(50, nGood - 1)-th smallest
//                      cosine by a rank count.  Only the count and the parallax are stored.
//   k_init_finish      one workgroup per pair: the selection rule, then CheckRT once more for
//                      the winner to write vP3D / vbTriangulated.
//
// Jacobi constants (the ones of orbx_jacobi4.h): a sweep visits the column pairs (p, q), p < q,
// in lexicographic order; a pair is rotated unless gamma == 0 or |gamma| <= 8 eps sqrt(alpha
// beta); the sweeps end with the first one that rotates nothing or after 30.  The null vector
// is the column of V under the smallest column norm (ties: the higher index).  The 3x3 SVD
// sorts the column norms descending (stable), u_j = b_j / w_j for j = 0, 1 and u_2 = u_0 x u_1
// with the sign of its projection on b_2, so that a vanishing third singular value (E, F)
// still has a unit vector.
//
// Float inputs are widened to double; everything after is double under -ffp-contract=off;
// outputs are rounded to float once.
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
#include "orbx_jacobi4.h"

namespace orbx {


constexpr int kInitThreads = 256;
constexpr int kInitWaves = kInitThreads / 64;
constexpr int kHypLanes = 32;   // hypotheses per workgroup of k_init_hyp
constexpr int kInitState = 8;   // ints per pair
enum { kIsN = 0, kIsN1, kIsNhyp, kIsModel, kIsNinl, kIsStatus, kIsRatioFail };
constexpr int kInitMats = 27;   // doubles per iteration: H21i, H12i, F21i
constexpr int kInitHyps = 8;
constexpr double kPi = 3.14159265358979323846;

struct InitWork {
    double* pts;      // [B][4][kcap] u1 v1 u2 v2 of correspondence e
    int32_t* idx1;    // [B][kcap]    its frame-1 keypoint
    double* norm;     // [B][8]       meanX1 meanY1 sX1 sY1 meanX2 meanY2 sX2 sY2
    int32_t* state;   // [B][8]
    double* mats;     // [B][its][27]
    int32_t* bad;     // [B][its]     1: a bad set
    double* scores;   // [B][2][its]
    uint8_t* inl;     // [B][kcap]    the chosen model's flags by correspondence
    double* hyp;      // [B][8][12]   R (row-major), t
    double* cosw;     // [B][8][kcap] cosParallax of the good points, +inf elsewhere
    int32_t* good;    // [B][8]
    double* par;      // [B][8]
    int kcap, max_iterations;
};

struct InitArgs {
    InitWork W;
    const int32_t* n1;
    const int32_t* n2;
    const orbx_keypoint* keys1;
    const orbx_keypoint* keys2;
    const int32_t* matches12;
    const int32_t* sets;
    int kcap, iterations;
    double fx, fy, cx, cy, sigma;
    orbx_initializer_result out;
};

// ---- small 3x3 algebra on row-major doubles, every index a compile-time constant ------------

__device__ __forceinline__ void mul3(const double* A, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

__device__ __forceinline__ double det3(const double* A) {
    return (A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6])) +
           A[2] * (A[3] * A[7] - A[4] * A[6]);
}

__device__ __forceinline__ void inv3(const double* A, double* I) {
    const double d = 1.0 / det3(A);
    I[0] = (A[4] * A[8] - A[5] * A[7]) * d;
    I[1] = (A[2] * A[7] - A[1] * A[8]) * d;
    I[2] = (A[1] * A[5] - A[2] * A[4]) * d;
    I[3] = (A[5] * A[6] - A[3] * A[8]) * d;
    I[4] = (A[0] * A[8] - A[2] * A[6]) * d;
    I[5] = (A[2] * A[3] - A[0] * A[5]) * d;
    I[6] = (A[3] * A[7] - A[4] * A[6]) * d;
    I[7] = (A[1] * A[6] - A[0] * A[7]) * d;
    I[8] = (A[0] * A[4] - A[1] * A[3]) * d;
}

// One Hestenes rotation of columns p, q of the 3x3 B and of V.
template <int P, int Q>
__device__ __forceinline__ bool rot3(double* B, double* V) {
    const double alpha = (B[P] * B[P] + B[3 + P] * B[3 + P]) + B[6 + P] * B[6 + P];
    const double beta = (B[Q] * B[Q] + B[3 + Q] * B[3 + Q]) + B[6 + Q] * B[6 + Q];
    const double gamma = (B[P] * B[Q] + B[3 + P] * B[3 + Q]) + B[6 + P] * B[6 + Q];
    if (gamma == 0.0 || fabs(gamma) <= kJacobiTol * sqrt(alpha * beta)) return false;
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t);
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
__device__ __forceinline__ void swap_cols3(double* B, double* V, double* w) {
    if (w[P] < w[Q]) {
        double x = w[P]; w[P] = w[Q]; w[Q] = x;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            x = B[3 * r + P]; B[3 * r + P] = B[3 * r + Q]; B[3 * r + Q] = x;
            x = V[3 * r + P]; V[3 * r + P] = V[3 * r + Q]; V[3 * r + Q] = x;
        }
    }
}

// A = U diag(w) V^T with w descending: B = A V (orthogonal columns), V, w.
__device__ __forceinline__ void svd3(const double* A, double* B, double* V, double* w) {
#pragma unroll
    for (int i = 0; i < 9; i++) {
        B[i] = A[i];
        V[i] = (i % 4 == 0) ? 1.0 : 0.0;
    }
    for (int sweep = 0; sweep < kSweepCap; sweep++) {
        bool rot = false;
        rot |= rot3<0, 1>(B, V);
        rot |= rot3<0, 2>(B, V);
        rot |= rot3<1, 2>(B, V);
        if (!rot) break;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) w[c] = sqrt((B[c] * B[c] + B[3 + c] * B[3 + c]) + B[6 + c] * B[6 + c]);
    swap_cols3<0, 1>(B, V, w);
    swap_cols3<1, 2>(B, V, w);
    swap_cols3<0, 1>(B, V, w);
}

// U of svd3's result: u_0, u_1 normalised columns of B, u_2 their cross product on b_2's side.
__device__ __forceinline__ void svd3_u(const double* B, const double* w, double* U) {
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
}

// ---- k_init_normalize -----------------------------------------------------------------------

// The sums of four per-thread values over the workgroup: a halving tree over the thread index.
__device__ __forceinline__ void block_sum4(double (*s)[kInitThreads], int tid, double& a, double& b, double& c,
                                           double& d) {
    __syncthreads();
    s[0][tid] = a;
    s[1][tid] = b;
    s[2][tid] = c;
    s[3][tid] = d;
    __syncthreads();
    for (int off = kInitThreads / 2; off > 0; off >>= 1) {
        if (tid < off) {
#pragma unroll
            for (int k = 0; k < 4; k++) s[k][tid] = s[k][tid] + s[k][tid + off];
        }
        __syncthreads();
    }
    a = s[0][0];
    b = s[1][0];
    c = s[2][0];
    d = s[3][0];
}

__device__ __forceinline__ int clamp_count(int n, int cap) { return n < 0 ? 0 : (n > cap ? cap : n); }

__global__ __launch_bounds__(kInitThreads) void k_init_normalize(InitArgs A) {
    __shared__ double s_red[4][kInitThreads];
    __shared__ int s_cnt[kInitWaves];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kcap = A.kcap, wcap = A.W.kcap;
    const int n1 = clamp_count(A.n1[b], kcap), n2 = clamp_count(A.n2[b], kcap);
    const orbx_keypoint* k1 = A.keys1 + (size_t)b * kcap;
    const orbx_keypoint* k2 = A.keys2 + (size_t)b * kcap;
    const int32_t* m12 = A.matches12 + (size_t)b * kcap;
    // Normalize (cc:1138-1200) of both frames, over all their keypoints
    double sx1 = 0.0, sy1 = 0.0, sx2 = 0.0, sy2 = 0.0;
    for (int i = tid; i < n1; i += kInitThreads) {
        sx1 = sx1 + (double)k1[i].x;
        sy1 = sy1 + (double)k1[i].y;
    }
    for (int i = tid; i < n2; i += kInitThreads) {
        sx2 = sx2 + (double)k2[i].x;
        sy2 = sy2 + (double)k2[i].y;
    }
    block_sum4(s_red, tid, sx1, sy1, sx2, sy2);
    const double mx1 = sx1 / (double)n1, my1 = sy1 / (double)n1, mx2 = sx2 / (double)n2, my2 = sy2 / (double)n2;
    double dx1 = 0.0, dy1 = 0.0, dx2 = 0.0, dy2 = 0.0;
    for (int i = tid; i < n1; i += kInitThreads) {
        dx1 = dx1 + fabs((double)k1[i].x - mx1);
        dy1 = dy1 + fabs((double)k1[i].y - my1);
    }
    for (int i = tid; i < n2; i += kInitThreads) {
        dx2 = dx2 + fabs((double)k2[i].x - mx2);
        dy2 = dy2 + fabs((double)k2[i].y - my2);
    }
    block_sum4(s_red, tid, dx1, dy1, dx2, dy2);
    if (tid == 0) {
        double* nm = A.W.norm + (size_t)b * 8;
        nm[0] = mx1;
        nm[1] = my1;
        nm[2] = 1.0 / (dx1 / (double)n1);
        nm[3] = 1.0 / (dy1 / (double)n1);
        nm[4] = mx2;
        nm[5] = my2;
        nm[6] = 1.0 / (dx2 / (double)n2);
        nm[7] = 1.0 / (dy2 / (double)n2);
    }
    // mvMatches12 (cc:77-85) in slot order
    double* pts = A.W.pts + (size_t)b * 4 * wcap;
    int32_t* idx1 = A.W.idx1 + (size_t)b * wcap;
    int total = 0;
    for (int base = 0; base < n1; base += kInitThreads) {
        const int i = base + tid;
        const int m = i < n1 ? m12[i] : -1;
        const bool keep = m >= 0 && m < n2;
        const unsigned long long bal = __ballot(keep);
        __syncthreads();
        if (lane == 0) s_cnt[wave] = __popcll(bal);
        __syncthreads();
        int off = total, all = 0;
        for (int w = 0; w < kInitWaves; w++) {
            if (w < wave) off += s_cnt[w];
            all += s_cnt[w];
        }
        if (keep) {
            const int e = off + __popcll(bal & ((1ull << lane) - 1ull));  // e <= i < kcap <= wcap
            pts[e] = (double)k1[i].x;
            pts[(size_t)wcap + e] = (double)k1[i].y;
            pts[(size_t)2 * wcap + e] = (double)k2[m].x;
            pts[(size_t)3 * wcap + e] = (double)k2[m].y;
            idx1[e] = i;
        }
        total += all;
    }
    if (tid == 0) {
        int32_t* st = A.W.state + (size_t)b * kInitState;
        st[kIsN] = total;
        st[kIsN1] = n1;
        st[kIsNhyp] = 0;
        st[kIsModel] = 1;
        st[kIsNinl] = 0;
        st[kIsStatus] = total < 8 ? ORBX_INIT_STATUS_TOO_FEW : 0;
        st[kIsRatioFail] = 0;
        st[7] = 0;
    }
}

// ---- k_init_hyp -----------------------------------------------------------------------------

// The right singular vector of the smallest singular value of this lane's ROWS x 9 matrix in
// LDS (destroyed), V after it.
template <int ROWS>
__device__ __forceinline__ void null_vector9(double* s, int lane, double* h) {
#define ORBX_AE(r, c) s[((r) * 9 + (c)) * kHypLanes + lane]
#define ORBX_VE(r, c) s[((ROWS * 9) + (r) * 9 + (c)) * kHypLanes + lane]
    for (int r = 0; r < 9; r++)
        for (int c = 0; c < 9; c++) ORBX_VE(r, c) = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kSweepCap; sweep++) {
        bool rot = false;
        for (int p = 0; p < 8; p++)
            for (int q = p + 1; q < 9; q++) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (int r = 0; r < ROWS; r++) {
                    const double x = ORBX_AE(r, p), y = ORBX_AE(r, q);
                    alpha = alpha + x * x;
                    beta = beta + y * y;
                    gamma = gamma + x * y;
                }
                if (gamma == 0.0 || fabs(gamma) <= kJacobiTol * sqrt(alpha * beta)) continue;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t);
                const double sn = c * t;
                for (int r = 0; r < ROWS; r++) {
                    const double x = ORBX_AE(r, p), y = ORBX_AE(r, q);
                    ORBX_AE(r, p) = c * x - sn * y;
                    ORBX_AE(r, q) = sn * x + c * y;
                }
                for (int r = 0; r < 9; r++) {
                    const double x = ORBX_VE(r, p), y = ORBX_VE(r, q);
                    ORBX_VE(r, p) = c * x - sn * y;
                    ORBX_VE(r, q) = sn * x + c * y;
                }
                rot = true;
            }
        if (!rot) break;
    }
    int bc = 0;
    double best = 0.0;
    for (int c = 0; c < 9; c++) {
        double n = 0.0;
        for (int r = 0; r < ROWS; r++) n = n + ORBX_AE(r, c) * ORBX_AE(r, c);
        if (c == 0 || n <= best) {
            best = n;
            bc = c;
        }
    }
#pragma unroll
    for (int r = 0; r < 9; r++) h[r] = ORBX_VE(r, bc);
#undef ORBX_VE
}

template <int ROWS>
__global__ __launch_bounds__(kHypLanes) void k_init_hyp(InitArgs A) {
    __shared__ double s[(ROWS * 9 + 81) * kHypLanes];
    const int b = blockIdx.y, lane = threadIdx.x;
    const int it = blockIdx.x * kHypLanes + lane;
    const int N = A.W.state[(size_t)b * kInitState + kIsN];
    if (it >= A.iterations || N < 8) return;
    const int wcap = A.W.kcap;
    const int32_t* set = A.sets + ((size_t)b * A.iterations + it) * 8;
    int id[8];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        id[j] = set[j];
        ok = ok && id[j] >= 0 && id[j] < N;
    }
#pragma unroll
    for (int j = 1; j < 8; j++)
#pragma unroll
        for (int k = 0; k < j; k++) ok = ok && id[j] != id[k];
    if (ROWS == 16) A.W.bad[(size_t)b * A.W.max_iterations + it] = ok ? 0 : 1;
    if (!ok) return;
    const double* nm = A.W.norm + (size_t)b * 8;
    const double mx1 = nm[0], my1 = nm[1], s1x = nm[2], s1y = nm[3], mx2 = nm[4], my2 = nm[5], s2x = nm[6], s2y = nm[7];
    const double* pts = A.W.pts + (size_t)b * 4 * wcap;
#pragma unroll
    for (int j = 0; j < 8; j++) {  // vPn1i, vPn2i (cc:1167-1186)
        const int e = id[j];
        const double u1 = (pts[e] - mx1) * s1x, v1 = (pts[(size_t)wcap + e] - my1) * s1y;
        const double u2 = (pts[(size_t)2 * wcap + e] - mx2) * s2x, v2 = (pts[(size_t)3 * wcap + e] - my2) * s2y;
        if (ROWS == 16) {  // cc:349-368
            ORBX_AE(2 * j, 0) = 0.0;
            ORBX_AE(2 * j, 1) = 0.0;
            ORBX_AE(2 * j, 2) = 0.0;
            ORBX_AE(2 * j, 3) = -u1;
            ORBX_AE(2 * j, 4) = -v1;
            ORBX_AE(2 * j, 5) = -1.0;
            ORBX_AE(2 * j, 6) = v2 * u1;
            ORBX_AE(2 * j, 7) = v2 * v1;
            ORBX_AE(2 * j, 8) = v2;
            ORBX_AE(2 * j + 1, 0) = u1;
            ORBX_AE(2 * j + 1, 1) = v1;
            ORBX_AE(2 * j + 1, 2) = 1.0;
            ORBX_AE(2 * j + 1, 3) = 0.0;
            ORBX_AE(2 * j + 1, 4) = 0.0;
            ORBX_AE(2 * j + 1, 5) = 0.0;
            ORBX_AE(2 * j + 1, 6) = -u2 * u1;
            ORBX_AE(2 * j + 1, 7) = -u2 * v1;
            ORBX_AE(2 * j + 1, 8) = -u2;
        } else {  // cc:413-421
            ORBX_AE(j, 0) = u2 * u1;
            ORBX_AE(j, 1) = u2 * v1;
            ORBX_AE(j, 2) = u2;
            ORBX_AE(j, 3) = v2 * u1;
            ORBX_AE(j, 4) = v2 * v1;
            ORBX_AE(j, 5) = v2;
            ORBX_AE(j, 6) = u1;
            ORBX_AE(j, 7) = v1;
            ORBX_AE(j, 8) = 1.0;
        }
    }
    double h[9];
    null_vector9<ROWS>(s, lane, h);
    const double T1[9] = {s1x, 0.0, -mx1 * s1x, 0.0, s1y, -my1 * s1y, 0.0, 0.0, 1.0};
    double* out = A.W.mats + ((size_t)b * A.W.max_iterations + it) * kInitMats;
    double tmp[9], M[9];
    if (ROWS == 16) {
        // T2^-1 of T2 = [s2x 0 -mx2 s2x; 0 s2y -my2 s2y; 0 0 1] in closed form
        const double T2i[9] = {1.0 / s2x, 0.0, (mx2 * s2x) / s2x, 0.0, 1.0 / s2y, (my2 * s2y) / s2y, 0.0, 0.0, 1.0};
        mul3(T2i, h, tmp);
        mul3(tmp, T1, M);  // H21i (cc:226)
        double Mi[9];
        inv3(M, Mi);       // H12i (cc:228)
#pragma unroll
        for (int i = 0; i < 9; i++) {
            out[i] = M[i];
            out[9 + i] = Mi[i];
        }
    } else {
        double Bm[9], V[9], w[3], Fn[9];
        svd3(h, Bm, V, w);  // cc:434-439: u diag(w0, w1, 0) vt = b_0 v_0^T + b_1 v_1^T
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) Fn[3 * i + j] = Bm[3 * i] * V[3 * j] + Bm[3 * i + 1] * V[3 * j + 1];
        const double T2t[9] = {s2x, 0.0, 0.0, 0.0, s2y, 0.0, -mx2 * s2x, -my2 * s2y, 1.0};
        mul3(T2t, Fn, tmp);
        mul3(tmp, T1, M);  // F21i (cc:297)
#pragma unroll
        for (int i = 0; i < 9; i++) out[18 + i] = M[i];
    }
}
#undef ORBX_AE

// ---- scoring --------------------------------------------------------------------------------

// CheckHomography's body for one correspondence (cc:529-584): the two score terms, the flag.
__device__ __forceinline__ double score_h(const double* H, const double* Hi, double u1, double v1, double u2, double v2,
                                          double inv_s2, bool& in) {
    const double th = 5.991;
    double sc = 0.0;
    in = true;
    const double w2 = 1.0 / ((Hi[6] * u2 + Hi[7] * v2) + Hi[8]);
    const double u2in1 = ((Hi[0] * u2 + Hi[1] * v2) + Hi[2]) * w2;
    const double v2in1 = ((Hi[3] * u2 + Hi[4] * v2) + Hi[5]) * w2;
    const double chi1 = ((u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1)) * inv_s2;
    if (chi1 > th) in = false;
    else sc = sc + (th - chi1);
    const double w1 = 1.0 / ((H[6] * u1 + H[7] * v1) + H[8]);
    const double u1in2 = ((H[0] * u1 + H[1] * v1) + H[2]) * w1;
    const double v1in2 = ((H[3] * u1 + H[4] * v1) + H[5]) * w1;
    const double chi2 = ((u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2)) * inv_s2;
    if (chi2 > th) in = false;
    else sc = sc + (th - chi2);
    return sc;
}

// CheckFundamental's body (cc:676-724)
__device__ __forceinline__ double score_f(const double* F, double u1, double v1, double u2, double v2, double inv_s2,
                                          bool& in) {
    const double th = 3.841, th_score = 5.991;
    double sc = 0.0;
    in = true;
    const double a2 = (F[0] * u1 + F[1] * v1) + F[2];
    const double b2 = (F[3] * u1 + F[4] * v1) + F[5];
    const double c2 = (F[6] * u1 + F[7] * v1) + F[8];
    const double num2 = (a2 * u2 + b2 * v2) + c2;
    const double chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv_s2;
    if (chi1 > th) in = false;
    else sc = sc + (th_score - chi1);
    const double a1 = (F[0] * u2 + F[3] * v2) + F[6];
    const double b1 = (F[1] * u2 + F[4] * v2) + F[7];
    const double c1 = (F[2] * u2 + F[5] * v2) + F[8];
    const double num1 = (a1 * u1 + b1 * v1) + c1;
    const double chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv_s2;
    if (chi2 > th) in = false;
    else sc = sc + (th_score - chi2);
    return sc;
}

__global__ __launch_bounds__(kInitThreads) void k_init_score(InitArgs A) {
    const int b = blockIdx.z, model = blockIdx.y, lane = threadIdx.x & 63;
    const int it = blockIdx.x * kInitWaves + (threadIdx.x >> 6);
    const int N = A.W.state[(size_t)b * kInitState + kIsN];
    if (it >= A.iterations || N < 8) return;
    double* dst = A.W.scores + ((size_t)b * 2 + model) * A.W.max_iterations + it;
    if (A.W.bad[(size_t)b * A.W.max_iterations + it]) {
        if (lane == 0) *dst = 0.0;
        return;
    }
    const double* mat = A.W.mats + ((size_t)b * A.W.max_iterations + it) * kInitMats;
    double M[9], Mi[9];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        M[i] = model == 0 ? mat[i] : mat[18 + i];
        Mi[i] = mat[9 + i];
    }
    const size_t c = (size_t)A.W.kcap;
    const double* pts = A.W.pts + (size_t)b * 4 * c;
    const double inv_s2 = 1.0 / (A.sigma * A.sigma);
    double acc = 0.0;
    for (int i = lane; i < N; i += 64) {
        bool in;
        const double u1 = pts[i], v1 = pts[c + i], u2 = pts[2 * c + i], v2 = pts[3 * c + i];
        acc = acc + (model == 0 ? score_h(M, Mi, u1, v1, u2, v2, inv_s2, in) : score_f(M, u1, v1, u2, v2, inv_s2, in));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc = acc + __shfl_xor(acc, off);
    if (lane == 0) *dst = acc;
}

// ---- k_init_select --------------------------------------------------------------------------

__device__ __forceinline__ void store_hyp(double* dst, const double* R, double t0, double t1, double t2) {
#pragma unroll
    for (int i = 0; i < 9; i++) dst[i] = R[i];
    dst[9] = t0;
    dst[10] = t1;
    dst[11] = t2;
}

// ReconstructH's eight (R, t) (cc:915-1033).  Returns false where d1/d2 or d2/d3 fails.
__device__ bool hypotheses_h(const InitArgs& A, const double* H, double* hyp) {
    const double K[9] = {A.fx, 0.0, A.cx, 0.0, A.fy, A.cy, 0.0, 0.0, 1.0};
    const double Ki[9] = {1.0 / A.fx, 0.0, -A.cx / A.fx, 0.0, 1.0 / A.fy, -A.cy / A.fy, 0.0, 0.0, 1.0};
    double tmp[9], M[9], B[9], V[9], w[3], U[9], Vt[9];
    mul3(Ki, H, tmp);
    mul3(tmp, K, M);
    svd3(M, B, V, w);
    svd3_u(B, w, U);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Vt[3 * i + j] = V[3 * j + i];
    const double s = det3(U) * det3(Vt);
    const double d1 = w[0], d2 = w[1], d3 = w[2];
    if (d1 / d2 < 1.00001 || d2 / d3 < 1.00001) return false;
    const double aux1 = sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
    const double aux3 = sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const double x1[4] = {aux1, aux1, -aux1, -aux1};
    const double x3[4] = {aux3, -aux3, aux3, -aux3};
    const double aux_st = sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
    const double ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const double st[4] = {aux_st, -aux_st, -aux_st, aux_st};
    const double aux_sp = sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
    const double cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    const double sp[4] = {aux_sp, -aux_sp, -aux_sp, aux_sp};
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int k = i & 3;
        const bool second = i >= 4;
        const double Rp[9] = {second ? cp : ct, 0.0, second ? sp[k] : -st[k], 0.0, second ? -1.0 : 1.0, 0.0,
                              second ? sp[k] : st[k], 0.0, second ? -cp : ct};
        double R[9];
        mul3(U, Rp, tmp);
        mul3(tmp, Vt, R);
#pragma unroll
        for (int j = 0; j < 9; j++) R[j] = s * R[j];
        const double f = second ? d1 + d3 : d1 - d3;
        const double tp0 = x1[k] * f, tp2 = (second ? x3[k] : -x3[k]) * f;
        const double t0 = U[0] * tp0 + U[2] * tp2, t1 = U[3] * tp0 + U[5] * tp2, t2 = U[6] * tp0 + U[8] * tp2;
        const double n = sqrt((t0 * t0 + t1 * t1) + t2 * t2);
        store_hyp(hyp + 12 * i, R, t0 / n, t1 / n, t2 / n);
    }
    return true;
}

// ReconstructF's four (R, t): E = K^T F K, DecomposeE (cc:760-771, 1391-1415)
__device__ void hypotheses_f(const InitArgs& A, const double* F, double* hyp) {
    const double K[9] = {A.fx, 0.0, A.cx, 0.0, A.fy, A.cy, 0.0, 0.0, 1.0};
    const double Kt[9] = {A.fx, 0.0, 0.0, 0.0, A.fy, 0.0, A.cx, A.cy, 1.0};
    double tmp[9], E[9], B[9], V[9], w[3], U[9], Vt[9];
    mul3(Kt, F, tmp);
    mul3(tmp, K, E);
    svd3(E, B, V, w);
    svd3_u(B, w, U);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Vt[3 * i + j] = V[3 * j + i];
    const double n = sqrt((U[2] * U[2] + U[5] * U[5]) + U[8] * U[8]);
    const double t0 = U[2] / n, t1 = U[5] / n, t2 = U[8] / n;
    const double W[9] = {0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0};
    const double Wt[9] = {0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0};
    double R1[9], R2[9];
    mul3(U, W, tmp);
    mul3(tmp, Vt, R1);
    if (det3(R1) < 0.0) {
#pragma unroll
        for (int i = 0; i < 9; i++) R1[i] = -R1[i];
    }
    mul3(U, Wt, tmp);
    mul3(tmp, Vt, R2);
    if (det3(R2) < 0.0) {
#pragma unroll
        for (int i = 0; i < 9; i++) R2[i] = -R2[i];
    }
    store_hyp(hyp, R1, t0, t1, t2);
    store_hyp(hyp + 12, R2, t0, t1, t2);
    store_hyp(hyp + 24, R1, -t0, -t1, -t2);
    store_hyp(hyp + 36, R2, -t0, -t1, -t2);
}

__global__ __launch_bounds__(kInitThreads) void k_init_select(InitArgs A) {
    __shared__ double s_M[kInitMats];  // the winners' H21, H12, F21
    __shared__ double s_score[2];
    __shared__ int s_best[2], s_status, s_n[2];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    int32_t* st = A.W.state + (size_t)b * kInitState;
    const int N = st[kIsN], n1 = st[kIsN1];
    const orbx_initializer_result& o = A.out;
    const size_t orow = (size_t)b * A.kcap;
    if (tid == 0) {
        int status = st[kIsStatus];
        for (int model = 0; model < 2; model++) {  // cc:209-243, 285-308
            double score = 0.0;
            int best = -1;
            if (N >= 8) {
                const double* sc = A.W.scores + ((size_t)b * 2 + model) * A.W.max_iterations;
                for (int it = 0; it < A.iterations; it++)
                    if (sc[it] > score) {  // a tie keeps the earlier iteration
                        score = sc[it];
                        best = it;
                    }
            }
            s_score[model] = score;
            s_best[model] = best;
        }
        if (N >= 8)
            for (int it = 0; it < A.iterations; it++)
                if (A.W.bad[(size_t)b * A.W.max_iterations + it]) status |= ORBX_INIT_STATUS_BAD_SET;
        s_status = status;
        s_n[0] = s_n[1] = 0;
    }
    __syncthreads();
    if (tid < kInitMats) {
        const int it = s_best[tid < 18 ? 0 : 1];
        s_M[tid] = it >= 0 ? A.W.mats[((size_t)b * A.W.max_iterations + it) * kInitMats + tid] : 0.0;
    }
    for (int i = tid; i < n1; i += kInitThreads) {
        if (o.inliers_H) o.inliers_H[orow + i] = 0;
        if (o.inliers_F) o.inliers_F[orow + i] = 0;
        if (o.triangulated) o.triangulated[orow + i] = 0;
        if (o.p3d) o.p3d[3 * (orow + i)] = o.p3d[3 * (orow + i) + 1] = o.p3d[3 * (orow + i) + 2] = 0.0f;
    }
    __syncthreads();
    const double SH = s_score[0], SF = s_score[1];
    const double RH = SH / (SH + SF);  // cc:145
    const int model = RH > 0.40 ? 0 : 1;
    const size_t c = (size_t)A.W.kcap;
    const double* pts = A.W.pts + (size_t)b * 4 * c;
    const int32_t* idx1 = A.W.idx1 + (size_t)b * c;
    uint8_t* inl = A.W.inl + (size_t)b * c;
    const double inv_s2 = 1.0 / (A.sigma * A.sigma);
    int nh = 0, nf = 0;
    for (int base = 0; base < N; base += kInitThreads) {
        const int i = base + tid;
        bool in_h = false, in_f = false;
        if (i < N) {
            const double u1 = pts[i], v1 = pts[c + i], u2 = pts[2 * c + i], v2 = pts[3 * c + i];
            if (s_best[0] >= 0) (void)score_h(s_M, s_M + 9, u1, v1, u2, v2, inv_s2, in_h);
            if (s_best[1] >= 0) (void)score_f(s_M + 18, u1, v1, u2, v2, inv_s2, in_f);
            inl[i] = (model == 0 ? in_h : in_f) ? 1 : 0;
            const int k = idx1[i];  // < n1
            if (in_h && o.inliers_H) o.inliers_H[orow + k] = 1;
            if (in_f && o.inliers_F) o.inliers_F[orow + k] = 1;
        }
        nh += __popcll(__ballot(in_h));
        nf += __popcll(__ballot(in_f));
    }
    if (lane == 0) {
        atomicAdd(&s_n[0], nh);
        atomicAdd(&s_n[1], nf);
    }
    __syncthreads();
    if (tid == 0) {
        double* hyp = A.W.hyp + (size_t)b * kInitHyps * 12;
        int nhyp = 4, ratio_fail = 0;
        if (model == 0) {
            nhyp = 8;
            if (!hypotheses_h(A, s_M, hyp)) {
                nhyp = 0;
                ratio_fail = 1;
            }
        } else {
            hypotheses_f(A, s_M + 18, hyp);
        }
        st[kIsNhyp] = nhyp;
        st[kIsModel] = model;
        st[kIsNinl] = s_n[model];
        st[kIsStatus] = s_status;
        st[kIsRatioFail] = ratio_fail;
        if (o.model) o.model[b] = model;
        if (o.n_matches) o.n_matches[b] = N;
        if (o.SH) o.SH[b] = (float)SH;
        if (o.SF) o.SF[b] = (float)SF;
        if (o.RH) o.RH[b] = (float)RH;
        if (o.best_it_H) o.best_it_H[b] = s_best[0];
        if (o.best_it_F) o.best_it_F[b] = s_best[1];
        if (o.H21)
            for (int i = 0; i < 9; i++) o.H21[(size_t)b * 9 + i] = (float)s_M[i];
        if (o.F21)
            for (int i = 0; i < 9; i++) o.F21[(size_t)b * 9 + i] = (float)s_M[18 + i];
        if (o.n_inliers_H) o.n_inliers_H[b] = s_n[0];
        if (o.n_inliers_F) o.n_inliers_F[b] = s_n[1];
        if (o.status) o.status[b] = s_status;
    }
}

// ---- CheckRT --------------------------------------------------------------------------------

struct RtCam {
    double R[9], t[3], O2[3];
    double fx, fy, cx, cy, th2;
};

__device__ __forceinline__ void load_cam(const InitArgs& A, const double* hyp, RtCam& C) {
#pragma unroll
    for (int i = 0; i < 9; i++) C.R[i] = hyp[i];
#pragma unroll
    for (int i = 0; i < 3; i++) C.t[i] = hyp[9 + i];
#pragma unroll
    for (int i = 0; i < 3; i++) C.O2[i] = -((C.R[i] * C.t[0] + C.R[3 + i] * C.t[1]) + C.R[6 + i] * C.t[2]);  // cc:1254
    C.fx = A.fx;
    C.fy = A.fy;
    C.cx = A.cx;
    C.cy = A.cy;
    C.th2 = 4.0 * (A.sigma * A.sigma);
}

// CheckRT's body for one inlier (cc:1267-1357): good, and then the point, its cosine and flag
__device__ __forceinline__ bool check_rt(const RtCam& C, double u1, double v1, double u2, double v2, double& X,
                                         double& Y, double& Z, double& cosp, bool& tri) {
    const double* R = C.R;
    // P2 = K [R | t] (cc:1252)
    const double p00 = C.fx * R[0] + C.cx * R[6], p01 = C.fx * R[1] + C.cx * R[7], p02 = C.fx * R[2] + C.cx * R[8],
                 p03 = C.fx * C.t[0] + C.cx * C.t[2];
    const double p10 = C.fy * R[3] + C.cy * R[6], p11 = C.fy * R[4] + C.cy * R[7], p12 = C.fy * R[5] + C.cy * R[8],
                 p13 = C.fy * C.t[1] + C.cy * C.t[2];
    const double p20 = R[6], p21 = R[7], p22 = R[8], p23 = C.t[2];
    double h0, h1, h2, h3;
    smallest_right_singular_vector(  // cc:1112-1124 with P1 = K [I | 0]
        u1 * 0.0 - C.fx, u1 * 0.0 - 0.0, u1 * 1.0 - C.cx, u1 * 0.0 - 0.0,
        v1 * 0.0 - 0.0, v1 * 0.0 - C.fy, v1 * 1.0 - C.cy, v1 * 0.0 - 0.0,
        u2 * p20 - p00, u2 * p21 - p01, u2 * p22 - p02, u2 * p23 - p03,
        v2 * p20 - p10, v2 * p21 - p11, v2 * p22 - p12, v2 * p23 - p13, h0, h1, h2, h3);
    X = h0 / h3;
    Y = h1 / h3;
    Z = h2 / h3;
    if (!isfinite(X) || !isfinite(Y) || !isfinite(Z)) return false;
    const double dist1 = sqrt((X * X + Y * Y) + Z * Z);
    const double n0 = X - C.O2[0], n1 = Y - C.O2[1], n2 = Z - C.O2[2];
    const double dist2 = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
    cosp = ((X * n0 + Y * n1) + Z * n2) / (dist1 * dist2);
    if (Z <= 0.0 && cosp < 0.99998) return false;
    const double x2 = ((R[0] * X + R[1] * Y) + R[2] * Z) + C.t[0];
    const double y2 = ((R[3] * X + R[4] * Y) + R[5] * Z) + C.t[1];
    const double z2 = ((R[6] * X + R[7] * Y) + R[8] * Z) + C.t[2];
    if (z2 <= 0.0 && cosp < 0.99998) return false;
    const double iz1 = 1.0 / Z;
    const double e1x = (C.fx * X * iz1 + C.cx) - u1, e1y = (C.fy * Y * iz1 + C.cy) - v1;
    if (e1x * e1x + e1y * e1y > C.th2) return false;
    const double iz2 = 1.0 / z2;
    const double e2x = (C.fx * x2 * iz2 + C.cx) - u2, e2y = (C.fy * y2 * iz2 + C.cy) - v2;
    if (e2x * e2x + e2y * e2y > C.th2) return false;
    tri = cosp < 0.99998;
    return true;
}

__global__ __launch_bounds__(kInitThreads) void k_init_checkrt(InitArgs A) {
    __shared__ int s_good;
    const int b = blockIdx.y, k = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int32_t* st = A.W.state + (size_t)b * kInitState;
    const int N = st[kIsN];
    if (k >= st[kIsNhyp]) return;
    if (tid == 0) s_good = 0;
    __syncthreads();
    RtCam C;
    load_cam(A, A.W.hyp + ((size_t)b * kInitHyps + k) * 12, C);
    const size_t c = (size_t)A.W.kcap;
    const double* pts = A.W.pts + (size_t)b * 4 * c;
    const uint8_t* inl = A.W.inl + (size_t)b * c;
    double* cw = A.W.cosw + ((size_t)b * kInitHyps + k) * c;
    int cnt = 0;
    for (int base = 0; base < N; base += kInitThreads) {
        const int i = base + tid;
        bool good = false;
        if (i < N) {
            double X, Y, Z, cosp = 0.0;
            bool tri;
            if (inl[i]) good = check_rt(C, pts[i], pts[c + i], pts[2 * c + i], pts[3 * c + i], X, Y, Z, cosp, tri);
            cw[i] = good ? cosp : __builtin_inf();
        }
        cnt += __popcll(__ballot(good));
    }
    if (lane == 0) atomicAdd(&s_good, cnt);
    __syncthreads();  // the cosines are in memory, the count is whole
    const int ngood = s_good;
    if (tid == 0) {
        A.W.good[(size_t)b * kInitHyps + k] = ngood;
        if (ngood == 0) A.W.par[(size_t)b * kInitHyps + k] = 0.0;
    }
    if (ngood == 0) return;
    const int target = ngood - 1 < 50 ? ngood - 1 : 50;  // cc:1369
    for (int i = tid; i < N; i += kInitThreads) {
        const double ci = cw[i];
        if (!(ci < __builtin_inf())) continue;
        int rank = 0;
        for (int j = 0; j < N; j++) {
            const double cj = cw[j];
            rank += (cj < ci || (cj == ci && j < i)) ? 1 : 0;
        }
        if (rank == target) A.W.par[(size_t)b * kInitHyps + k] = acos(ci) * 180.0 / kPi;  // cc:1371
    }
}

__global__ __launch_bounds__(kInitThreads) void k_init_finish(InitArgs A) {
    __shared__ int s_ok, s_k;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int32_t* st = A.W.state + (size_t)b * kInitState;
    const int N = st[kIsN];
    const orbx_initializer_result& o = A.out;
    const double* hyp = A.W.hyp + (size_t)b * kInitHyps * 12;
    if (tid == 0) {
        const int nhyp = st[kIsNhyp], model = st[kIsModel], ninl = st[kIsNinl];
        const int32_t* good = A.W.good + (size_t)b * kInitHyps;
        const double* par = A.W.par + (size_t)b * kInitHyps;
        int ok = 0, win = 0, best_good = 0, second_good = 0, nsimilar = 0;
        double parallax = 0.0;
        if (model == 1) {  // cc:802-883
            int max_good = 0;
            for (int k = 0; k < nhyp; k++) max_good = good[k] > max_good ? good[k] : max_good;
            const int by_inliers = (int)(0.9 * (double)ninl);
            const int n_min_good = by_inliers > 50 ? by_inliers : 50;
            for (int k = 0; k < nhyp; k++)
                if ((double)good[k] > 0.7 * (double)max_good) nsimilar++;
            for (int k = nhyp - 1; k >= 0; k--)
                if (good[k] == max_good) win = k;
            for (int k = 0; k < nhyp; k++)
                if (k != win && good[k] > second_good) second_good = good[k];
            best_good = max_good;
            parallax = par[win];
            ok = !(max_good < n_min_good || nsimilar > 1) && parallax > 1.0;
        } else if (!st[kIsRatioFail]) {  // cc:1036-1096
            parallax = -1.0;
            for (int k = 0; k < nhyp; k++) {
                if (good[k] > best_good) {
                    second_good = best_good;
                    best_good = good[k];
                    win = k;
                    parallax = par[k];
                } else if (good[k] > second_good) {
                    second_good = good[k];
                }
            }
            ok = (double)second_good < 0.75 * (double)best_good && parallax >= 1.0 && best_good > 50 &&
                 (double)best_good > 0.9 * (double)ninl;
        }
        s_ok = ok;
        s_k = win;
        if (o.ok) o.ok[b] = ok;
        if (o.best_good) o.best_good[b] = best_good;
        if (o.second_good) o.second_good[b] = second_good;
        if (o.n_similar) o.n_similar[b] = nsimilar;
        if (o.parallax) o.parallax[b] = (float)parallax;
        if (o.R21)
            for (int i = 0; i < 9; i++) o.R21[(size_t)b * 9 + i] = ok ? (float)hyp[12 * win + i] : 0.0f;
        if (o.t21)
            for (int i = 0; i < 3; i++) o.t21[(size_t)b * 3 + i] = ok ? (float)hyp[12 * win + 9 + i] : 0.0f;
    }
    __syncthreads();
    if (!s_ok || (!o.p3d && !o.triangulated)) return;
    RtCam C;
    load_cam(A, hyp + 12 * s_k, C);
    const size_t c = (size_t)A.W.kcap, orow = (size_t)b * A.kcap;
    const double* pts = A.W.pts + (size_t)b * 4 * c;
    const uint8_t* inl = A.W.inl + (size_t)b * c;
    const int32_t* idx1 = A.W.idx1 + (size_t)b * c;
    for (int i = tid; i < N; i += kInitThreads) {
        if (!inl[i]) continue;
        double X, Y, Z, cosp;
        bool tri;
        if (!check_rt(C, pts[i], pts[c + i], pts[2 * c + i], pts[3 * c + i], X, Y, Z, cosp, tri)) continue;
        const size_t k = orow + idx1[i];  // idx1 < n1: k_init_select zeroed these slots
        if (o.p3d) {
            o.p3d[3 * k] = (float)X;
            o.p3d[3 * k + 1] = (float)Y;
            o.p3d[3 * k + 2] = (float)Z;
        }
        if (o.triangulated) o.triangulated[k] = tri ? 1 : 0;
    }
}

}  // namespace orbx

// ---------------------------------------------------------------------------------------
// Host side

struct orbx_initializer {
    orbx_matcher* matcher = nullptr;
    int device = 0, max_batch = 0, kcap = 0, max_iterations = 0;
    hipStream_t stream = nullptr;  // the matcher's
    char* work = nullptr;
    orbx::DeviceBuffer stage;      // the single host form's pair and results
    orbx::InitWork W{};
};

namespace {

using namespace orbx;

// the argument checks of both forms, before any GPU work
int check_batch(const orbx_initializer* s, const orbx_initializer_batch* in) {
    if (in->batch < 0 || in->batch > s->max_batch || in->kcap < 1 || in->kcap > s->kcap || in->max_iterations < 1 ||
        in->max_iterations > s->max_iterations || !(in->sigma > 0.0f))
        return fail(ORBX_ERR_ARG, "bad argument");
    if (!in->K) return fail(ORBX_ERR_ARG, "null host array");
    if (in->batch > 0 && (!in->n1 || !in->n2 || !in->keys1 || !in->keys2 || !in->matches12 || !in->sets))
        return fail(ORBX_ERR_ARG, "null buffer");
    return ORBX_OK;
}

}  // namespace

extern "C" {

int orbx_initializer_create(orbx_matcher* m, int max_batch, int kcap, int max_iterations, orbx_initializer** out) {
    if (!out) return fail(ORBX_ERR_ARG, "null argument");
    *out = nullptr;
    if (!m) return fail(ORBX_ERR_ARG, "null matcher");
    if (max_batch < 1 || kcap < 1 || kcap > 8192 || max_iterations < 1 || max_iterations > ORBX_INIT_MAX_ITERATIONS)
        return fail(ORBX_ERR_ARG, "bad argument");
    if ((size_t)max_batch * (size_t)kcap * 8 >= ((size_t)1 << 31) ||
        (size_t)max_batch * (size_t)max_iterations * kInitMats >= ((size_t)1 << 31))
        return fail(ORBX_ERR_ARG, "max_batch x kcap x 8 or max_batch x max_iterations x 27 of 2^31 or more");
    orbx_initializer* s = new (std::nothrow) orbx_initializer();
    if (!s) return fail(ORBX_ERR_ARG, "out of host memory");
    s->matcher = m;
    s->device = matcher_device(m);
    s->stream = matcher_stream(m);
    s->max_batch = max_batch;
    s->kcap = kcap;
    s->max_iterations = max_iterations;
    const size_t B = (size_t)max_batch, slots = B * kcap, its = B * max_iterations;
    Layout L(up256);
    const size_t o_pts = L.take(slots * 4 * 8), o_idx1 = L.take(slots * 4), o_norm = L.take(B * 8 * 8),
                 o_state = L.take(B * kInitState * 4), o_mats = L.take(its * kInitMats * 8), o_bad = L.take(its * 4),
                 o_scores = L.take(its * 2 * 8), o_inl = L.take(slots), o_hyp = L.take(B * kInitHyps * 12 * 8),
                 o_cosw = L.take(slots * kInitHyps * 8), o_good = L.take(B * kInitHyps * 4),
                 o_par = L.take(B * kInitHyps * 8);
    hipError_t e = hipSetDevice(s->device);
    if (e == hipSuccess) e = hipMalloc((void**)&s->work, L.total());
    if (e != hipSuccess) {
        delete s;
        set_last_error(std::string("orbx_initializer_create: ") + hipGetErrorString(e));
        return ORBX_ERR_HIP;
    }
    s->W.pts = (double*)(s->work + o_pts);
    s->W.idx1 = (int32_t*)(s->work + o_idx1);
    s->W.norm = (double*)(s->work + o_norm);
    s->W.state = (int32_t*)(s->work + o_state);
    s->W.mats = (double*)(s->work + o_mats);
    s->W.bad = (int32_t*)(s->work + o_bad);
    s->W.scores = (double*)(s->work + o_scores);
    s->W.inl = (uint8_t*)(s->work + o_inl);
    s->W.hyp = (double*)(s->work + o_hyp);
    s->W.cosw = (double*)(s->work + o_cosw);
    s->W.good = (int32_t*)(s->work + o_good);
    s->W.par = (double*)(s->work + o_par);
    s->W.kcap = kcap;
    s->W.max_iterations = max_iterations;
    *out = s;
    return ORBX_OK;
}

void orbx_initializer_destroy(orbx_initializer* s) {
    if (!s || orbx::unloading()) return;  // DESIGN.md §1 "Teardown"
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    if (s->work) (void)hipFree(s->work);
    s->stage.release();
    delete s;
}

int orbx_initializer_initialize_device(orbx_initializer* s, const orbx_initializer_batch* in,
                                       const orbx_initializer_result* out, void* stream) {
    if (!s || !in || !out) return fail(ORBX_ERR_ARG, "null argument");
    const int rc = check_batch(s, in);
    if (rc) return rc;
    const int B = in->batch;
    if (B == 0) return ORBX_OK;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = stream ? (hipStream_t)stream : s->stream;
    InitArgs A{};
    A.W = s->W;
    A.n1 = in->n1;
    A.n2 = in->n2;
    A.keys1 = in->keys1;
    A.keys2 = in->keys2;
    A.matches12 = in->matches12;
    A.sets = in->sets;
    A.kcap = in->kcap;
    A.iterations = in->max_iterations;
    A.fx = (double)in->K[0];
    A.fy = (double)in->K[1];
    A.cx = (double)in->K[2];
    A.cy = (double)in->K[3];
    A.sigma = (double)in->sigma;
    A.out = *out;
    const unsigned its = (unsigned)A.iterations;
    k_init_normalize<<<B, kInitThreads, 0, st>>>(A);
    HIP_TRY(hipGetLastError());
    const dim3 ghyp((its + kHypLanes - 1) / kHypLanes, (unsigned)B);
    k_init_hyp<16><<<ghyp, kHypLanes, 0, st>>>(A);
    HIP_TRY(hipGetLastError());
    k_init_hyp<8><<<ghyp, kHypLanes, 0, st>>>(A);
    HIP_TRY(hipGetLastError());
    k_init_score<<<dim3((its + kInitWaves - 1) / kInitWaves, 2, (unsigned)B), kInitThreads, 0, st>>>(A);
    HIP_TRY(hipGetLastError());
    k_init_select<<<B, kInitThreads, 0, st>>>(A);
    HIP_TRY(hipGetLastError());
    k_init_checkrt<<<dim3(kInitHyps, (unsigned)B), kInitThreads, 0, st>>>(A);
    HIP_TRY(hipGetLastError());
    k_init_finish<<<B, kInitThreads, 0, st>>>(A);
    HIP_TRY(hipGetLastError());
    return ORBX_OK;
}

int orbx_initializer_initialize(orbx_initializer* s, const orbx_initializer_batch* in,
                                const orbx_initializer_result* out) {
    if (!s || !in || !out) return fail(ORBX_ERR_ARG, "null argument");
    if (in->batch != 1) return fail(ORBX_ERR_ARG, "the host form takes one frame pair");
    int rc = check_batch(s, in);
    if (rc) return rc;
    CallClock clock(s->matcher);
    const size_t kcap = (size_t)in->kcap, its = (size_t)in->max_iterations;
    const int n1 = in->n1[0] < 0 ? 0 : (in->n1[0] > in->kcap ? in->kcap : in->n1[0]);
    const int n2 = in->n2[0] < 0 ? 0 : (in->n2[0] > in->kcap ? in->kcap : in->n2[0]);
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    const size_t N1 = (size_t)n1;
    const struct {
        int32_t n1, n2;
    } n12{n1, n2}, *d_n = nullptr;
    orbx_initializer_batch d = *in;
    orbx_initializer_result o{};
    HostStage h(up256);
    h.in(&d_n, &n12, 1, 1);
    h.in(&d.keys1, in->keys1, N1, kcap);
    h.in(&d.keys2, in->keys2, (size_t)n2, kcap);
    h.in(&d.matches12, in->matches12, N1, kcap);
    h.in(&d.sets, in->sets, 8 * its, 8 * its);
    // results: twelve ints (one spare) and the floats packed, then each array rounded to 256
    h.out(&o.ok, &out->ok, 1, 1);
    h.out(&o.model, &out->model, 1, 1);
    h.out(&o.n_matches, &out->n_matches, 1, 1);
    h.out(&o.best_it_H, &out->best_it_H, 1, 1);
    h.out(&o.best_it_F, &out->best_it_F, 1, 1);
    h.out(&o.n_inliers_H, &out->n_inliers_H, 1, 1);
    h.out(&o.n_inliers_F, &out->n_inliers_F, 1, 1);
    h.out(&o.best_good, &out->best_good, 1, 1);
    h.out(&o.second_good, &out->second_good, 1, 1);
    h.out(&o.n_similar, &out->n_similar, 1, 1);
    h.out(&o.status, &out->status, 1, 2);
    h.out(&o.SH, &out->SH, 1, 1);
    h.out(&o.SF, &out->SF, 1, 1);
    h.out(&o.RH, &out->RH, 1, 1);
    h.out(&o.parallax, &out->parallax, 1, 1);
    h.out(&o.H21, &out->H21, 9, 9);
    h.out(&o.F21, &out->F21, 9, 9);
    h.out(&o.R21, &out->R21, 9, 9);
    h.out(&o.t21, &out->t21, 3, 3);
    h.res.align256();
    h.out(&o.inliers_H, &out->inliers_H, N1, up256(kcap));
    h.out(&o.inliers_F, &out->inliers_F, N1, up256(kcap));
    h.out(&o.triangulated, &out->triangulated, N1, up256(kcap));
    h.out(&o.p3d, &out->p3d, 3 * N1, up256(kcap * 12) / 4);
    HIP_TRY(h.stage(s->stage, st));
    d.n1 = &d_n->n1;
    d.n2 = &d_n->n2;
    rc = orbx_initializer_initialize_device(s, &d, &o, st);
    if (rc) return rc;
    HIP_TRY(h.download(st));
    return ORBX_OK;
}

int orbx_initializer_sets(int32_t* sets, int n, int iterations) {
    if (!sets || n < 0 || iterations < 0) return fail(ORBX_ERR_ARG, "bad argument");
    srand(0);  // DUtils::Random::SeedRandOnce(0) on its first use (cc:103)
    std::vector<int32_t> avail;
    for (int it = 0; it < iterations; it++) {
        if (n < 8) {
            for (int j = 0; j < 8; j++) sets[(size_t)it * 8 + j] = 0;
            continue;
        }
        avail.resize((size_t)n);
        for (int i = 0; i < n; i++) avail[(size_t)i] = i;  // vAvailableIndices = vAllIndices
        for (int j = 0; j < 8; j++) {
            const int d = (int)avail.size();  // RandomInt(0, size - 1), DUtils/Random.cpp:47-49
            const int randi = (int)(((double)rand() / ((double)RAND_MAX + 1.0)) * d);
            sets[(size_t)it * 8 + j] = avail[(size_t)randi];
            avail[(size_t)randi] = avail.back();
            avail.pop_back();
        }
    }
    return ORBX_OK;
}

}  // extern "C"
