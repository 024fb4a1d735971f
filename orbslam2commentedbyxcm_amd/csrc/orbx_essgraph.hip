// orbx_essgraph.hip -- Optimizer::OptimizeEssentialGraph (the pose-graph optimisation of
// LoopClosing::CorrectLoop) for a batch of maps in HBM: one persistent workgroup per problem
// forms the measurements, builds the adjacency and the envelope, runs the Levenberg-Marquardt
// iterations and recovers the poses and the map points; the host reads nothing back in between.
//
// Reference: src/Optimizer.cc:873-1150 and, under Thirdparty/g2o/g2o,
//   types/types_seven_dof_expmap.h:60-69, 106-114      oplusImpl, EdgeSim3::computeError
//   types/sim3.h:64-272                                Sim3(R, t, s), exp, log, map, inverse, operator*
//   core/base_binary_edge.hpp:55-120, 131-205          constructQuadraticForm, numeric linearizeOplus
//   core/optimization_algorithm_levenberg.cpp:61-189   solve, computeScale (lambda: setUserLambdaInit)
//   core/block_solver.hpp                              BlockSolver_7_3 with nothing marginalised
// DESIGN.md §4.22.
//
// Float inputs are widened to double; everything after is double (the build keeps
// -ffp-contract=off); outputs are rounded to float once.
//
// No workgroup waits on another and no sum uses a floating-point atomic.  Every sum has one
// owner and a fixed shape:
//   a vertex's block column of H (its diagonal block and the blocks above it) and its part of
//     b: one wave; lane l < 49 owns entry l of every block, lanes 49..55 the entries of b; the
//     wave walks the vertex's incident edges in edge order, which is g2o's order;
//   chi2 and computeScale: thread t adds its edges (vertices) t, t + 256, ..., then block_sum;
//   an entry of the factor: the pivots in ascending order, each term (l u) d, exactly the
//     terms lm::ldlt_solve_block gives it; the terms left out are exact zeros.
// The integer atomics only count: the adjacency lists they fill are sorted into edge order,
// and the order of a block row's column list touches no sum.
//
// The linear system is a block envelope (skyline) in natural (mnId) order: block column f
// holds the 7 x 7 blocks (g, f), g = first[f] .. f, where first[f] is the smallest index among
// f and its neighbours.  H, its factor, b, the solution and every work vector live in the
// HBM workspace: 7 F doubles pass the LDS of a compute unit near F = 2900, and one path for
// every size is worth more than the LDS's latency at small ones.  The scan,
// the owner's sort, the row lists and the solver are orbx_envelope.h's, shared with
// orbx_globalba.hip and instantiated here with 7 x 7 blocks.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "orbx.h"
#include "orbx_envelope.h"
#include "orbx_error.h"
#include "orbx_kernels.h"
#include "orbx_layout.h"
#include "orbx_lm.h"
#include "orbx_sim3.h"

namespace orbx {

namespace {

constexpr int kEgThreads = 256;
constexpr int kEgWaves = kEgThreads / 64;

static_assert(kEgThreads == env::kThreads, "orbx_envelope.h is written for this workgroup");
using env::block_scan;
using env::sort_ascending;

// One problem's rows and its regions of the workspace; the envelope H, its factor L, b, x,
// the work vectors and the envelope's index lists are env::Envelope's.
struct Prob : env::Envelope {
    int K, E, P, loop;
    bool fix_scale;
    const int32_t* ev;    // [E][2]
    const S3* probes;     // [14] kernel arguments
    double* S;            // [K][3][8]: vScw, the estimate, its backup
    double* meas;         // [E][8]
    double* J;            // [E][2][49]: the Jacobian of vertex 0 / 1, column d at [7 d .. 7 d + 6]
    double* err;          // [E][7]
    int32_t *ok, *free_idx, *free_kf, *adj_off, *adj, *deg;
    double* s_red;
};

// EdgeSim3::computeError, types_seven_dof_expmap.h:106-114: (C * S_i * S_j^-1).log()
__device__ __forceinline__ void edge_error(const S3& CSi, const S3& SjInv, double (&e)[7]) {
    s3_log(s3_mul(CSi, SjInv), e);
}

__device__ __forceinline__ double dot7(const double (&e)[7]) {  // chi2 with information = I
    double s = e[0] * e[0];
#pragma unroll
    for (int r = 1; r < 7; r++) s += e[r] * e[r];
    return s;
}

// computeActiveErrors + activeChi2 at estimate slot `slot`; with `jac` also linearizeOplus of
// every edge (base_binary_edge.hpp:131-205): work item w < E is vertex 0 of edge w (and the
// edge's error), w >= E vertex 1 of edge w - E; a fixed vertex has no Jacobian.
__device__ __forceinline__ double errors(const Prob& Q, int slot, bool jac) {
    double v[1] = {0.0};
    const double scalar = 1.0 / (2 * 1e-9);
    const int items = jac ? 2 * Q.E : Q.E;
    for (int w = threadIdx.x; w < items; w += kEgThreads) {
        const int side = w >= Q.E, e = side ? w - Q.E : w;
        if (!Q.ok[e]) continue;
        const int vi = Q.ev[2 * e], vj = Q.ev[2 * e + 1];
        const S3 Si = s3_load(Q.S + ((size_t)vi * 3 + slot) * 8), Sj = s3_load(Q.S + ((size_t)vj * 3 + slot) * 8);
        const S3 C = s3_load(Q.meas + (size_t)e * 8);
        double* Jc = Q.J + ((size_t)e * 2 + side) * 49;
        if (side == 0) {
            const S3 SjInv = s3_inverse(Sj);
            double err[7];
            edge_error(s3_mul(C, Si), SjInv, err);
            v[0] += dot7(err);
            if (!jac) continue;
#pragma unroll
            for (int r = 0; r < 7; r++) Q.err[(size_t)e * 7 + r] = err[r];
            if (vi == Q.loop) continue;
#pragma unroll 1
            for (int d = 0; d < 7; d++) {
                double ep[7], em[7];
                edge_error(s3_mul(C, s3_mul(Q.probes[2 * d], Si)), SjInv, ep);
                edge_error(s3_mul(C, s3_mul(Q.probes[2 * d + 1], Si)), SjInv, em);
#pragma unroll
                for (int r = 0; r < 7; r++) Jc[7 * d + r] = scalar * (ep[r] - em[r]);
            }
        } else {
            if (vj == Q.loop) continue;
            const S3 CSi = s3_mul(C, Si);
#pragma unroll 1
            for (int d = 0; d < 7; d++) {
                double ep[7], em[7];
                edge_error(CSi, s3_inverse(s3_mul(Q.probes[2 * d], Sj)), ep);
                edge_error(CSi, s3_inverse(s3_mul(Q.probes[2 * d + 1], Sj)), em);
#pragma unroll
                for (int r = 0; r < 7; r++) Jc[7 * d + r] = scalar * (ep[r] - em[r]);
            }
        }
    }
    lm::block_sum<1, kEgWaves>(v, Q.s_red);
    return v[0];
}

// buildSystem (base_binary_edge.hpp:55-120 with information = I): H's block column f and b's
// entries of vertex f by one wave, the vertex's edges in edge order.  An edge's off-diagonal
// block J_g^T J_f is added by the owner of the later of its two columns.
__device__ __forceinline__ void build_system(const Prob& Q) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int a = lane < 49 ? lane / 7 : lane - 49, c = lane < 49 ? lane % 7 : 0;
    for (int f = wave; f < Q.F; f += kEgWaves) {
        const int v = Q.free_kf[f], f0 = Q.first[f];
        double* col = Q.H + (size_t)Q.col_off[f] * 49;
        if (lane < 49)
            for (int g = f0; g < f; g++) col[(size_t)(g - f0) * 49 + lane] = 0.0;
        double acc = 0.0;
        for (int t = Q.adj_off[v]; t < Q.adj_off[v + 1]; t++) {
            const int ent = Q.adj[t], e = ent >> 1, side = ent & 1;
            const double* Jf = Q.J + ((size_t)e * 2 + side) * 49;
            if (lane < 49) {
                double s = Jf[7 * a] * Jf[7 * c];
#pragma unroll
                for (int r = 1; r < 7; r++) s += Jf[7 * a + r] * Jf[7 * c + r];
                acc += s;
                const int g = Q.free_idx[Q.ev[2 * e + (1 - side)]];
                if (g >= 0 && g < f) {
                    const double* Jg = Q.J + ((size_t)e * 2 + (1 - side)) * 49;
                    double o = Jg[7 * a] * Jf[7 * c];
#pragma unroll
                    for (int r = 1; r < 7; r++) o += Jg[7 * a + r] * Jf[7 * c + r];
                    double* blk = col + (size_t)(g - f0) * 49;
                    blk[lane] = blk[lane] + o;
                }
            } else if (lane < 56) {
                const double* er = Q.err + (size_t)e * 7;
                double s = Jf[7 * a] * -er[0];
#pragma unroll
                for (int r = 1; r < 7; r++) s += Jf[7 * a + r] * -er[r];
                acc += s;
            }
        }
        if (lane < 49)
            col[(size_t)(f - f0) * 49 + lane] = acc;
        else if (lane < 56)
            Q.b[7 * f + a] = acc;
    }
    __syncthreads();
}

__device__ __forceinline__ void return_inputs(const EssGraphArgs& A, const Prob& Q, int k0, int p0, int b, int status) {
    const int tid = threadIdx.x;
    for (int i = tid; i < Q.K * 12; i += kEgThreads) A.kf_Tcw_out[(size_t)k0 * 12 + i] = A.kf_Tcw[(size_t)k0 * 12 + i];
    for (int i = tid; i < Q.P * 3; i += kEgThreads) A.pt_pos_out[(size_t)p0 * 3 + i] = A.pt_pos[(size_t)p0 * 3 + i];
    if (A.Scw_out)
        for (int i = tid; i < Q.K * 8; i += kEgThreads)
            A.Scw_out[(size_t)k0 * 8 + i] = Q.S[((size_t)(i / 8) * 3) * 8 + (i & 7)];
    if (tid == 0) {
        if (A.trace) A.trace[2 * b] = A.trace[2 * b + 1] = 0;
        if (A.chi2) A.chi2[2 * b] = A.chi2[2 * b + 1] = 0.0;
        if (A.ticks) A.ticks[2 * b] = A.ticks[2 * b + 1] = 0;
        A.status[b] = status;
    }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(kEgThreads) void k_essential_graph(EssGraphArgs A) {
    __shared__ double s_red[kEgWaves];
    __shared__ long long s_scan[kEgWaves];
    __shared__ int s_cnt[8];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int k0 = clampi(A.kf_off[b], 0, A.n_kf), e0 = clampi(A.edge_off[b], 0, A.n_edges),
              p0 = clampi(A.pt_off[b], 0, A.n_pt);
    Prob Q;
    Q.K = clampi(A.kf_off[b + 1] - k0, 0, A.n_kf - k0);
    Q.E = clampi(A.edge_off[b + 1] - e0, 0, A.n_edges - e0);
    Q.P = clampi(A.pt_off[b + 1] - p0, 0, A.n_pt - p0);
    Q.loop = A.loop_kf[b];
    Q.F = 0;
    Q.fix_scale = A.fix_scale != 0;
    Q.ev = A.edge_v + (size_t)e0 * 2;
    Q.probes = (const S3*)A.probes;
    Q.S = A.S + (size_t)k0 * 24;
    Q.meas = A.meas + (size_t)e0 * 8;
    Q.J = A.J + (size_t)e0 * 98;
    Q.err = A.err + (size_t)e0 * 7;
    Q.H = A.H + (size_t)b * (size_t)A.max_env_blocks * 49;
    Q.L = A.L + (size_t)b * (size_t)A.max_env_blocks * 49;
    Q.b = A.vec + (size_t)k0 * 28;
    Q.x = Q.b + (size_t)Q.K * 7;
    Q.xs = Q.x + (size_t)Q.K * 7;
    Q.ys = Q.xs + (size_t)Q.K * 7;
    Q.ok = A.edge_ok + e0;
    Q.free_idx = A.free_idx + k0;
    Q.free_kf = A.free_kf + k0;
    Q.first = A.first + k0 + b;
    Q.adj_off = A.adj_off + k0 + b;  // K + 1 entries per problem
    Q.adj = A.adj + (size_t)e0 * 2;
    Q.deg = A.deg + k0;
    Q.rows = A.rows + (size_t)b * (size_t)A.max_env_blocks;
    Q.col_off = A.col_off + k0 + b;
    Q.row_off = A.row_off + k0 + b;
    Q.s_red = s_red;
    const int K = Q.K, E = Q.E, P = Q.P;
    const int32_t* kinds = A.edge_kind + e0;

    // vScw (cc:913-945): the corrected Sim3 where there is one, Sim3(Rcw, tcw, 1) otherwise
    int nbadidx = 0;
    for (int v = tid; v < K; v += kEgThreads) {
        const int c = A.kf_corr[k0 + v];
        S3 s;
        if (c >= 0 && c < A.n_corr) {
            s = s3_load(A.corr_S + (size_t)c * 8);
        } else {
            s = s3_from_tcw(A.kf_Tcw + (size_t)(k0 + v) * 12);
            if (c != -1) nbadidx++;
        }
        double* d = Q.S + (size_t)v * 24;
        s3_store(d, s);
        s3_store(d + 8, s);
        s3_store(d + 16, s);
        Q.deg[v] = 0;
        Q.x[7 * v] = Q.x[7 * v + 1] = Q.x[7 * v + 2] = Q.x[7 * v + 3] = Q.x[7 * v + 4] = Q.x[7 * v + 5] =
            Q.x[7 * v + 6] = 0.0;
    }
    __syncthreads();
    if (Q.loop < 0 || Q.loop >= K) {
        return_inputs(A, Q, k0, p0, b, ORBX_ESSENTIAL_GRAPH_STATUS_NO_FIXED_KF);
        return;
    }

    // The measurements (cc:954-1089) and the degrees
    for (int e = tid; e < E; e += kEgThreads) {
        const int vi = Q.ev[2 * e], vj = Q.ev[2 * e + 1], kind = kinds[e];
        const bool ok = vi >= 0 && vi < K && vj >= 0 && vj < K && vi != vj && (kind == 0 || kind == 1);
        Q.ok[e] = ok;
        if (!ok) {
            nbadidx++;
            continue;
        }
        S3 Si, Sj;
        if (kind == 0) {
            Si = s3_load(Q.S + (size_t)vi * 24);
            Sj = s3_load(Q.S + (size_t)vj * 24);
        } else {
            Si = s3_from_tcw(A.kf_Tcw + (size_t)(k0 + vi) * 12);
            Sj = s3_from_tcw(A.kf_Tcw + (size_t)(k0 + vj) * 12);
        }
        s3_store(Q.meas + (size_t)e * 8, s3_mul(Sj, s3_inverse(Si)));
        atomicAdd(&Q.deg[vi], 1);
        atomicAdd(&Q.deg[vj], 1);
    }
    __syncthreads();
    auto degree = [&](int v) { return __hip_atomic_load(&Q.deg[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };

    // The vertices that may move and have an edge, in mnId order; the adjacency lists
    const int F = block_scan<int>([&](int v) { return v != Q.loop && degree(v) > 0 ? 1 : 0; }, (int*)Q.first, K,
                                  (int*)s_scan);
    Q.F = F;
    __syncthreads();
    for (int v = tid; v < K; v += kEgThreads) {
        const bool fr = v != Q.loop && degree(v) > 0;
        const int f = Q.first[v];
        Q.free_idx[v] = fr ? f : -1;
    }
    __syncthreads();
    for (int v = tid; v < K; v += kEgThreads)
        if (Q.free_idx[v] >= 0) Q.free_kf[Q.free_idx[v]] = v;
    block_scan<int>(degree, (int*)Q.adj_off, K, (int*)s_scan);
    __syncthreads();
    for (int v = tid; v < K; v += kEgThreads) Q.deg[v] = 0;
    __syncthreads();
    for (int e = tid; e < E; e += kEgThreads) {
        if (!Q.ok[e]) continue;
        const int vi = Q.ev[2 * e], vj = Q.ev[2 * e + 1];
        Q.adj[Q.adj_off[vi] + atomicAdd(&Q.deg[vi], 1)] = 2 * e;
        Q.adj[Q.adj_off[vj] + atomicAdd(&Q.deg[vj], 1)] = 2 * e + 1;
    }
    __syncthreads();
    for (int v = tid; v < K; v += kEgThreads)  // into edge order
        sort_ascending(Q.adj + Q.adj_off[v], Q.adj_off[v + 1] - Q.adj_off[v]);
    __syncthreads();

    // The envelope: first[f], the block offsets of the columns, the columns of every block row
    for (int f = tid; f < F; f += kEgThreads) {
        const int v = Q.free_kf[f];
        int m = f;
        for (int t = Q.adj_off[v]; t < Q.adj_off[v + 1]; t++) {
            const int ent = Q.adj[t], g = Q.free_idx[Q.ev[2 * (ent >> 1) + (1 - (ent & 1))]];
            if (g >= 0 && g < m) m = g;
        }
        Q.first[f] = A.dense ? 0 : m;
    }
    __syncthreads();
    const long long blocks = block_scan<long long>([&](int f) { return (long long)(f - Q.first[f] + 1); }, Q.col_off, F, s_scan);
    const int nbad = lm::block_sum_int<kEgWaves>(nbadidx, s_cnt);
    if (blocks > A.max_env_blocks) {
        return_inputs(A, Q, k0, p0, b, ORBX_ESSENTIAL_GRAPH_STATUS_CAPACITY | (nbad > 0 ? ORBX_ESSENTIAL_GRAPH_STATUS_BAD_INDEX : 0));
        return;
    }
    env::row_lists(Q, Q.deg, s_scan);

    // SparseOptimizer::optimize with OptimizationAlgorithmLevenberg, as orbx_optsim3.hip's
    const int max_its = A.iterations > 0 ? A.iterations : 20;
    int its = 0, trials = 0;
    double chi0 = 0.0, chi = 0.0;
    long long t_lin = 0, t_solve = 0;  // A.ticks
    if (F == 0) {
        chi0 = chi = errors(Q, 1, false);
    } else {
        double lam = 0.0, ni = 2.0;
        int nbadit = 0;
        for (int it = 0; it < max_its; it++) {
            const long long c0 = wall_clock64();
            chi = errors(Q, 1, true);
            __syncthreads();
            build_system(Q);
            t_lin += wall_clock64() - c0;
            if (it == 0) {
                chi0 = chi;
                lam = 1e-16;  // setUserLambdaInit, cc:890
                ni = 2.0;
                nbadit = 0;
            }
            const double ini_chi = chi;
            int qmax = 0;
            double rho = 0.0;
            do {
                const long long c1 = wall_clock64();
                const bool ok = env::solve<7, true>(Q, lam);
                __syncthreads();
                t_solve += wall_clock64() - c1;
                // push, oplus (exp(x) * estimate; _fix_scale zeroes the solver's entry in place), computeScale
                double sc[1] = {0.0};
                for (int f = tid; f < F; f += kEgThreads) {
                    double* xv = Q.x + 7 * f;
                    if (Q.fix_scale) xv[6] = 0;
                    const double xf[7] = {xv[0], xv[1], xv[2], xv[3], xv[4], xv[5], xv[6]};
                    double* s = Q.S + (size_t)Q.free_kf[f] * 24 + 8;
                    const S3 cur = s3_load(s);
                    s3_store(s + 8, cur);
                    s3_store(s, s3_mul(s3_exp(xf), cur));
#pragma unroll
                    for (int j = 0; j < 7; j++) sc[0] += xf[j] * (lam * xf[j] + Q.b[7 * f + j]);
                }
                __syncthreads();
                double temp = errors(Q, 1, false);
                if (!ok) temp = DBL_MAX;
                lm::block_sum<1, kEgWaves>(sc, s_red);
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
                } else {
                    lam *= ni;
                    ni *= 2.0;
                    for (int f = tid; f < F; f += kEgThreads) {  // pop
                        double* s = Q.S + (size_t)Q.free_kf[f] * 24 + 8;
                        s3_store(s, s3_load(s + 8));
                    }
                }
                __syncthreads();
                qmax++;
            } while (rho < 0 && qmax < 10);
            trials += qmax;
            its++;
            if (qmax == 10 || rho == 0) break;
            if ((ini_chi - chi) * 1e3 < ini_chi)
                nbadit++;
            else
                nbadit = 0;
            if (nbadit >= 3) break;
        }
    }

    // Recovery (cc:1100-1149)
    for (int v = tid; v < K; v += kEgThreads) {
        const S3 s = s3_load(Q.S + (size_t)v * 24 + 8);
        s3_to_tcw(s, A.kf_Tcw_out + (size_t)(k0 + v) * 12);
        if (A.Scw_out) s3_store(A.Scw_out + (size_t)(k0 + v) * 8, s);
    }
    int nbadpt = 0;
    for (int p = tid; p < P; p += kEgThreads) {
        const int r = A.pt_ref[p0 + p];
        const float* in = A.pt_pos + (size_t)(p0 + p) * 3;
        float* out = A.pt_pos_out + (size_t)(p0 + p) * 3;
        if (r < 0 || r >= K) {
            out[0] = in[0];
            out[1] = in[1];
            out[2] = in[2];
            nbadpt++;
            continue;
        }
        const double* s = Q.S + (size_t)r * 24;
        double cx, cy, cz, wx, wy, wz;
        s3_map(s3_load(s), (double)in[0], (double)in[1], (double)in[2], cx, cy, cz);
        s3_map(s3_inverse(s3_load(s + 8)), cx, cy, cz, wx, wy, wz);
        out[0] = (float)wx;
        out[1] = (float)wy;
        out[2] = (float)wz;
    }
    const int nbad2 = lm::block_sum_int<kEgWaves>(nbadpt, s_cnt);
    if (tid == 0) {
        if (A.trace) {
            A.trace[2 * b] = its;
            A.trace[2 * b + 1] = trials;
        }
        if (A.chi2) {
            A.chi2[2 * b] = chi0;
            A.chi2[2 * b + 1] = chi;
        }
        if (A.ticks) {
            A.ticks[2 * b] = t_lin;
            A.ticks[2 * b + 1] = t_solve;
        }
        A.status[b] = nbad + nbad2 > 0 ? ORBX_ESSENTIAL_GRAPH_STATUS_BAD_INDEX : 0;
    }
}

// the workspace's regions, in order; returns its size
size_t carve(EssGraphArgs& A, int batch, char* base) {
    const size_t nk = (size_t)A.n_kf, ne = (size_t)A.n_edges, nb = (size_t)batch * (size_t)A.max_env_blocks;
    Layout L(up256);
    auto take = [&](auto*& field, size_t count) {
        using T = std::remove_reference_t<decltype(*field)>;
        field = (T*)(base + L.take(count * sizeof(T)));
    };
    take(A.S, nk * 24);
    take(A.meas, ne * 8);
    take(A.J, ne * 98);
    take(A.err, ne * 7);
    take(A.H, nb * 49);
    take(A.L, nb * 49);
    take(A.vec, nk * 28);
    take(A.col_off, nk + batch);
    take(A.row_off, nk + batch);
    take(A.rows, nb);
    take(A.edge_ok, ne);
    take(A.free_idx, nk);
    take(A.free_kf, nk);
    take(A.first, nk + batch);
    take(A.adj_off, nk + batch);
    take(A.adj, ne * 2);
    take(A.deg, nk);
    take(A.ticks, (size_t)batch * 2);
    return L.total();
}

}  // namespace

size_t essential_graph_workspace_bytes(int batch, int n_kf, int n_edges, long long max_env_blocks) {
    EssGraphArgs A{};
    A.n_kf = n_kf;
    A.n_edges = n_edges;
    A.max_env_blocks = max_env_blocks;
    return carve(A, batch, nullptr);
}

hipError_t launch_essential_graph(EssGraphArgs A, int batch, char* workspace, hipStream_t stream) {
    if (batch <= 0) return hipSuccess;
    carve(A, batch, workspace);
    // "essgraph_stamps": problem 0's wall-clock ticks (100 MHz) to stderr (diagnostics only;
    // synchronises the stream)
    const bool stamps = tuning(Tune::EssgraphStamps, 0) > 0;
    const long long* d_ticks = A.ticks;
    if (!stamps) A.ticks = nullptr;
    s3_probe_increments(A.fix_scale != 0, A.probes);
    k_essential_graph<<<batch, kEgThreads, 0, stream>>>(A);
    hipError_t e = hipGetLastError();
    if (stamps && e == hipSuccess) {
        long long t[2] = {0, 0};
        e = hipMemcpyAsync(t, d_ticks, sizeof(t), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e == hipSuccess) fprintf(stderr, "essgraph_stamps: linearisation %lld solve %lld\n", t[0], t[1]);
    }
    return e;
}

}  // namespace orbx
