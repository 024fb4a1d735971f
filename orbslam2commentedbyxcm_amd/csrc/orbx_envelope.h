// orbx_envelope.h -- the block-envelope (skyline) linear system shared by the kernels whose
// reduced system has no cap on its size (orbx_essgraph.hip with 7 x 7 blocks, orbx_globalba.hip
// with 6 x 6 blocks): the workgroup scan and the owner's sort that build index lists from
// integer counters, the row lists of an envelope, and the right-looking block-pivot LDL^T with
// its substitutions.  One 256-thread workgroup works on one system; everything is double and
// every function is inlined into its kernel.  DESIGN.md §4.22 item 4.
//
// Block column f holds the D x D blocks (g, f), g = first[f] .. f, first[f] <= f; fill never
// leaves such an envelope.  Every entry of the factor and of the substitutions receives the
// terms lm::ldlt_solve_block gives it, in its order; the terms left out are exact zeros.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace orbx {
namespace env {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

// Exclusive prefix sums of value(0 .. n-1) into out[0 .. n] (out[n] = the total, also returned
// to every thread), in chunks of the workgroup, in index order.
template <class T, class F>
__device__ __forceinline__ T block_scan(F value, T* out, int n, T* s_scan) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    T carry = 0;
    for (int c0 = 0; c0 < n; c0 += kThreads) {
        const int i = c0 + tid;
        const T v = i < n ? value(i) : (T)0;
        T inc = v;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const T o = __shfl_up(inc, m, 64);
            if (lane >= m) inc += o;
        }
        if (lane == 63) s_scan[wave] = inc;
        __syncthreads();
        T off = carry, total = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) {
            if (w < wave) off += s_scan[w];
            total += s_scan[w];
        }
        if (i < n) out[i] = off + inc - v;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) out[n] = carry;
    return carry;
}

// l[0 .. n) into ascending order in place, by one thread: a heapsort, so that a hub keyframe
// with thousands of edges costs n log n.
__device__ __forceinline__ void sort_ascending(int32_t* l, int n) {
    auto sift = [&](int root, int end) {
        const int key = l[root];
        for (;;) {
            int c = 2 * root + 1;
            if (c >= end) break;
            if (c + 1 < end && l[c + 1] > l[c]) c++;
            if (l[c] <= key) break;
            l[root] = l[c];
            root = c;
        }
        l[root] = key;
    };
    for (int i = n / 2 - 1; i >= 0; i--) sift(i, n);
    for (int end = n - 1; end > 0; end--) {
        const int top = l[0];
        l[0] = l[end];
        l[end] = top;
        sift(0, end);
    }
}

// One system's regions of the workspace.
struct Envelope {
    int F;                 // block columns
    double *H, *L;         // the envelope and its factor (H == L: factored in place)
    double *b, *x, *xs, *ys;
    int32_t *first, *rows;
    long long *col_off, *row_off;
};

template <int D>
__device__ __forceinline__ double* diag_block(const Envelope& Q, double* M, int f) {
    return M + (size_t)(Q.col_off[f] + f - Q.first[f]) * (D * D);
}

// The columns of every block row, from first[] and col_off[].  Block row g holds the columns
// q with first[q] <= g < q: their number is a running sum of +1 at first[q] and -1 at q, and
// one wave per column enters it into its rows.  The order of a row's columns only decides
// which thread works on which block, never the order of an entry's terms, so the lists need
// no sorting.  All of it is linear in the envelope.  deg: F integers of scratch.
__device__ __forceinline__ void row_lists(const Envelope& Q, int32_t* deg, long long* s_scan) {
    const int tid = threadIdx.x, F = Q.F;
    auto degree = [&](int v) { return __hip_atomic_load(&deg[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    for (int g = tid; g < F; g += kThreads) deg[g] = 0;
    __syncthreads();
    for (int q = tid; q < F; q += kThreads)
        if (Q.first[q] < q) {
            atomicAdd(&deg[Q.first[q]], 1);
            atomicAdd(&deg[q], -1);
        }
    __syncthreads();
    block_scan<long long>([&](int g) { return (long long)degree(g); }, Q.row_off, F, s_scan);
    __syncthreads();
    block_scan<long long>([&](int g) { return Q.row_off[g] + degree(g); }, Q.row_off, F, s_scan);
    __syncthreads();
    for (int g = tid; g < F; g += kThreads) deg[g] = 0;
    __syncthreads();
    for (int q = tid >> 6; q < F; q += kWaves)
        for (int g = Q.first[q] + (tid & 63); g < q; g += 64) Q.rows[Q.row_off[g] + atomicAdd(&deg[g], 1)] = q;
    __syncthreads();
}

// (H + lambda I) x = b by the block-envelope LDL^T without pivoting.  Every entry of the
// factor and of the substitutions receives the terms lm::ldlt_solve_block gives it, in its
// order; the terms outside the envelope are exact zeros.  Only a pivot that is exactly zero
// (or not finite) is a failed solve; Q.x is then left as it was.  kCopy: H is kept and the
// factor is made in L; otherwise L holds the system on entry and is factored in place.
template <int D, bool kCopy>
__device__ __forceinline__ bool solve(const Envelope& Q, double lam) {
    constexpr int DD = D * D;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int F = Q.F, n = D * F;
    if (kCopy) {
        const size_t words = (size_t)Q.col_off[F] * DD;
        for (size_t i = tid; i < words; i += kThreads) Q.L[i] = Q.H[i];
        __syncthreads();
    }
    for (int i = tid; i < n; i += kThreads) {
        const int f = i / D, r = i - D * f;
        double* dd = diag_block<D>(Q, Q.L, f) + (D + 1) * r;
        *dd = *dd + lam;
        Q.xs[i] = Q.b[i];
    }
    __syncthreads();
    // The factorisation and the forward substitution, one block pivot at a time
    for (int g = 0; g < F; g++) {
        // the pivot block, by every thread: the D scalar pivots in order
        double U[D][D], d[D], y[D];
        {
            const double* blk = diag_block<D>(Q, Q.L, g);
#pragma unroll
            for (int r = 0; r < D; r++)
#pragma unroll
                for (int k = r; k < D; k++) U[r][k] = blk[D * r + k];
        }
        bool ok = true;
#pragma unroll
        for (int r = 0; r < D; r++) {
            d[r] = U[r][r];
            if (d[r] == 0.0 || !isfinite(d[r])) ok = false;
#pragma unroll
            for (int k = r + 1; k < D; k++) U[r][k] = U[r][k] / d[r];
#pragma unroll
            for (int i = r + 1; i < D; i++)
#pragma unroll
                for (int k = i; k < D; k++) U[i][k] = U[i][k] - U[r][i] * U[r][k] * d[r];
        }
        if (!ok) return false;  // the same for every thread
#pragma unroll
        for (int r = 0; r < D; r++) {
            double t = Q.xs[D * g + r];
#pragma unroll
            for (int k = 0; k < r; k++) t = t - U[k][r] * y[k];
            y[r] = t;
        }
        // block row g: one thread per scalar column of the columns that reach up to g
        const long long r0 = Q.row_off[g];
        const int m = (int)(Q.row_off[g + 1] - r0);
        for (int w = tid; w < D * m; w += kThreads) {
            const int q = Q.rows[r0 + w / D], cc = w % D;
            double* blk = Q.L + (size_t)(Q.col_off[q] + g - Q.first[q]) * DD + cc;
            double u[D];
#pragma unroll
            for (int r = 0; r < D; r++) u[r] = blk[D * r];
#pragma unroll
            for (int r = 0; r < D; r++) {
                u[r] = u[r] / d[r];
#pragma unroll
                for (int i = r + 1; i < D; i++) u[i] = u[i] - U[r][i] * u[r] * d[r];
            }
            double t = Q.xs[D * q + cc];
#pragma unroll
            for (int r = 0; r < D; r++) {
                blk[D * r] = u[r];
                t = t - u[r] * y[r];
            }
            Q.xs[D * q + cc] = t;
        }
        __syncthreads();
        if (tid == 0) {
            double* blk = diag_block<D>(Q, Q.L, g);
#pragma unroll
            for (int r = 0; r < D; r++) {
                blk[(D + 1) * r] = d[r];
#pragma unroll
                for (int k = r + 1; k < D; k++) blk[D * r + k] = U[r][k];
                Q.ys[D * g + r] = y[r];
            }
        }
        // the trailing blocks (qa, qb), qa <= qb, of the row's columns: one wave each
        const long long pairs = (long long)m * (m + 1) / 2;
        for (long long p = wave; p < pairs; p += kWaves) {
            long long ib = (long long)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
            while (ib * (ib + 1) / 2 > p) ib--;
            while ((ib + 1) * (ib + 2) / 2 <= p) ib++;
            const long long ia = p - ib * (ib + 1) / 2;
            if (lane >= DD) continue;
            const int ra = lane / D, cb = lane % D;
            if (ia == ib && ra > cb) continue;
            int qa = Q.rows[r0 + ia], qb = Q.rows[r0 + ib];
            if (qa > qb) {  // a row's columns are in no particular order
                const int q = qa;
                qa = qb;
                qb = q;
            }
            const double* ua = Q.L + (size_t)(Q.col_off[qa] + g - Q.first[qa]) * DD + ra;
            const double* ub = Q.L + (size_t)(Q.col_off[qb] + g - Q.first[qb]) * DD + cb;
            double* tgt = Q.L + (size_t)(Q.col_off[qb] + qa - Q.first[qb]) * DD + lane;
            double t = *tgt;
#pragma unroll
            for (int r = 0; r < D; r++) t = t - ua[D * r] * ub[D * r] * d[r];
            *tgt = t;
        }
        __syncthreads();
    }
    for (int i = tid; i < n; i += kThreads) {
        const int f = i / D, r = i - D * f;
        Q.xs[i] = Q.ys[i] / diag_block<D>(Q, Q.L, f)[(D + 1) * r];
    }
    __syncthreads();
    // The back substitution, one block column at a time, the columns descending
    for (int f = F - 1; f >= 0; f--) {
        const double* blk = diag_block<D>(Q, Q.L, f);
        double xf[D];
#pragma unroll
        for (int cc = D - 1; cc >= 0; cc--) {
            double t = Q.xs[D * f + cc];
#pragma unroll
            for (int k = D - 1; k > cc; k--) t = t - blk[D * cc + k] * xf[k];
            xf[cc] = t;
        }
        if (tid == 0) {
#pragma unroll
            for (int cc = 0; cc < D; cc++) Q.x[D * f + cc] = xf[cc];
        }
        const int f0 = Q.first[f];
        const double* col = Q.L + (size_t)Q.col_off[f] * DD;
        for (int w = tid; w < D * (f - f0); w += kThreads) {
            const double* u = col + (size_t)(w / D) * DD + D * (w % D);
            double t = Q.xs[D * f0 + w];
#pragma unroll
            for (int cc = D - 1; cc >= 0; cc--) t = t - u[cc] * xf[cc];
            Q.xs[D * f0 + w] = t;
        }
        __syncthreads();
    }
    return true;
}

}  // namespace env
}  // namespace orbx
