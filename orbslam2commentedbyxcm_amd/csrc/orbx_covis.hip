// orbx_covis.hip -- the covisibility graph in HBM: MapPoint::GetObservations() as a CSR over
// MapPoint ids, KeyFrame::UpdateConnections / AddConnection / UpdateBestCovisibles /
// EraseConnection (KeyFrame.cc:139-182, 324-415, 506-520, 607-620) with the per-keyframe lists
// that GetVectorCovisibleKeyFrames, GetBestCovisibilityKeyFrames and GetCovisiblesByWeight read,
// and the graph assembly of Optimizer::LocalBundleAdjustment (Optimizer.cc:526-583, 656-760).
// DESIGN.md 4.24.
//
// Everything is integer work; the keyframe id stands in for the reference's KeyFrame* wherever
// the reference's order is a pointer order.  Integer atomics count; every stored byte is then
// put in an order that does not depend on scheduling (segments ranked by keyframe id, rows
// compacted in ascending id, lists sorted on (weight << 32 | id) keys by orbx_block_sort.h).
// No workgroup waits on another.
//
// Refresh (four launches):
//   k_covis_clean  one 1024-thread workgroup per keyframe row sorts (MapPoint id << 32 | index)
//                  keys; the first key of a run keeps the observation, the others become NULL
//                  in the cleaned copy of the row and set DUPLICATE; a row that is not bad counts
//                  its points
//   k_covis_scan   one workgroup: exclusive scan of the counts -> obs_off
//   k_covis_fill   one thread per slot: the observers of a point in arrival order (atomic cursor)
//   k_covis_rank   one thread per slot: its rank among the point's observers by keyframe id is
//                  its place in the segment
// UpdateConnections (two launches; the batch's ids come from the host, or, for CorrectLoop's
// members, ids and count stay on the device):
//   k_covis_update one workgroup per query keyframe: histogram over keyframe ids -- in LDS when
//                  max_keyframes <= the bound (ORBX_COVIS_LDS_KEYFRAMES, "covis_lds_keyframes"),
//                  else in a zeroed global row --, compaction to the sparse row, the thresholded
//                  list, the parent
//   k_covis_merge  one workgroup per keyframe that the batch did not rewrite: looks itself up
//                  in the fresh rows (binary search), merges the AddConnection messages into its
//                  dense row and, only if an entry is new or differs, re-orders its whole row
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "orbx.h"
#include "orbx_block_sort.h"
#include "orbx_covis.h"
#include "orbx_host.h"

namespace orbx {
namespace {

constexpr int kCvGroups = 128;     // workgroups of a launch that takes a global dense row each
constexpr int kCvMaxKeyframes = 1 << 20;

__device__ __forceinline__ int* cv_dense(const CovisDev& D, unsigned long long* s_dyn) {
    return D.dense_lds ? (int*)(s_dyn + kSortMaxKeys) : D.ws + (size_t)blockIdx.x * D.K;
}

__global__ __launch_bounds__(kCvThreads) void k_covis_clean(CovisDev D, const int32_t* kf_mp) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_dyn[];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int nq = clampi(D.kf_n[q], 0, D.cap);
    const bool bad = D.kf_bad && D.kf_bad[q];
    const size_t r0 = (size_t)q * D.cap;
    for (int i = tid; i < D.cap; i += kCvThreads) D.clean[r0 + i] = -1;
    int np = kSortThreads;
    while (np < nq) np <<= 1;
    const int ne = np / kSortThreads;
    unsigned long long r[kSortPer];
#pragma unroll
    for (int e = 0; e < kSortPer; e++) {
        r[e] = ~0ull;
        const int i = e * kSortThreads + tid;
        if (e < ne && i < nq) {
            const int p = kf_mp[r0 + i];
            if (p >= 0 && p < D.nm) r[e] = (unsigned long long)(unsigned)p << 32 | (unsigned)i;
        }
    }
    block_bitonic_sort64(r, ne, s_dyn);  // ends with a barrier: the -1 fill is complete too
    int dup = 0;
    for (int j = tid; j < np; j += kCvThreads) {
        const unsigned long long key = s_dyn[j];
        if (key == ~0ull) continue;
        const int p = (int)(unsigned)(key >> 32), i = (int)(unsigned)(key & 0xFFFFFFFFull);
        if (j > 0 && (int)(unsigned)(s_dyn[j - 1] >> 32) == p) {
            dup = 1;  // a lower index holds the observation
            continue;
        }
        D.clean[r0 + i] = p;
        if (!bad) atomicAdd(&D.obs_cnt[p], 1);
    }
    dup = __syncthreads_or(dup);
    if (tid == 0) D.status[q] = (D.status[q] & ~ORBX_COVIS_STATUS_DUPLICATE) | (dup ? ORBX_COVIS_STATUS_DUPLICATE : 0);
}

__global__ __launch_bounds__(kCvThreads) void k_covis_scan(CovisDev D) {
    __shared__ int s_w[kCvWaves];
    const int tid = threadIdx.x;
    int base = 0;
    for (int p0 = 0; p0 < D.nm; p0 += kCvThreads) {
        const int p = p0 + tid;
        const int c = p < D.nm ? D.obs_cnt[p] : 0;
        int tot;
        const int pos = cv_block_scan(c, s_w, tot);
        if (p < D.nm) {
            D.obs_off[p] = base + pos;
            D.obs_cnt[p] = 0;
        }
        base += tot;
    }
    if (tid == 0) D.obs_off[D.nm] = base;
}

__global__ void k_covis_fill(CovisDev D) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= (long long)D.nk * D.cap) return;
    const int q = (int)(s / D.cap);
    if (D.kf_bad && D.kf_bad[q]) return;
    const int p = D.clean[s];
    if (p < 0) return;
    D.tmp_kf[D.obs_off[p] + atomicAdd(&D.obs_cnt[p], 1)] = q;
}

__global__ void k_covis_rank(CovisDev D) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= (long long)D.nk * D.cap) return;
    const int q = (int)(s / D.cap), i = (int)(s - (long long)q * D.cap);
    if (D.kf_bad && D.kf_bad[q]) return;
    const int p = D.clean[s];
    if (p < 0) return;
    const int o0 = D.obs_off[p], o1 = D.obs_off[p + 1];
    int rank = 0;
    for (int o = o0; o < o1; o++) rank += D.tmp_kf[o] < q;
    D.obs_kf[o0 + rank] = q;
    D.obs_idx[o0 + rank] = i;
}

__global__ __launch_bounds__(kCvThreads) void k_covis_update(CovisDev D, const int32_t* ids, int Q, const int32_t* d_Q) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_dyn[];
    __shared__ CvScratch S;
    const int tid = threadIdx.x;
    if (d_Q) Q = clampi(*d_Q, 0, Q);  // the batch's size lives on the device
    int* dense = cv_dense(D, s_dyn);
    for (int b = blockIdx.x; b < Q; b += gridDim.x) {
        const int q = ids[b];
        if (q < D.nk && D.kf_bad && D.kf_bad[q]) {  // uniform
            if (tid == 0) D.status[q] |= ORBX_COVIS_STATUS_BAD_KEYFRAME;
            continue;
        }
        for (int k = tid; k < D.K; k += kCvThreads) dense[k] = 0;
        __syncthreads();
        const int nq = q < D.nk ? clampi(D.kf_n[q], 0, D.cap) : 0;
        for (int i = tid; i < nq; i += kCvThreads) {
            const int p = D.clean[(size_t)q * D.cap + i];
            if (p < 0 || (D.mp_bad && D.mp_bad[p])) continue;  // cc:337-341
            const int o1 = D.obs_off[p + 1];
            for (int o = D.obs_off[p]; o < o1; o++) {
                const int kf = D.obs_kf[o];
                if (kf != q) atomicAdd(&dense[kf], 1);  // cc:348-351
            }
        }
        __syncthreads();
        int m, n15, kfmax;
        cv_dense_to_row(D, q, dense, S, m, n15, kfmax);
        if (m == 0) continue;  // cc:356
        if (m > D.max_conn) {
            if (tid == 0) D.status[q] |= ORBX_COVIS_STATUS_CAPACITY;
            continue;
        }
        const int front = cv_order_row(D, q, m, false, n15, kfmax, s_dyn);
        if (tid == 0) {
            D.kmax[q] = n15 == 0 ? kfmax : -1;
            D.fresh[q] = 1;
            if (D.first[q] && q != 0) {  // cc:407-413
                D.parent[q] = front;
                D.first[q] = 0;
            }
        }
    }
}

__global__ __launch_bounds__(kCvThreads) void k_covis_merge(CovisDev D, const int32_t* ids, int Q, const int32_t* d_Q) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_dyn[];
    __shared__ CvScratch S;
    const int tid = threadIdx.x;
    if (d_Q) Q = clampi(*d_Q, 0, Q);
    int* dense = cv_dense(D, s_dyn);
    for (int t = blockIdx.x; t < D.K; t += gridDim.x) {
        if (D.fresh[t]) continue;
        int any = 0;
        for (int b = tid; b < Q; b += kCvThreads) {
            const int q = ids[b];
            if (!D.fresh[q]) continue;
            const int w = cv_row_lookup(D, q, t);
            any |= w >= kCvTh || (w > 0 && D.kmax[q] == t);  // cc:376-387
        }
        if (!__syncthreads_or(any)) continue;
        for (int k = tid; k < D.K; k += kCvThreads) dense[k] = 0;
        __syncthreads();
        const size_t r0 = (size_t)t * D.max_conn;
        for (int j = tid; j < D.row_n[t]; j += kCvThreads) dense[D.row_kf[r0 + j]] = D.row_w[r0 + j];
        __syncthreads();
        int changed = 0;
        for (int b = tid; b < Q; b += kCvThreads) {  // AddConnection, cc:139-149; the ids differ
            const int q = ids[b];
            if (!D.fresh[q]) continue;
            const int w = cv_row_lookup(D, q, t);
            if ((w >= kCvTh || (w > 0 && D.kmax[q] == t)) && dense[q] != w) {
                dense[q] = w;
                changed = 1;
            }
        }
        if (!__syncthreads_or(changed)) continue;
        int m, n15, kfmax;
        cv_dense_to_row(D, t, dense, S, m, n15, kfmax);
        if (m > D.max_conn) {
            if (tid == 0) D.status[t] |= ORBX_COVIS_STATUS_CAPACITY;
            continue;
        }
        cv_order_row(D, t, m, true, 0, -1, s_dyn);
    }
}

__global__ __launch_bounds__(kCvThreads) void k_covis_erase(CovisDev D, int id) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_dyn[];
    __shared__ CvScratch S;
    const int tid = threadIdx.x;
    int* dense = cv_dense(D, s_dyn);
    const int nrow = D.row_n[id];
    for (int j = blockIdx.x; j < nrow; j += gridDim.x) {
        const int t = D.row_kf[(size_t)id * D.max_conn + j];
        if (t == id || cv_row_lookup(D, t, id) == 0) continue;  // cc:612: nothing held, nothing re-ordered
        for (int k = tid; k < D.K; k += kCvThreads) dense[k] = 0;
        __syncthreads();
        const size_t r0 = (size_t)t * D.max_conn;
        for (int i = tid; i < D.row_n[t]; i += kCvThreads)
            if (D.row_kf[r0 + i] != id) dense[D.row_kf[r0 + i]] = D.row_w[r0 + i];
        __syncthreads();
        int m, n15, kfmax;
        cv_dense_to_row(D, t, dense, S, m, n15, kfmax);
        if (m == 0) {
            if (tid == 0) {
                D.row_n[t] = 0;
                D.ord_n[t] = 0;
            }
            continue;
        }
        cv_order_row(D, t, m, true, 0, -1, s_dyn);
    }
}

__global__ void k_covis_clear(CovisDev D, int id) {  // cc:519-520
    D.row_n[id] = 0;
    D.ord_n[id] = 0;
}

__global__ void k_covis_best(CovisDev D, int N, int32_t* out, int32_t* out_n) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= (long long)D.K * N) return;
    const int k = (int)(s / N), j = (int)(s - (long long)k * N);
    const int c = D.ord_n[k] < N ? D.ord_n[k] : N;  // cc:203-208
    out[s] = j < c ? D.ord_kf[(size_t)k * D.max_conn + j] : -1;
    if (j == 0) out_n[k] = c;
}

__global__ void k_covis_by_weight(CovisDev D, int w, int32_t* out, int32_t* out_n) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= D.K) return;
    const size_t r0 = (size_t)k * D.max_conn;
    const int c = D.ord_n[k];
    int n = 0;
    if (c > 0) {
        // upper_bound(w, weightComp = a > b): the first weight with w > weight (cc:218-220)
        int lo = 0, hi = c;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (w > D.ord_w[r0 + mid]) hi = mid;
            else lo = mid + 1;
        }
        n = (lo == c && D.ord_w[r0 + c - 1] < w) ? 0 : lo;  // cc:222
    }
    out_n[k] = n;
    if (out)
        for (int j = 0; j < D.max_conn; j++) out[r0 + j] = j < n ? D.ord_kf[r0 + j] : -1;
}


// ---- Optimizer::LocalBundleAdjustment's graph assembly (Optimizer.cc:526-583, 656-760) ----
// One workgroup per problem, twice: a counting launch, a one-thread scan over the problems that
// lays them out against the capacities, and the writing launch.  Marks per MapPoint / keyframe
// (INT_MAX = none) live in a workspace row per workgroup and are reset before the next problem:
//   pmark[p]  the first slot (position in lLocalKeyFrames * cap + index) that names point p
//   kmark[kf] -(row + 2) once the keyframe has a row, -1 for a bad neighbour (marked, no row),
//             else the first edge (in lLocalMapPoints order, observers ascending) that names it
constexpr int kAsmGroups = 64;
constexpr int kAsmNone = INT_MAX;

__device__ void cv_assemble(const CovisDev& D, const orbx_local_ba_assembly& A, const AsmWs& W, int b, int cur, bool write, int* s_w) {
    const int tid = threadIdx.x;
    int* pmark = W.pmark + (size_t)blockIdx.x * D.n;
    int* kmark = W.kmark + (size_t)blockIdx.x * D.K;
    int* loc = W.loc + (size_t)blockIdx.x * (D.max_conn + 1);
    const int k0 = write ? W.base[3 * b] : 0, p0 = write ? W.base[3 * b + 1] : 0, o0 = write ? W.base[3 * b + 2] : 0;
    const size_t c0 = (size_t)cur * D.max_conn;
    const int nn = D.ord_n[cur];
    // lLocalKeyFrames: pKF, then its GetVectorCovisibleKeyFrames() without the bad ones (cc:528-539)
    if (tid == 0) {
        loc[0] = cur;
        cv_st(kmark + cur, -2);
    }
    int nl = 1;
    for (int j0 = 0; j0 < nn; j0 += kCvThreads) {
        const int j = j0 + tid;
        const int kf = j < nn ? D.ord_kf[c0 + j] : -1;
        const bool good = kf >= 0 && kf != cur && !(kf < D.nk && D.kf_bad && D.kf_bad[kf]);
        int tot;
        const int pos = cv_block_scan(good, s_w, tot);
        if (kf >= 0 && kf != cur) cv_st(kmark + kf, good ? -(nl + pos + 2) : -1);
        if (good) loc[nl + pos] = kf;
        nl += tot;
    }
    __syncthreads();
    if (write)
        for (int l = tid; l < nl; l += kCvThreads) {
            const int kf = loc[l];
            A.kf_id[k0 + l] = kf;
            A.kf_slot[k0 + l] = kf;
            A.kf_fixed[k0 + l] = kf == 0;
            for (int c = 0; c < 12; c++) A.kf_Tcw[(size_t)(k0 + l) * 12 + c] = A.kf_pose[(size_t)kf * 12 + c];
        }
    // lLocalMapPoints: the first slot that names a point (cc:544-561)
    const long long slots = (long long)nl * D.cap;
    auto point_at = [&](long long s) -> int {
        const int l = (int)(s / D.cap), i = (int)(s - (long long)l * D.cap), kf = loc[l];
        if (kf >= D.nk || i >= clampi(D.kf_n[kf], 0, D.cap)) return -1;
        const int p = D.clean[(size_t)kf * D.cap + i];
        return p < 0 || (D.mp_bad && D.mp_bad[p]) ? -1 : p;
    };
    for (long long s = tid; s < slots; s += kCvThreads) {
        const int p = point_at(s);
        if (p >= 0) atomicMin(pmark + p, (int)s);
    }
    __syncthreads();
    // points in order, their edge offsets, and the first edge that names each keyframe without a row
    int np = 0, ne = 0;
    for (long long s0 = 0; s0 < slots; s0 += kCvThreads) {
        const long long s = s0 + tid;
        const int p = s < slots ? point_at(s) : -1;
        const bool win = p >= 0 && cv_ld(pmark + p) == (int)s;
        const int a = win ? D.obs_off[p] : 0, deg = win ? D.obs_off[p + 1] - a : 0;
        int tp, te;
        const int j = np + cv_block_scan(win, s_w, tp), e = ne + cv_block_scan(deg, s_w, te);
        if (win) {
            for (int k = 0; k < deg; k++) {
                const int kf = D.obs_kf[a + k];
                if (cv_ld(kmark + kf) >= 0) atomicMin(kmark + kf, e + k);  // cc:576
            }
            if (write) {
                A.pt_id[p0 + j] = p;
                A.obs_off[p0 + j] = o0 + e;
                for (int c = 0; c < 3; c++) A.pt_pos[(size_t)(p0 + j) * 3 + c] = A.mp_pos[(size_t)p * 3 + c];
            }
        }
        np += tp;
        ne += te;
    }
    __syncthreads();
    // lFixedCameras in the order of the walk (cc:566-583)
    int nf = 0;
    ne = 0;
    for (long long s0 = 0; s0 < slots; s0 += kCvThreads) {
        const long long s = s0 + tid;
        const int p = s < slots ? point_at(s) : -1;
        const bool win = p >= 0 && cv_ld(pmark + p) == (int)s;
        const int a = win ? D.obs_off[p] : 0, deg = win ? D.obs_off[p + 1] - a : 0;
        int te, tf;
        const int e = ne + cv_block_scan(deg, s_w, te);
        int mine = 0;
        for (int k = 0; k < deg; k++) mine += cv_ld(kmark + D.obs_kf[a + k]) == e + k;
        int f = nf + cv_block_scan(mine, s_w, tf);
        for (int k = 0; k < deg && mine; k++) {
            const int kf = D.obs_kf[a + k];
            if (cv_ld(kmark + kf) != e + k) continue;
            const int row = nl + f++;
            cv_st(kmark + kf, -(row + 2));
            if (write) {
                A.kf_id[k0 + row] = kf;
                A.kf_slot[k0 + row] = kf;
                A.kf_fixed[k0 + row] = 1;
                for (int c = 0; c < 12; c++) A.kf_Tcw[(size_t)(k0 + row) * 12 + c] = A.kf_pose[(size_t)kf * 12 + c];
            }
        }
        ne += te;
        nf += tf;
    }
    __syncthreads();
    if (!write && tid == 0) {
        W.raw[3 * b] = nl + nf;
        W.raw[3 * b + 1] = np;
        W.raw[3 * b + 2] = ne;
    }
    // the edges (cc:656-760), then the marks back to none
    ne = 0;
    for (long long s0 = 0; s0 < slots; s0 += kCvThreads) {
        const long long s = s0 + tid;
        const int p = s < slots ? point_at(s) : -1;
        const bool win = p >= 0 && cv_ld(pmark + p) == (int)s;
        const int a = win ? D.obs_off[p] : 0, deg = win ? D.obs_off[p + 1] - a : 0;
        int te;
        const int e = ne + cv_block_scan(deg, s_w, te);
        if (write)
            for (int k = 0; k < deg; k++) {
                A.obs_kf[o0 + e + k] = -(cv_ld(kmark + D.obs_kf[a + k]) + 2);
                A.obs_kp[o0 + e + k] = D.obs_idx[a + k];
            }
        ne += te;
    }
    __syncthreads();
    for (long long s = tid; s < slots; s += kCvThreads) {
        const int p = point_at(s);
        if (p < 0 || cv_ld(pmark + p) != (int)s) continue;
        for (int o = D.obs_off[p]; o < D.obs_off[p + 1]; o++) cv_st(kmark + D.obs_kf[o], kAsmNone);
    }
    __syncthreads();
    for (long long s = tid; s < slots; s += kCvThreads) {
        const int p = point_at(s);
        if (p >= 0) cv_st(pmark + p, kAsmNone);
    }
    for (int j = tid; j < nn; j += kCvThreads) cv_st(kmark + D.ord_kf[c0 + j], kAsmNone);
    if (tid == 0) cv_st(kmark + cur, kAsmNone);
    __syncthreads();
}

__global__ __launch_bounds__(kCvThreads) void k_covis_assemble(CovisDev D, orbx_local_ba_assembly A, AsmWs W, const int32_t* cur, int write) {
    __shared__ int s_w[kCvWaves];
    for (int b = blockIdx.x; b < A.batch; b += gridDim.x) {
        if (write && (A.status[b] & ORBX_LOCAL_BA_STATUS_CAPACITY)) continue;  // uniform
        cv_assemble(D, A, W, b, cur[b], write != 0, s_w);
    }
}

// One thread lays the problems out in order: one that does not fit what is left gets empty ranges
// and CAPACITY, the others go where they would without it.
__global__ void k_covis_layout(orbx_local_ba_assembly A, AsmWs W) {
    int k = 0, p = 0, o = 0;
    for (int b = 0; b < A.batch; b++) {
        const int nk = W.raw[3 * b], np = W.raw[3 * b + 1], no = W.raw[3 * b + 2];
        const bool fits = k + nk <= A.max_kf_rows && p + np <= A.max_pt_rows && o + no <= A.max_obs;
        A.kf_off[b] = k;
        A.pt_off[b] = p;
        W.base[3 * b] = k;
        W.base[3 * b + 1] = p;
        W.base[3 * b + 2] = o;
        A.status[b] = fits ? 0 : ORBX_LOCAL_BA_STATUS_CAPACITY;
        A.counts[3 * b] = fits ? nk : 0;
        A.counts[3 * b + 1] = fits ? np : 0;
        A.counts[3 * b + 2] = fits ? no : 0;
        if (fits) {
            k += nk;
            p += np;
            o += no;
        }
    }
    A.kf_off[A.batch] = k;
    A.pt_off[A.batch] = p;
    A.obs_off[p] = o;
}

// the index part of Optimizer.cc:828-853
__global__ void k_covis_apply_kf(orbx_local_ba_apply A) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= A.kf_off[A.batch] || A.kf_fixed[r]) return;
    const int kf = A.kf_id[r];
    if (kf < 0 || kf >= A.n_keyframes) return;
    for (int c = 0; c < 12; c++) A.kf_pose[(size_t)kf * 12 + c] = A.kf_Tcw_opt[(size_t)r * 12 + c];
}

__global__ void k_covis_apply_pt(orbx_local_ba_apply A) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= A.pt_off[A.batch]) return;
    const int p = A.pt_id[j];
    if (p >= 0 && p < A.n_mappoints)
        for (int c = 0; c < 3; c++) A.mp_pos[(size_t)p * 3 + c] = A.pt_pos_opt[(size_t)j * 3 + c];
    if (!A.erase || !A.kf_mp) return;
    int lo = 0, hi = A.batch;  // the problem of point j: the last b with pt_off[b] <= j
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (A.pt_off[mid] <= j) lo = mid;
        else hi = mid;
    }
    const int k0 = A.kf_off[lo], nk = A.kf_off[lo + 1] - k0;
    for (int o = A.obs_off[j]; o < A.obs_off[j + 1]; o++) {
        if (!A.erase[o]) continue;
        const int r = A.obs_kf[o], kp = A.obs_kp[o];
        if (r < 0 || r >= nk || kp < 0 || kp >= A.cap) continue;
        const int kf = A.kf_id[k0 + r];
        if (kf >= 0 && kf < A.n_keyframes) A.kf_mp[(size_t)kf * A.cap + kp] = -1;  // EraseMapPointMatch
    }
}

}  // namespace
}  // namespace orbx

namespace {

using namespace orbx;

void free_covis(orbx_covis* h) {
    for (void* p : h->allocs)
        if (p) (void)hipFree(p);
    h->asm_batch.release();
    h->host_map.release();
    h->lm_ws_buf.release();
    h->lm_batch.release();
    h->lm_host.release();
    if (h->stream) (void)hipStreamDestroy(h->stream);
}

template <class K>
int set_lds(K kern, size_t lds) {
    HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return ORBX_OK;
}

int dense_grid(const orbx_covis* h, int items) { return h->D.dense_lds ? items : std::min(items, kCvGroups); }

// UpdateConnections of the Q keyframes ids[] (a device array; at most *d_Q of them when d_Q is given)
int launch_update(orbx_covis* h, const int32_t* ids, int Q, const int32_t* d_Q, hipStream_t s) {
    const CovisDev& D = h->D;
    HIP_TRY(hipMemsetAsync(D.fresh, 0, (size_t)D.K, s));
    static thread_local bool attr = false;
    if (!attr) {
        const size_t most = (size_t)kSortMaxKeys * 8 + (size_t)ORBX_COVIS_LDS_KEYFRAMES * 4;
        int rc;
        if ((rc = set_lds(k_covis_update, most)) || (rc = set_lds(k_covis_merge, most))) return rc;
        attr = true;
    }
    k_covis_update<<<dense_grid(h, Q), kCvThreads, h->lds, s>>>(D, ids, Q, d_Q);
    HIP_TRY(hipGetLastError());
    k_covis_merge<<<dense_grid(h, D.K), kCvThreads, h->lds, s>>>(D, ids, Q, d_Q);
    HIP_TRY(hipGetLastError());
    return ORBX_OK;
}

}  // namespace

namespace orbx {

int covis_update_ids_device(orbx_covis* h, const int32_t* d_ids, const int32_t* d_n, int max_q, hipStream_t s) {
    return max_q > 0 ? launch_update(h, d_ids, max_q, d_n, s) : ORBX_OK;
}

}  // namespace orbx

extern "C" {

int orbx_covis_create(int device, int max_keyframes, int cap, int max_mappoints, int max_conn, orbx_covis** out) {
    if (!out) return fail(ORBX_ERR_ARG, "null argument");
    *out = nullptr;
    if (device < 0 || max_keyframes < 1 || cap < 1 || max_mappoints < 1 || max_conn < 1)
        return fail(ORBX_ERR_ARG, "bad argument");
    if (max_conn > ORBX_COVIS_MAX_CONN) return fail(ORBX_ERR_ARG, "max_conn above 8192");
    if (cap > kSortMaxKeys) return fail(ORBX_ERR_ARG, "cap above 8192");
    if (max_keyframes > kCvMaxKeyframes || (long long)max_keyframes * cap > INT_MAX ||
        (long long)max_keyframes * max_conn > INT_MAX)
        return fail(ORBX_ERR_ARG, "map too large");
    orbx_covis* h = new (std::nothrow) orbx_covis();
    if (!h) return fail(ORBX_ERR_ARG, "out of host memory");
    CovisDev& D = h->D;
    h->device = device;
    D.K = max_keyframes;
    D.cap = cap;
    D.n = max_mappoints;
    D.max_conn = max_conn;
    const int bound = tuning(Tune::CovisLdsKeyframes, ORBX_COVIS_LDS_KEYFRAMES);
    D.dense_lds = max_keyframes <= std::min(bound, ORBX_COVIS_LDS_KEYFRAMES);
    h->lds = (size_t)kSortMaxKeys * 8 + (D.dense_lds ? (size_t)max_keyframes * 4 : 0);
    const size_t K = (size_t)max_keyframes, slots = K * cap, conn = K * max_conn;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    auto alloc = [&](auto** p, size_t bytes, int fill) {
        if (e != hipSuccess) return;
        void* v = nullptr;
        e = hipMalloc(&v, bytes ? bytes : 4);
        if (e != hipSuccess) return;
        h->allocs.push_back(v);
        *p = (std::remove_reference_t<decltype(**p)>*)v;
        e = hipMemsetAsync(v, fill, bytes ? bytes : 4, h->stream);
    };
    alloc(&D.clean, slots * 4, 0xFF);
    alloc(&D.obs_off, ((size_t)max_mappoints + 1) * 4, 0);
    alloc(&D.obs_cnt, (size_t)max_mappoints * 4, 0);
    alloc(&D.obs_kf, slots * 4, 0);
    alloc(&D.obs_idx, slots * 4, 0);
    alloc(&D.tmp_kf, slots * 4, 0);
    alloc(&D.row_kf, conn * 4, 0);
    alloc(&D.row_w, conn * 4, 0);
    alloc(&D.row_n, K * 4, 0);
    alloc(&D.ord_kf, conn * 4, 0);
    alloc(&D.ord_w, conn * 4, 0);
    alloc(&D.ord_n, K * 4, 0);
    alloc(&D.parent, K * 4, 0xFF);
    alloc(&D.first, K, 1);
    alloc(&D.status, K * 4, 0);
    alloc(&D.kmax, K * 4, 0xFF);
    alloc(&D.fresh, K, 0);
    alloc(&D.ws, D.dense_lds ? 0 : (size_t)kCvGroups * K * 4, 0);
    alloc(&h->ids, K * 4, 0);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) {
        free_covis(h);
        delete h;
        set_last_error(std::string("orbx_covis_create: ") + hipGetErrorString(e));
        return ORBX_ERR_HIP;
    }
    *out = h;
    return ORBX_OK;
}

void orbx_covis_destroy(orbx_covis* h) {
    if (!h || orbx::unloading()) return;
    (void)hipSetDevice(h->device);
    if (h->last) (void)hipStreamSynchronize(h->last);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    free_covis(h);
    delete h;
}

void* orbx_covis_stream(orbx_covis* h) { return h ? (void*)h->stream : nullptr; }

int orbx_covis_refresh_observations_device(orbx_covis* h, int n_keyframes, const int32_t* kf_mp, const int32_t* kf_n,
                                           const uint8_t* kf_bad, int n_mappoints, const uint8_t* mp_bad, void* stream) {
    if (!h) return fail(ORBX_ERR_ARG, "null graph");
    if (n_keyframes < 0 || n_keyframes > h->D.K || n_mappoints < 0 || n_mappoints > h->D.n)
        return fail(ORBX_ERR_ARG, "more keyframes or MapPoints than the graph was created for");
    if (n_keyframes > 0 && (!kf_mp || !kf_n)) return fail(ORBX_ERR_ARG, "null keyframe table");
    hipStream_t s;
    int rc = covis_enter(h, stream, &s);
    if (rc) return rc;
    CovisDev& D = h->D;
    D.nk = n_keyframes;
    D.nm = n_mappoints;
    D.kf_n = kf_n;
    D.kf_bad = kf_bad;
    D.mp_bad = mp_bad;
    h->refreshed = true;
    h->host_form = false;
    HIP_TRY(hipMemsetAsync(D.obs_cnt, 0, (size_t)D.n * 4, s));
    if (n_keyframes > 0) {
        static thread_local bool attr = false;
        if (!attr) {
            if ((rc = set_lds(k_covis_clean, (size_t)kSortMaxKeys * 8))) return rc;
            attr = true;
        }
        k_covis_clean<<<n_keyframes, kCvThreads, (size_t)kSortMaxKeys * 8, s>>>(D, kf_mp);
        HIP_TRY(hipGetLastError());
    }
    k_covis_scan<<<1, kCvThreads, 0, s>>>(D);
    HIP_TRY(hipGetLastError());
    const long long slots = (long long)n_keyframes * D.cap;
    if (slots > 0) {
        const int grid = (int)((slots + 255) / 256);
        k_covis_fill<<<grid, 256, 0, s>>>(D);
        HIP_TRY(hipGetLastError());
        k_covis_rank<<<grid, 256, 0, s>>>(D);
        HIP_TRY(hipGetLastError());
    }
    return ORBX_OK;
}

int orbx_covis_refresh_observations(orbx_covis* h, int n_keyframes, const int32_t* kf_mp, const int32_t* kf_n,
                                    const uint8_t* kf_bad, int n_mappoints, const uint8_t* mp_bad) {
    if (!h) return fail(ORBX_ERR_ARG, "null graph");
    if (n_keyframes < 0 || n_keyframes > h->D.K || n_mappoints < 0 || n_mappoints > h->D.n)
        return fail(ORBX_ERR_ARG, "more keyframes or MapPoints than the graph was created for");
    if (n_keyframes > 0 && (!kf_mp || !kf_n)) return fail(ORBX_ERR_ARG, "null keyframe table");
    hipStream_t s;
    int rc = covis_enter(h, nullptr, &s);
    if (rc) return rc;
    // the graph keeps kf_n and the bad flags for the later calls: they live in its own copy
    const size_t nk = (size_t)n_keyframes, table = nk * h->D.cap * 4;
    auto round = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t o_n = round(table), o_kb = o_n + round(nk * 4), o_mb = o_kb + round(nk), total = o_mb + round((size_t)n_mappoints);
    HIP_TRY(h->host_map.reserve(total + 256, s));
    char* p = h->host_map.p;
    // pageable sources: staged by the runtime before each call returns
    if (table) HIP_TRY(hipMemcpyAsync(p, kf_mp, table, hipMemcpyHostToDevice, s));
    if (nk) HIP_TRY(hipMemcpyAsync(p + o_n, kf_n, nk * 4, hipMemcpyHostToDevice, s));
    if (nk && kf_bad) HIP_TRY(hipMemcpyAsync(p + o_kb, kf_bad, nk, hipMemcpyHostToDevice, s));
    if (n_mappoints && mp_bad) HIP_TRY(hipMemcpyAsync(p + o_mb, mp_bad, (size_t)n_mappoints, hipMemcpyHostToDevice, s));
    rc = orbx_covis_refresh_observations_device(h, n_keyframes, (const int32_t*)p, (const int32_t*)(p + o_n),
                                                kf_bad ? (const uint8_t*)(p + o_kb) : nullptr, n_mappoints,
                                                mp_bad ? (const uint8_t*)(p + o_mb) : nullptr, nullptr);
    h->host_form = true;
    return rc;
}

int orbx_covis_update_connections_device(orbx_covis* h, const int32_t* ids, int Q, void* stream) {
    if (Q < 0 || (Q > 0 && !ids)) return fail(ORBX_ERR_ARG, "bad argument");
    // the batch's result does not depend on the order of its ids: ascending
    std::vector<int32_t> sorted(ids, ids + Q);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
        return fail(ORBX_ERR_ARG, "a repeated keyframe id");
    if (!h) return fail(ORBX_ERR_ARG, "null graph");
    for (int b = 0; b < Q; b++)
        if (ids[b] < 0 || ids[b] >= h->D.K) return fail(ORBX_ERR_ARG, "keyframe id outside the graph");
    if (!h->refreshed) return fail(ORBX_ERR_STATE, "no observations: call orbx_covis_refresh_observations_device first");
    if (Q == 0) return ORBX_OK;
    hipStream_t s;
    int rc = covis_enter(h, stream, &s);
    if (rc) return rc;
    h->h_ids.swap(sorted);
    // pageable source: staged by the runtime before the call returns
    HIP_TRY(hipMemcpyAsync(h->ids, h->h_ids.data(), (size_t)Q * 4, hipMemcpyHostToDevice, s));
    return launch_update(h, h->ids, Q, nullptr, s);
}

int orbx_covis_erase_keyframe_device(orbx_covis* h, int id, void* stream) {
    if (!h || id < 0 || id >= h->D.K) return fail(ORBX_ERR_ARG, "bad argument");
    if (id == 0) return ORBX_OK;  // cc:497
    hipStream_t s;
    int rc = covis_enter(h, stream, &s);
    if (rc) return rc;
    static thread_local bool attr = false;
    if (!attr) {
        if ((rc = set_lds(k_covis_erase, (size_t)kSortMaxKeys * 8 + (size_t)ORBX_COVIS_LDS_KEYFRAMES * 4))) return rc;
        attr = true;
    }
    k_covis_erase<<<std::min(h->D.max_conn, kCvGroups), kCvThreads, h->lds, s>>>(h->D, id);
    HIP_TRY(hipGetLastError());
    k_covis_clear<<<1, 1, 0, s>>>(h->D, id);
    HIP_TRY(hipGetLastError());
    return ORBX_OK;
}

int orbx_covis_view_device(orbx_covis* h, orbx_covis_view* v) {
    if (!h || !v) return fail(ORBX_ERR_ARG, "null argument");
    const CovisDev& D = h->D;
    *v = orbx_covis_view{D.K,      D.cap,  D.n,     D.max_conn, D.nk,     D.nm,     D.obs_off, D.obs_kf, D.obs_idx, D.clean,
                         D.row_kf, D.row_w, D.row_n, D.ord_kf,   D.ord_w,  D.ord_n,  D.parent,  D.first,  D.status};
    return ORBX_OK;
}

int orbx_covis_best_covisibles_device(orbx_covis* h, int N, int32_t* out, int32_t* out_n, void* stream) {
    if (!h || N < 1 || !out || !out_n) return fail(ORBX_ERR_ARG, "bad argument");
    hipStream_t s;
    int rc = covis_enter(h, stream, &s);
    if (rc) return rc;
    const long long total = (long long)h->D.K * N;
    k_covis_best<<<(int)((total + 255) / 256), 256, 0, s>>>(h->D, N, out, out_n);
    HIP_TRY(hipGetLastError());
    return ORBX_OK;
}

int orbx_covis_covisibles_by_weight_device(orbx_covis* h, int w, int32_t* out, int32_t* out_n, void* stream) {
    if (!h || !out_n) return fail(ORBX_ERR_ARG, "bad argument");
    hipStream_t s;
    int rc = covis_enter(h, stream, &s);
    if (rc) return rc;
    k_covis_by_weight<<<(h->D.K + 255) / 256, 256, 0, s>>>(h->D, w, out, out_n);
    HIP_TRY(hipGetLastError());
    return ORBX_OK;
}

int orbx_covis_read(orbx_covis* h, const void* src, void* dst, size_t bytes) {
    if (!h || (bytes && (!src || !dst))) return fail(ORBX_ERR_ARG, "bad argument");
    hipStream_t s;
    int rc = covis_enter(h, nullptr, &s);
    if (rc) return rc;
    if (bytes) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return ORBX_OK;
}

int orbx_covis_ordered(orbx_covis* h, int id, int32_t* kf, int32_t* w, int cap, int* n) {
    if (!h || id < 0 || id >= h->D.K || cap < 0 || !n || (cap > 0 && !kf)) return fail(ORBX_ERR_ARG, "bad argument");
    hipStream_t s;
    int rc = covis_enter(h, nullptr, &s);
    if (rc) return rc;
    const CovisDev& D = h->D;
    int32_t cnt = 0;
    HIP_TRY(hipMemcpyAsync(&cnt, D.ord_n + id, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *n = cnt;
    const int c = std::min((int)cnt, cap);
    if (c > 0) {
        HIP_TRY(hipMemcpyAsync(kf, D.ord_kf + (size_t)id * D.max_conn, (size_t)c * 4, hipMemcpyDeviceToHost, s));
        if (w) HIP_TRY(hipMemcpyAsync(w, D.ord_w + (size_t)id * D.max_conn, (size_t)c * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return ORBX_OK;
}

int orbx_local_ba_assemble_device(orbx_covis* h, const orbx_local_ba_assembly* a, void* stream) {
    if (!h || !a) return fail(ORBX_ERR_ARG, "null argument");
    if (a->batch < 0 || a->max_kf_rows < 0 || a->max_pt_rows < 0 || a->max_obs < 0) return fail(ORBX_ERR_ARG, "negative size");
    if (!a->kf_off || !a->pt_off || !a->obs_off || !a->counts || !a->status) return fail(ORBX_ERR_ARG, "null table");
    if (a->batch > 0 && (!a->cur_kf || !a->kf_pose || !a->mp_pos)) return fail(ORBX_ERR_ARG, "null map");
    if ((a->max_kf_rows > 0 && (!a->kf_Tcw || !a->kf_fixed || !a->kf_slot || !a->kf_id)) ||
        (a->max_pt_rows > 0 && (!a->pt_pos || !a->pt_id)) || (a->max_obs > 0 && (!a->obs_kf || !a->obs_kp)))
        return fail(ORBX_ERR_ARG, "null table");
    for (int b = 0; b < a->batch; b++)
        if (a->cur_kf[b] < 0 || a->cur_kf[b] >= h->D.K) return fail(ORBX_ERR_ARG, "keyframe id outside the graph");
    if (!h->refreshed) return fail(ORBX_ERR_STATE, "no observations: call orbx_covis_refresh_observations_device first");
    hipStream_t s;
    int rc = covis_enter(h, stream, &s);
    if (rc) return rc;
    const CovisDev& D = h->D;
    AsmWs& W = h->asm_ws;
    if (!W.pmark) {  // the marks start, and are left by every problem, at "none"
        const size_t np = (size_t)kAsmGroups * D.n, nk = (size_t)kAsmGroups * D.K, nl = (size_t)kAsmGroups * (D.max_conn + 1);
        char* p = nullptr;
        HIP_TRY(hipMalloc((void**)&p, (np + nk + nl) * 4));
        h->allocs.push_back(p);
        W.pmark = (int32_t*)p;
        W.kmark = W.pmark + np;
        W.loc = W.kmark + nk;
        std::vector<int32_t> none(np + nk, INT_MAX);
        HIP_TRY(hipMemcpyAsync(p, none.data(), none.size() * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    const size_t B = (size_t)a->batch;
    HIP_TRY(h->asm_batch.reserve((B * 7 + 1) * 4, s));
    int32_t* cur = (int32_t*)h->asm_batch.p;
    W.raw = cur + B;
    W.base = W.raw + 3 * B;
    if (B) {
        // pageable source: staged by the runtime before the call returns
        HIP_TRY(hipMemcpyAsync(cur, a->cur_kf, B * 4, hipMemcpyHostToDevice, s));
        const int grid = (int)std::min<size_t>(B, kAsmGroups);
        k_covis_assemble<<<grid, kCvThreads, 0, s>>>(D, *a, W, cur, 0);
        HIP_TRY(hipGetLastError());
        k_covis_layout<<<1, 1, 0, s>>>(*a, W);
        HIP_TRY(hipGetLastError());
        k_covis_assemble<<<grid, kCvThreads, 0, s>>>(D, *a, W, cur, 1);
        HIP_TRY(hipGetLastError());
    } else {
        k_covis_layout<<<1, 1, 0, s>>>(*a, W);
        HIP_TRY(hipGetLastError());
    }
    return ORBX_OK;
}

int orbx_local_ba_apply_device(orbx_covis* h, const orbx_local_ba_apply* a, void* stream) {
    if (!h || !a) return fail(ORBX_ERR_ARG, "null argument");
    if (a->batch < 0 || a->max_kf_rows < 0 || a->max_pt_rows < 0 || a->cap < 0 || a->n_keyframes < 0 || a->n_mappoints < 0)
        return fail(ORBX_ERR_ARG, "negative size");
    if (!a->kf_off || !a->pt_off || !a->obs_off || !a->kf_pose || !a->mp_pos) return fail(ORBX_ERR_ARG, "null table");
    if ((a->max_kf_rows > 0 && (!a->kf_id || !a->kf_fixed || !a->kf_Tcw_opt)) || (a->max_pt_rows > 0 && (!a->pt_id || !a->pt_pos_opt)) ||
        (a->erase && a->kf_mp && (!a->obs_kf || !a->obs_kp || !a->kf_id)))
        return fail(ORBX_ERR_ARG, "null table");
    hipStream_t s;
    int rc = covis_enter(h, stream, &s);
    if (rc) return rc;
    if (a->max_kf_rows > 0) {
        k_covis_apply_kf<<<(a->max_kf_rows + 255) / 256, 256, 0, s>>>(*a);
        HIP_TRY(hipGetLastError());
    }
    if (a->max_pt_rows > 0) {
        k_covis_apply_pt<<<(a->max_pt_rows + 255) / 256, 256, 0, s>>>(*a);
        HIP_TRY(hipGetLastError());
    }
    return ORBX_OK;
}

}  // extern "C"
