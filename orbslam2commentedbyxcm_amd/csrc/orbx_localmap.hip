// orbx_localmap.hip -- Tracking::UpdateLocalMap (UpdateLocalKeyFrames + UpdateLocalPoints,
// Tracking.cc:1342-1500) for a batch of frames on the covisibility graph of orbx_covis.hip, and
// TrackLocalMap's tally (cc:1047-1081).  DESIGN.md 4.25.
//
// Everything is integer work; the keyframe id stands in for the reference's KeyFrame* wherever
// the reference iterates a map or set of pointers.  Integer atomics count and mark; every stored
// byte is then put in an order that does not depend on scheduling.  No workgroup waits on another.
//
//   k_lm_children  one workgroup: the CSR of the spanning tree's children from `parent` (count,
//                  scan, arrival order, rank by id), shared by the batch
//   k_lm_frames    one workgroup per frame, counting launch: the votes into a histogram over
//                  keyframe ids (LDS or a global row, the graph's dense-row choice), strategy 1 by
//                  a scan in ascending id, strategy 2 by one wavefront whose lanes test an entry's
//                  10 neighbours, then its children 64 at a time, and pick the first by ballot
//                  ("already local" is an LDS bitmap of K bits); the list goes to local_kf; the
//                  distinct points of the list are counted by atomicMin on per-MapPoint slot
//                  marks, which the frame resets
//   k_lm_layout    one thread lays the frames out against the capacities
//   k_lm_frames    writing launch: nulls the bad MapPoints of frame_mp and repeats the points
//                  only: first appearances in slot order by a scan
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <vector>

#include "orbx.h"
#include "orbx_covis.h"
#include "orbx_host.h"

namespace orbx {
namespace {

constexpr int kLmNone = INT_MAX;
constexpr int kLmMaxList = 80;     // cc:1448
constexpr int kLmNeighbours = 10;  // cc:1454
// Workspace rows (a mark per MapPoint, and the histogram when it is global): one per frame of the
// batch while they fit 256 MiB, and never more than 1024 -- four resident 1024-thread
// workgroups for each of the 256 CUs.  A tracking batch of 256 frames on a map of 200 000
// MapPoints takes 195 MiB and every frame has its own workgroup.
constexpr int kLmMaxGroups = 1024;
constexpr size_t kLmWsBytes = (size_t)256 << 20;
constexpr int kLmRawEmpty = 1, kLmRawOver = 2;

struct LmArgs {
    orbx_local_map_update U;
    const int32_t* parent;
    LocalMapWs W;
    int32_t* raw;  // [B][4] list length, points, kLmRaw* flags, pKFmax
    int hist_lds;
};

struct LmShared {
    int w[kCvWaves];
    int nl, over, np;
    unsigned long long best;
};

__device__ __forceinline__ bool lm_bad(const CovisDev& D, int kf) { return kf < D.nk && D.kf_bad && D.kf_bad[kf]; }

__device__ __forceinline__ bool lm_bit(unsigned* bm, int k) {
    return (__hip_atomic_load(bm + (k >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >> (k & 31)) & 1u;
}
__device__ __forceinline__ void lm_set(unsigned* bm, int k) { atomicOr(bm + (k >> 5), 1u << (k & 31)); }

__global__ void k_lm_fill(int32_t* p, size_t count, int32_t v) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}

// mspChildrens of every keyframe: the keyframes c that are not bad and have parent[c] == k, in
// ascending id (KeyFrame.cc: ChangeParent and EraseChild keep the two in step).
__global__ __launch_bounds__(kCvThreads) void k_lm_children(CovisDev D, LocalMapWs W, const int32_t* parent) {
    __shared__ int s_w[kCvWaves];
    const int tid = threadIdx.x;
    auto parent_of = [&](int c) -> int {
        const int p = parent[c];
        return p >= 0 && p < D.K && !lm_bad(D, c) ? p : -1;
    };
    for (int k = tid; k < D.K; k += kCvThreads) cv_st(W.child_cnt + k, 0);
    __syncthreads();
    for (int c = tid; c < D.K; c += kCvThreads) {
        const int p = parent_of(c);
        if (p >= 0) atomicAdd(&W.child_cnt[p], 1);
    }
    __syncthreads();
    int base = 0;
    for (int k0 = 0; k0 < D.K; k0 += kCvThreads) {
        const int k = k0 + tid;
        const int c = k < D.K ? cv_ld(W.child_cnt + k) : 0;
        int tot;
        const int pos = cv_block_scan(c, s_w, tot);
        if (k < D.K) {
            W.child_off[k] = base + pos;
            cv_st(W.child_cnt + k, 0);
        }
        base += tot;
    }
    if (tid == 0) W.child_off[D.K] = base;
    __syncthreads();
    for (int c = tid; c < D.K; c += kCvThreads) {
        const int p = parent_of(c);
        if (p >= 0) cv_st(W.child_tmp + W.child_off[p] + atomicAdd(&W.child_cnt[p], 1), c);
    }
    __syncthreads();
    for (int c = tid; c < D.K; c += kCvThreads) {
        const int p = parent_of(c);
        if (p < 0) continue;
        const int o0 = W.child_off[p], o1 = W.child_off[p + 1];
        int rank = 0;
        for (int o = o0; o < o1; o++) rank += cv_ld(W.child_tmp + o) < c;
        W.child_ids[o0 + rank] = c;
    }
}

// Strategy 2 (cc:1445-1493) by the workgroup's first wavefront, all 64 lanes: walks the m1
// strategy-1 entries of lkf and appends behind them.  Returns the list's length; over: an entry
// did not fit max_kf.
__device__ int lm_walk(const CovisDev& D, const LmArgs& A, int32_t* lkf, unsigned* bm, int m1, int& over) {
    const int lane = threadIdx.x;
    const int max_kf = A.U.max_local_kf;
    int nl = m1;
    over = 0;
    auto append = [&](int kf) {
        if (lane == 0) {
            if (nl < max_kf) lkf[nl] = kf;
            lm_set(bm, kf);  // mnTrackReferenceForFrame
        }
        over |= nl >= max_kf;
        nl++;
    };
    for (int e0 = 0; e0 < m1; e0 += 64) {
        const int mine = e0 + lane < m1 ? lkf[e0 + lane] : -1;
        const int je = m1 - e0 < 64 ? m1 - e0 : 64;
        for (int j = 0; j < je; j++) {
            if (nl > kLmMaxList) return nl;  // cc:1448
            const int k = __shfl(mine, j, 64);
            int nn = D.ord_n[k];
            nn = nn < kLmNeighbours ? nn : kLmNeighbours;  // GetBestCovisibilityKeyFrames(10)
            const int c0 = A.W.child_off[k], c1 = A.W.child_off[k + 1];
            const int pk = A.parent[k];
            const int nkf = lane < nn ? D.ord_kf[(size_t)k * D.max_conn + lane] : -1;
            unsigned long long m = __ballot(nkf >= 0 && !lm_bad(D, nkf) && !lm_bit(bm, nkf));
            if (m) append(__shfl(nkf, __ffsll((long long)m) - 1, 64));  // cc:1455-1466
            for (int c = c0; c < c1; c += 64) {                          // cc:1469-1480
                const int ch = c + lane < c1 ? A.W.child_ids[c + lane] : -1;
                m = __ballot(ch >= 0 && !lm_bad(D, ch) && !lm_bit(bm, ch));
                if (m) {
                    append(__shfl(ch, __ffsll((long long)m) - 1, 64));
                    break;
                }
            }
            if (pk >= 0 && pk < D.K && !lm_bit(bm, pk)) {  // cc:1483-1491: not tested for badness
                append(pk);
                return nl;  // the reference's break leaves the outer loop
            }
        }
    }
    return nl;
}

// UpdateLocalPoints (cc:1354-1380) over the nl keyframes of lkf.  Counting: returns the number of
// distinct points.  Writing: out[0 .. np_max) receives them in first-appearance order.  The marks
// are left at "none".  Uniform over the workgroup.
__device__ int lm_points(const CovisDev& D, const int32_t* lkf, int nl, int* pmark, bool write, int32_t* out, int np_max,
                         LmShared& S) {
    const int tid = threadIdx.x;
    const long long slots = (long long)nl * D.cap;
    auto point_at = [&](long long s) -> int {
        const int l = (int)(s / D.cap), i = (int)(s - (long long)l * D.cap), kf = lkf[l];
        if (kf < 0 || kf >= D.nk) return -1;
        const int p = D.clean[(size_t)kf * D.cap + i];
        return p < 0 || (D.mp_bad && D.mp_bad[p]) ? -1 : p;
    };
    if (tid == 0) S.np = 0;
    __syncthreads();
    int mine = 0;
    for (long long s = tid; s < slots; s += kCvThreads) {
        const int p = point_at(s);
        if (p >= 0) mine += atomicMin(pmark + p, (int)s) == kLmNone;  // the first to mark a point counts it
    }
    if (mine) atomicAdd(&S.np, mine);
    __syncthreads();
    const int np = S.np;
    if (write) {
        int base = 0;
        for (long long s0 = 0; s0 < slots; s0 += kCvThreads) {
            const long long s = s0 + tid;
            const int p = s < slots ? point_at(s) : -1;
            const bool win = p >= 0 && cv_ld(pmark + p) == (int)s;
            int tot;
            const int j = base + cv_block_scan(win, S.w, tot);
            if (win && j < np_max) out[j] = p;
            base += tot;
        }
        __syncthreads();
    }
    for (long long s = tid; s < slots; s += kCvThreads) {
        const int p = point_at(s);
        if (p >= 0) cv_st(pmark + p, kLmNone);
    }
    __syncthreads();
    return np;
}

__global__ __launch_bounds__(kCvThreads) void k_lm_frames(CovisDev D, LmArgs A, int write) {
    extern __shared__ __attribute__((aligned(16))) int s_lm[];
    __shared__ LmShared S;
    const int tid = threadIdx.x;
    const orbx_local_map_update& U = A.U;
    int* hist = A.hist_lds ? s_lm : A.W.hist + (size_t)blockIdx.x * D.K;
    unsigned* bm = (unsigned*)(s_lm + (A.hist_lds ? D.K : 0));
    int* pmark = A.W.pmark + (size_t)blockIdx.x * D.n;
    const int words = (D.K + 31) >> 5;
    for (int b = blockIdx.x; b < U.batch; b += gridDim.x) {
        int32_t* fmp = U.frame_mp + (size_t)b * U.cap;
        int32_t* lkf = U.local_kf + (size_t)b * U.max_local_kf;
        const int nb = clampi(U.n[b], 0, U.cap);
        if (write) {
            if (U.status[b] & ORBX_LOCAL_MAP_STATUS_CAPACITY) continue;  // uniform
            for (int i = tid; i < nb; i += kCvThreads) {
                const int p = fmp[i];
                if (p >= 0 && p < D.nm && D.mp_bad && D.mp_bad[p]) fmp[i] = -1;  // cc:1405
            }
            lm_points(D, lkf, U.counts[2 * b], pmark, true, U.local_ids + U.local_off[b], U.counts[2 * b + 1], S);
            continue;
        }
        for (int k = tid; k < D.K; k += kCvThreads) cv_st(hist + k, 0);
        for (int k = tid; k < words; k += kCvThreads) bm[k] = 0u;
        if (tid == 0) S.best = 0ull;
        __syncthreads();
        for (int i = tid; i < nb; i += kCvThreads) {  // cc:1393-1408
            const int p = fmp[i];
            if (p < 0 || p >= D.nm || (D.mp_bad && D.mp_bad[p])) continue;
            const int o1 = D.obs_off[p + 1];
            for (int o = D.obs_off[p]; o < o1; o++) atomicAdd(&hist[D.obs_kf[o]], 1);
        }
        __syncthreads();
        int any = 0;
        for (int k = tid; k < D.K; k += kCvThreads) any |= cv_ld(hist + k) > 0;
        any = __syncthreads_or(any);
        int nl, flags = 0, kfmax = -1;
        if (!any) {  // cc:1411: the list of the frame before stays
            flags = kLmRawEmpty;
            nl = clampi(U.local_kf_n[b], 0, U.max_local_kf);
        } else {
            int base = 0;  // cc:1423-1442
            unsigned long long lb = 0ull;
            for (int k0 = 0; k0 < D.K; k0 += kCvThreads) {
                const int k = k0 + tid;
                const int w = k < D.K ? cv_ld(hist + k) : 0;
                const bool good = w > 0 && !lm_bad(D, k);
                int tot;
                const int idx = base + cv_block_scan(good, S.w, tot);
                if (good) {
                    if (idx < U.max_local_kf) lkf[idx] = k;
                    lm_set(bm, k);
                    // the lowest id among the maxima: the strict > in ascending id (cc:1432)
                    const unsigned long long key = (unsigned long long)(unsigned)w << 32 | (0xFFFFFFFFu - (unsigned)k);
                    lb = key > lb ? key : lb;
                }
                base += tot;
            }
            if (lb) atomicMax(&S.best, lb);
            __syncthreads();
            if (S.best) kfmax = (int)(0xFFFFFFFFu - (unsigned)(S.best & 0xFFFFFFFFull));
            if (base > U.max_local_kf) {
                nl = base;
                flags = kLmRawOver;
            } else {
                if (tid < 64) {
                    int over;
                    const int n2 = lm_walk(D, A, lkf, bm, base, over);
                    if (tid == 0) {
                        S.nl = n2;
                        S.over = over;
                    }
                }
                __syncthreads();
                nl = S.nl;
                if (S.over) flags = kLmRawOver;
            }
        }
        const int np = (flags & kLmRawOver) ? 0 : lm_points(D, lkf, nl, pmark, false, nullptr, 0, S);
        if (tid == 0) {
            A.raw[4 * b] = nl;
            A.raw[4 * b + 1] = np;
            A.raw[4 * b + 2] = flags;
            A.raw[4 * b + 3] = kfmax;
        }
        __syncthreads();
    }
}

// One thread lays the frames out in order: one that does not fit gets an empty range and
// CAPACITY, the others go where they would without it.
__global__ void k_lm_layout(LmArgs A) {
    const orbx_local_map_update& U = A.U;
    long long off = 0;
    for (int b = 0; b < U.batch; b++) {
        const int nl = A.raw[4 * b], np = A.raw[4 * b + 1], fl = A.raw[4 * b + 2], kfmax = A.raw[4 * b + 3];
        const bool empty = fl & kLmRawEmpty;
        const bool fits = !(fl & kLmRawOver) && nl <= U.max_local_kf && np <= U.max_local_points && off + np <= U.max_total;
        U.local_off[b] = (int)off;
        U.status[b] = (fits ? 0 : ORBX_LOCAL_MAP_STATUS_CAPACITY) | (empty ? ORBX_LOCAL_MAP_STATUS_EMPTY : 0);
        U.counts[2 * b] = fits ? nl : 0;
        U.counts[2 * b + 1] = fits ? np : 0;
        if (!fits) {
            U.local_kf_n[b] = 0;
        } else if (!empty) {
            U.local_kf_n[b] = nl;
            if (kfmax >= 0) U.ref_kf[b] = kfmax;  // cc:1496-1499
        }
        if (fits) off += np;
    }
    U.local_off[U.batch] = (int)off;
}

constexpr int kTallyThreads = 256;

__global__ __launch_bounds__(kTallyThreads) void k_lm_tally(orbx_track_local_map_tally T) {
    __shared__ int s_n;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) s_n = 0;
    __syncthreads();
    const int nb = clampi(T.n[b], 0, T.cap);
    int32_t* fmp = T.frame_mp + (size_t)b * T.cap;
    int mine = 0;
    for (int i = tid; i < nb; i += kTallyThreads) {
        const int p = fmp[i];
        if (p < 0 || p >= T.n_mappoints) continue;
        if (!T.outlier[(size_t)b * T.cap + i]) {
            if (T.mp_found) atomicAdd(&T.mp_found[p], 1);  // IncreaseFound()
            mine += T.only_tracking || T.observations[p] > 0;
        } else if (T.stereo) {
            fmp[i] = -1;
        }
    }
    if (mine) atomicAdd(&s_n, mine);
    __syncthreads();
    if (tid == 0) {
        const int m = s_n;
        T.matches_inliers[b] = m;
        T.ok[b] = !((T.recently_relocalised && T.recently_relocalised[b] && m < 50) || m < 30);
    }
}

int check_update(const orbx_covis* h, const orbx_local_map_update* u) {
    if (!u) return fail(ORBX_ERR_ARG, "null argument");
    if (u->batch < 0 || u->cap < 0 || u->max_local_kf < 0 || u->max_local_points < 0 || u->max_total < 0)
        return fail(ORBX_ERR_ARG, "negative size");
    if (!u->local_off || (u->batch > 0 && (!u->frame_mp || !u->n || !u->local_kf_n || !u->ref_kf || !u->counts || !u->status)) ||
        (u->batch > 0 && u->max_local_kf > 0 && !u->local_kf) || (u->max_total > 0 && !u->local_ids))
        return fail(ORBX_ERR_ARG, "null table");
    if (!h) return fail(ORBX_ERR_ARG, "null graph");
    if (u->cap != h->D.cap) return fail(ORBX_ERR_ARG, "cap differs from the graph's");
    if (!h->refreshed) return fail(ORBX_ERR_ARG, "no observations: call orbx_covis_refresh_observations_device first");
    return ORBX_OK;
}

}  // namespace
}  // namespace orbx

using namespace orbx;

extern "C" {

int orbx_update_local_map_device(orbx_covis* h, const orbx_local_map_update* u, void* stream) {
    int rc = check_update(h, u);
    if (rc) return rc;
    hipStream_t s;
    if ((rc = covis_enter(h, stream, &s))) return rc;
    const CovisDev& D = h->D;
    LocalMapWs& W = h->lm_ws;
    const size_t K = (size_t)D.K, B = (size_t)u->batch;
    if (!W.child_off) {
        int32_t* p = nullptr;
        HIP_TRY(hipMalloc((void**)&p, (4 * K + 1) * 4));
        h->allocs.push_back(p);
        W.child_off = p;
        W.child_cnt = p + K + 1;
        W.child_tmp = W.child_cnt + K;
        W.child_ids = W.child_tmp + K;
    }
    LmArgs A{};
    A.U = *u;
    A.parent = u->parent ? u->parent : D.parent;
    A.hist_lds = D.dense_lds;
    const size_t row = ((size_t)D.n + (A.hist_lds ? 0 : K)) * 4;
    const int groups = (int)std::max<size_t>(1, std::min<size_t>({B, (size_t)kLmMaxGroups, kLmWsBytes / row}));
    if (groups > W.groups) {  // the marks start, and are left by every frame, at "none"
        HIP_TRY(h->lm_ws_buf.reserve((size_t)groups * row, s));
        W.pmark = (int32_t*)h->lm_ws_buf.p;
        W.hist = W.pmark + (size_t)groups * D.n;
        W.groups = groups;
        k_lm_fill<<<1024, 256, 0, s>>>(W.pmark, (size_t)groups * D.n, kLmNone);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(h->lm_batch.reserve((B * 4 + 1) * 4, s));
    A.raw = (int32_t*)h->lm_batch.p;
    A.W = W;
    if (B) {
        const size_t lds = ((A.hist_lds ? K : 0) + (K + 31) / 32) * 4;
        static thread_local size_t lds_set = 0;
        if (lds > lds_set) {
            HIP_TRY(hipFuncSetAttribute((const void*)k_lm_frames, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            lds_set = lds;
        }
        const int grid = (int)std::min<size_t>(B, (size_t)W.groups);
        k_lm_children<<<1, kCvThreads, 0, s>>>(D, W, A.parent);
        HIP_TRY(hipGetLastError());
        k_lm_frames<<<grid, kCvThreads, lds, s>>>(D, A, 0);
        HIP_TRY(hipGetLastError());
        k_lm_layout<<<1, 1, 0, s>>>(A);
        HIP_TRY(hipGetLastError());
        k_lm_frames<<<grid, kCvThreads, lds, s>>>(D, A, 1);
        HIP_TRY(hipGetLastError());
    } else {
        k_lm_layout<<<1, 1, 0, s>>>(A);
        HIP_TRY(hipGetLastError());
    }
    return ORBX_OK;
}

int orbx_update_local_map(orbx_covis* h, const orbx_local_map_update* u) {
    int rc = check_update(h, u);
    if (rc) return rc;
    hipStream_t s;
    if ((rc = covis_enter(h, nullptr, &s))) return rc;
    const size_t B = (size_t)u->batch, K = (size_t)h->D.K;
    auto round = [](size_t b) { return (b + 255) / 256 * 256; };
    // in/out and out arrays, then the inputs
    struct Part {
        const void* src;
        void* dst;
        size_t bytes, off;
    };
    Part parts[] = {{u->frame_mp, u->frame_mp, B * u->cap * 4, 0},
                    {u->local_kf, u->local_kf, B * u->max_local_kf * 4, 0},
                    {u->local_kf_n, u->local_kf_n, B * 4, 0},
                    {u->ref_kf, u->ref_kf, B * 4, 0},
                    {nullptr, u->local_off, (B + 1) * 4, 0},
                    {nullptr, u->local_ids, (size_t)u->max_total * 4, 0},
                    {nullptr, u->counts, B * 8, 0},
                    {nullptr, u->status, B * 4, 0},
                    {u->n, nullptr, B * 4, 0},
                    {u->parent, nullptr, u->parent ? K * 4 : 0, 0}};
    size_t total = 0;
    for (Part& p : parts) {
        p.off = total;
        total += round(p.bytes);
    }
    HIP_TRY(h->lm_host.reserve(total + 256, s));
    char* d = h->lm_host.p;
    // pageable sources: staged by the runtime before each call returns
    for (const Part& p : parts)
        if (p.src && p.bytes) HIP_TRY(hipMemcpyAsync(d + p.off, p.src, p.bytes, hipMemcpyHostToDevice, s));
    orbx_local_map_update v = *u;
    v.frame_mp = (int32_t*)(d + parts[0].off);
    v.local_kf = (int32_t*)(d + parts[1].off);
    v.local_kf_n = (int32_t*)(d + parts[2].off);
    v.ref_kf = (int32_t*)(d + parts[3].off);
    v.local_off = (int32_t*)(d + parts[4].off);
    v.local_ids = (int32_t*)(d + parts[5].off);
    v.counts = (int32_t*)(d + parts[6].off);
    v.status = (int32_t*)(d + parts[7].off);
    v.n = (const int32_t*)(d + parts[8].off);
    v.parent = u->parent ? (const int32_t*)(d + parts[9].off) : nullptr;
    if ((rc = orbx_update_local_map_device(h, &v, nullptr))) return rc;
    for (const Part& p : parts)
        if (p.dst && p.bytes) HIP_TRY(hipMemcpyAsync(p.dst, d + p.off, p.bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return ORBX_OK;
}

int orbx_track_local_map_tally_device(orbx_covis* h, const orbx_track_local_map_tally* t, void* stream) {
    if (!t) return fail(ORBX_ERR_ARG, "null argument");
    if (t->batch < 0 || t->cap < 0 || t->n_mappoints < 0) return fail(ORBX_ERR_ARG, "negative size");
    if (t->batch > 0 && (!t->frame_mp || !t->n || !t->outlier || !t->matches_inliers || !t->ok ||
                         (t->n_mappoints > 0 && !t->observations)))
        return fail(ORBX_ERR_ARG, "null table");
    if (!h) return fail(ORBX_ERR_ARG, "null graph");
    if (t->batch == 0) return ORBX_OK;
    hipStream_t s;
    int rc = covis_enter(h, stream, &s);
    if (rc) return rc;
    k_lm_tally<<<t->batch, kTallyThreads, 0, s>>>(*t);
    HIP_TRY(hipGetLastError());
    return ORBX_OK;
}

}  // extern "C"
