// orbx_covis.h -- what the translation units that work on the covisibility graph share
// (orbx_covis.hip, orbx_localmap.hip, orbx_culling.hip, orbx_correctloop.hip): the graph's device
// arrays, the handle, the small device helpers and the row helpers.  DESIGN.md 4.24 - 4.27.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "orbx.h"
#include "orbx_block_sort.h"
#include "orbx_host.h"

namespace orbx {

constexpr int kCvThreads = kSortThreads;
constexpr int kCvWaves = kCvThreads / 64;
constexpr int kCvTh = 15;  // KeyFrame.cc:362

struct CovisDev {
    int K, cap, n, max_conn, dense_lds;  // dense_lds: the dense row lives in LDS
    int nk, nm;                          // keyframes / MapPoints of the last refresh
    const int32_t* kf_n;
    const uint8_t* kf_bad;
    const uint8_t* mp_bad;
    int32_t* clean;    // [K][cap] mvpMapPoints without NULL, out-of-range ids and later copies
    int32_t* obs_off;  // [n + 1]
    int32_t* obs_cnt;  // [n] counts, then cursors
    int32_t* obs_kf;   // [K * cap]
    int32_t* obs_idx;  // [K * cap]
    int32_t* tmp_kf;   // [K * cap] observers in arrival order
    int32_t *row_kf, *row_w, *row_n;  // mConnectedKeyFrameWeights, ascending id
    int32_t *ord_kf, *ord_w, *ord_n;  // mvpOrderedConnectedKeyFrames / mvOrderedWeights
    int32_t* parent;                  // mpParent, -1 = NULL
    uint8_t* first;                   // mbFirstConnection
    int32_t* status;
    int32_t* kmax;   // per fresh keyframe: pKFmax when no entry reached th, else -1
    uint8_t* fresh;  // rewritten by the running batch
    int32_t* ws;     // [kCvGroups][K] dense rows when they do not fit LDS
};

// workspace of orbx_local_ba_assemble_device
struct AsmWs {
    int32_t* pmark;  // [kAsmGroups][n]
    int32_t* kmark;  // [kAsmGroups][K]
    int32_t* loc;    // [kAsmGroups][max_conn + 1] lLocalKeyFrames
    int32_t* raw;    // [B][3] what each problem needs
    int32_t* base;   // [B][3] where it goes
};

// workspace of orbx_update_local_map_device: a row per workgroup in flight
struct LocalMapWs {
    int groups = 0;            // rows allocated
    int32_t* pmark = nullptr;  // [groups][n] the first slot that names a MapPoint, INT_MAX = none
    int32_t* hist = nullptr;   // [groups][K] the vote histogram when it does not fit LDS
    int32_t* child_off = nullptr;  // [K + 1] CSR of the spanning tree's children
    int32_t* child_cnt = nullptr;  // [K]
    int32_t* child_tmp = nullptr;  // [K] children in arrival order
    int32_t* child_ids = nullptr;  // [K] children in ascending id
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Words that atomics update in L2 are read and reset past the vector L1, which an atomic leaves stale.
__device__ __forceinline__ int cv_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cv_st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// exclusive prefix of v over the workgroup's threads in thread order; every thread gets the total
static __device__ int cv_block_scan(int v, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int before = 0, tot = 0;
    for (int w = 0; w < kCvWaves; w++) {
        const int c = s_w[w];
        if (w < wave) before += c;
        tot += c;
    }
    __syncthreads();
    total = tot;
    return before + inc - v;
}

struct CvScratch {
    int w[kCvWaves];
    int m, n15;
    unsigned long long best;
};

// Entries, entries >= th and the maximum (the lowest id among equal weights: the strict > in
// ascending id order, cc:370) of a dense row; then, unless it is empty or exceeds max_conn,
// keyframe t's sparse row in ascending id.  Uniform over the workgroup.
static __device__ void cv_dense_to_row(const CovisDev& D, int t, const int* dense, CvScratch& S, int& m, int& n15, int& kfmax) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        S.m = 0;
        S.n15 = 0;
        S.best = 0ull;
    }
    __syncthreads();
    int lm = 0, l15 = 0;
    unsigned long long lb = 0ull;
    for (int k = tid; k < D.K; k += kCvThreads) {
        const int w = cv_ld(dense + k);
        if (w > 0) {
            lm++;
            l15 += w >= kCvTh;
            const unsigned long long key = (unsigned long long)(unsigned)w << 32 | (0xFFFFFFFFu - (unsigned)k);
            lb = key > lb ? key : lb;
        }
    }
    if (lm) {
        atomicAdd(&S.m, lm);
        atomicAdd(&S.n15, l15);
        atomicMax(&S.best, lb);
    }
    __syncthreads();
    m = S.m;
    n15 = S.n15;
    kfmax = m ? (int)(0xFFFFFFFFu - (unsigned)(S.best & 0xFFFFFFFFull)) : -1;
    if (m == 0 || m > D.max_conn) return;
    int base = 0;
    const size_t r0 = (size_t)t * D.max_conn;
    for (int k0 = 0; k0 < D.K; k0 += kCvThreads) {
        const int k = k0 + tid;
        const int w = k < D.K ? cv_ld(dense + k) : 0;
        int tot;
        const int pos = cv_block_scan(w > 0, S.w, tot);
        if (w > 0) {
            D.row_kf[r0 + base + pos] = k;
            D.row_w[r0 + base + pos] = w;
        }
        base += tot;
    }
    if (tid == 0) D.row_n[t] = m;
    __syncthreads();
}

// Keyframe t's ordered list from its row of m entries: sort on (weight, id) and push_front =
// weight descending, id descending among equal weights.  all: every entry (UpdateBestCovisibles);
// else the entries >= th, or kfmax alone when there is none (UpdateConnections).  Returns the
// list's front.  Uniform over the workgroup.
static __device__ int cv_order_row(const CovisDev& D, int t, int m, bool all, int n15, int kfmax, unsigned long long* s_sort) {
    const int tid = threadIdx.x;
    int np = kSortThreads;
    while (np < m) np <<= 1;
    const int ne = np / kSortThreads;
    const size_t r0 = (size_t)t * D.max_conn;
    unsigned long long r[kSortPer];
#pragma unroll
    for (int e = 0; e < kSortPer; e++) {
        r[e] = 0ull;
        const int i = e * kSortThreads + tid;
        if (e < ne && i < m) {
            const int w = D.row_w[r0 + i], id = D.row_kf[r0 + i];
            if (all || w >= kCvTh || (n15 == 0 && id == kfmax)) r[e] = (unsigned long long)(unsigned)w << 32 | (unsigned)id;
        }
    }
    block_bitonic_sort64(r, ne, s_sort);
    const int cnt = all ? m : (n15 > 0 ? n15 : 1);
    for (int j = tid; j < cnt; j += kCvThreads) {
        const unsigned long long key = s_sort[np - 1 - j];
        D.ord_kf[r0 + j] = (int)(unsigned)(key & 0xFFFFFFFFull);
        D.ord_w[r0 + j] = (int)(unsigned)(key >> 32);
    }
    const int front = (int)(unsigned)(s_sort[np - 1] & 0xFFFFFFFFull);
    if (tid == 0) D.ord_n[t] = cnt;
    __syncthreads();
    return front;
}

// weight of keyframe id in keyframe q's row, 0 if absent
__device__ __forceinline__ int cv_row_lookup(const CovisDev& D, int q, int id) {
    const size_t r0 = (size_t)q * D.max_conn;
    int lo = 0, hi = D.row_n[q];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (D.row_kf[r0 + mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return lo < D.row_n[q] && D.row_kf[r0 + lo] == id ? D.row_w[r0 + lo] : 0;
}

}  // namespace orbx

struct orbx_covis {
    orbx::CovisDev D{};
    int device = 0;
    hipStream_t stream = nullptr, last = nullptr;
    std::vector<void*> allocs;
    int32_t* ids = nullptr;  // [K] a batch's ids
    std::vector<int32_t> h_ids;
    size_t lds = 0;
    bool refreshed = false;
    bool host_form = false;       // the last refresh was the host form: the map is the graph's own copy
    int32_t* cull_ws = nullptr;   // [2][K] the children and marks of SetBadFlag, allocated by the first cull
    float* cl_pose_ws = nullptr;  // [max_conn + 1][12] CorrectLoop's corrected poses, allocated by the first propagation
    int32_t* eg_ws = nullptr;     // the essential graph assembly's workspace, allocated by the first assembly
    orbx::AsmWs asm_ws{};  // allocated by the first assembly
    orbx::DeviceBuffer asm_batch;
    orbx::DeviceBuffer host_map;  // the host form's copy of the map
    orbx::LocalMapWs lm_ws;       // allocated by the first UpdateLocalMap, grown with the batch
    orbx::DeviceBuffer lm_ws_buf, lm_batch, lm_host;
};

namespace orbx {

// The graph's calls are ordered on one stream at a time: a call on another stream first waits
// for the last one.
inline int covis_enter(orbx_covis* h, void* stream, hipStream_t* s) {
    HIP_TRY(hipSetDevice(h->device));
    *s = stream ? (hipStream_t)stream : h->stream;
    if (h->last && h->last != *s) HIP_TRY(hipStreamSynchronize(h->last));
    h->last = *s;
    return ORBX_OK;
}

// KeyFrame::UpdateConnections of the keyframes d_ids[0 .. min(*d_n, max_q)): distinct ids inside the
// graph, ids and count on the device (orbx_covis.hip); the caller has entered the graph on s
int covis_update_ids_device(orbx_covis* h, const int32_t* d_ids, const int32_t* d_n, int max_q, hipStream_t s);

}  // namespace orbx
