// orbx_covis.h -- what the translation units that work on the covisibility graph share
// (orbx_covis.hip, orbx_localmap.hip): the graph's device arrays, the handle, and the small
// device helpers.  DESIGN.md 4.24, 4.25.
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

}  // namespace orbx
