// orbx_culling.hip -- LocalMapping::KeyFrameCulling (LocalMapping.cc:708-775), the whole of
// KeyFrame::SetBadFlag (KeyFrame.cc:492-598) with MapPoint::EraseObservation / SetBadFlag
// (MapPoint.cc:152-212), LocalMapping::MapPointCulling (LocalMapping.cc:185-220) and
// MapPoint::Observations() on the covisibility graph in HBM.  DESIGN.md 4.26.
//
// Integer work against the literal model (tests/culling_model.py); the keyframe id stands in for
// KeyFrame* wherever the reference's order is a pointer order.  No workgroup waits on another and
// no stored byte depends on scheduling.
//
//   k_cull_eval  one 1024-thread workgroup per candidate of the current keyframe's ordered list,
//                all at once, against the state on entry: {nMPs, nRedundantObservations, verdict}
//   k_cull_walk  one workgroup walks the candidates in list order.  Until the first cull it takes
//                k_cull_eval's counts; from then on it counts each candidate itself, with the same
//                device function, on the live state.  A cull runs SetBadFlag's cascade: the
//                neighbours' rows purged and re-ordered one after the other, the observations'
//                effect on nObs, the MapPoints that fall to nObs <= 2 (bad, their entries -1 in the
//                caller's table and the graph's cleaned copy), the children's new parents, kf_bad.
//                "cull_serial": the walk counts every candidate itself and k_cull_eval is not run.
//   k_set_bad    SetBadFlag of a list of keyframes, one workgroup, in order
//   k_mp_cull    one workgroup over the recent list in passes of 1024: a pass decides every entry
//                on the state the passes before it left, then writes; the kept entries are
//                compacted in order
//   k_obs_count  Observations() of every MapPoint
// The three mutating calls end with the observation refresh's own launches on the mutated table.
//
// Within k_cull_walk / k_set_bad one workgroup writes and later re-reads the graph's rows through
// the shared row helpers' plain accesses: a workgroup runs on one CU and its waves share that
// CU's vector L1, which is write-through, so a barrier orders them.  The words this file writes
// and reads again itself (flags, the cleaned table, parents, marks) go past the L1.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "orbx.h"
#include "orbx_block_sort.h"
#include "orbx_covis.h"
#include "orbx_host.h"

namespace orbx {
namespace {

constexpr int kCullGroups = 128;  // workgroups of k_cull_eval: candidates beyond them are strided
constexpr int kCullThObs = 3;     // LocalMapping.cc:720

struct CullWs {
    int32_t* child;  // [K] mspChildrens in ascending id
    int32_t* mark;   // [K] 0, 1 = a child without a new parent yet, 2 = in sParentCandidates
};

struct CullShared {
    unsigned long long best;
    int new_bad, status;
};

__device__ __forceinline__ int cu_ldb(const uint8_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cu_stb(uint8_t* p, uint8_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Observations() of MapPoint p (MapPoint.cc:134-146: a stereo observation counts 2) over the
// observers that are not bad; cnt: the observers other than k whose octave is <= lvl + 1
// (LocalMapping.cc:737-752, a plain count: the early break does not change the verdict).
template <bool Live>
__device__ __forceinline__ int cu_nobs(const CovisDev& D, const orbx_map_tables& M, int p, int k, int lvl, int& cnt) {
    int nobs = 0;
    cnt = 0;
    const int o1 = D.obs_off[p + 1];
    for (int o = D.obs_off[p]; o < o1; o++) {
        const int kf = D.obs_kf[o];
        if (Live ? cu_ldb(M.kf_bad + kf) : (int)M.kf_bad[kf]) continue;
        const size_t s = (size_t)kf * D.cap + D.obs_idx[o];
        nobs += (M.kf_u_right && M.kf_u_right[s] >= 0.f) ? 2 : 1;
        if (k >= 0 && kf != k && M.kf_keys_un[s].octave <= lvl + 1) cnt++;
    }
    return nobs;
}

// nMPs and nRedundantObservations of candidate k (LocalMapping.cc:722-760) over the cleaned row.
// Uniform over the workgroup.
template <bool Live>
__device__ void cu_eval(const CovisDev& D, const orbx_map_tables& M, int monocular, int k, int* s_w, int& nmps, int& nred) {
    const int nq = clampi(D.kf_n[k], 0, D.cap);
    const size_t r0 = (size_t)k * D.cap;
    int a = 0, b = 0;
    for (int i = threadIdx.x; i < nq; i += kCvThreads) {
        const int p = Live ? cv_ld(D.clean + r0 + i) : D.clean[r0 + i];
        if (p < 0 || (Live ? cu_ldb(M.mp_bad + p) : (int)M.mp_bad[p])) continue;
        if (!monocular) {
            const float d = M.kf_depth[r0 + i];
            if (d > M.kf_th_depth[k] || d < 0.f) continue;
        }
        a++;
        int cnt;
        const int nobs = cu_nobs<Live>(D, M, p, k, M.kf_keys_un[r0 + i].octave, cnt);
        if (nobs > kCullThObs && cnt >= kCullThObs) b++;
    }
    (void)cv_block_scan(a, s_w, nmps);
    (void)cv_block_scan(b, s_w, nred);
}

// LocalMapping.cc:768: a double product against an int
__device__ __forceinline__ bool cu_verdict(int nmps, int nred) { return (double)nred > 0.9 * (double)nmps; }

__device__ __forceinline__ bool cu_skipped(const CovisDev& D, const orbx_map_tables& M, int k, bool live) {
    return k <= 0 || k >= D.nk || (live ? cu_ldb(M.kf_bad + k) : (int)M.kf_bad[k]);  // cc:718; a bad one: outside the reference
}

__global__ __launch_bounds__(kCvThreads) void k_cull_eval(CovisDev D, orbx_map_tables M, int monocular, int cur, int32_t* counts) {
    __shared__ int s_w[kCvWaves];
    const int nc = clampi(D.ord_n[cur], 0, D.max_conn);
    for (int j = blockIdx.x; j < nc; j += gridDim.x) {
        const int k = D.ord_kf[(size_t)cur * D.max_conn + j];
        int nmps = 0, nred = 0;
        const bool skip = cu_skipped(D, M, k, false);  // uniform
        if (!skip) cu_eval<false>(D, M, monocular, k, s_w, nmps, nred);
        if (threadIdx.x == 0) {
            counts[3 * j] = nmps;
            counts[3 * j + 1] = nred;
            counts[3 * j + 2] = !skip && cu_verdict(nmps, nred);
        }
    }
}

__device__ __forceinline__ int* cu_dense(const CovisDev& D, unsigned long long* s_dyn) {
    return D.dense_lds ? (int*)(s_dyn + kSortMaxKeys) : D.ws;  // one workgroup: the first global row
}

// KeyFrame::SetBadFlag of keyframe k.  Returns 0 (id 0, cc:497; outside the graph's keyframes or
// bad already: outside the reference), 2 (mbNotErase: only mbToBeErased is set, cc:500-503) or 1.
// Uniform over the workgroup.
__device__ int cu_set_bad(const CovisDev& D, const orbx_map_tables& M, const CullWs& W, int k, unsigned long long* s_dyn,
                          CvScratch& S, CullShared& C) {
    const int tid = threadIdx.x;
    if (cu_skipped(D, M, k, true)) return 0;
    if (M.kf_not_erase && M.kf_not_erase[k]) {
        if (tid == 0 && M.kf_to_be_erased) cu_stb(M.kf_to_be_erased + k, 1);
        return 2;
    }
    int* dense = cu_dense(D, s_dyn);
    // EraseConnection(this) on the row's keyframes, one after the other (cc:506-508, 607-620)
    const int nrow = D.row_n[k];
    for (int j = 0; j < nrow; j++) {
        const int t = D.row_kf[(size_t)k * D.max_conn + j];
        if (t == k || cv_row_lookup(D, t, k) == 0) continue;  // cc:612: nothing held, nothing re-ordered
        for (int q = tid; q < D.K; q += kCvThreads) dense[q] = 0;
        __syncthreads();
        const size_t r0 = (size_t)t * D.max_conn;
        for (int i = tid; i < D.row_n[t]; i += kCvThreads)
            if (D.row_kf[r0 + i] != k) dense[D.row_kf[r0 + i]] = D.row_w[r0 + i];
        __syncthreads();
        int m, n15, kfmax;
        cv_dense_to_row(D, t, dense, S, m, n15, kfmax);
        if (m == 0) {
            if (tid == 0) {
                D.row_n[t] = 0;
                D.ord_n[t] = 0;
            }
            __syncthreads();
            continue;
        }
        cv_order_row(D, t, m, true, 0, -1, s_dyn);
    }
    if (tid == 0) {
        D.row_n[k] = 0;  // cc:519-520
        D.ord_n[k] = 0;
        cu_stb(M.kf_bad + k, 1);  // cc:592; set here: from now on k is no observer and no child
    }
    __syncthreads();
    // EraseObservation(this) on every entry (cc:510-512, MapPoint.cc:152-180); the row keeps its entries
    const int nq = clampi(D.kf_n[k], 0, D.cap);
    int nb = 0;
    for (int i = tid; i < nq; i += kCvThreads) {
        const int p = cv_ld(D.clean + (size_t)k * D.cap + i);
        if (p < 0 || cu_ldb(M.mp_bad + p)) continue;  // a bad MapPoint holds no observation
        int cnt;
        if (cu_nobs<true>(D, M, p, -1, 0, cnt) > 2) continue;
        cu_stb(M.mp_bad + p, 1);  // MapPoint::SetBadFlag, cc:195-212
        nb++;
        for (int o = D.obs_off[p]; o < D.obs_off[p + 1]; o++) {
            const int kf = D.obs_kf[o];
            if (cu_ldb(M.kf_bad + kf)) continue;
            const size_t s = (size_t)kf * D.cap + D.obs_idx[o];
            cv_st(D.clean + s, -1);  // EraseMapPointMatch
            cv_st(M.kf_mp + s, -1);
        }
    }
    if (nb) atomicAdd(&C.new_bad, nb);
    // the children's new parents (cc:522-584)
    const int P = cv_ld(D.parent + k);
    int nch = 0;
    for (int c0 = 0; c0 < D.nk; c0 += kCvThreads) {
        const int c = c0 + tid;
        const bool is = c < D.nk && c != k && c != P && !cu_ldb(M.kf_bad + c) && cv_ld(D.parent + c) == k;
        int tot;
        const int pos = cv_block_scan(is, S.w, tot);
        if (is) {
            cv_st(W.child + nch + pos, c);
            cv_st(W.mark + c, 1);
        }
        nch += tot;
    }
    if (tid == 0) {
        if (P >= 0) cv_st(W.mark + P, 2);
        else C.status |= ORBX_CULL_STATUS_NO_PARENT;  // the reference dereferences NULL here
    }
    __syncthreads();
    for (int round = 0; round < nch; round++) {
        if (tid == 0) C.best = 0ull;
        __syncthreads();
        // the largest weight over (child ascending) x (position in its ordered list) whose keyframe
        // is a candidate; strict >: the first in that order wins a tie
        for (int j = 0; j < nch; j++) {
            const int c = cv_ld(W.child + j);
            if (cv_ld(W.mark + c) != 1) continue;  // uniform
            const int n = clampi(D.ord_n[c], 0, D.max_conn);
            for (int pos = tid; pos < n; pos += kCvThreads) {
                const int kf = D.ord_kf[(size_t)c * D.max_conn + pos];
                if (cv_ld(W.mark + kf) != 2) continue;
                const unsigned rank = (unsigned)j * (unsigned)D.max_conn + (unsigned)pos;
                atomicMax(&C.best, (unsigned long long)(unsigned)cv_row_lookup(D, c, kf) << 32 | (0xFFFFFFFFu - rank));
            }
        }
        __syncthreads();
        const unsigned long long best = C.best;
        __syncthreads();
        if (best == 0ull) break;
        if (tid == 0) {
            const unsigned rank = 0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull);
            const int c = cv_ld(W.child + (int)(rank / (unsigned)D.max_conn));
            cv_st(D.parent + c, D.ord_kf[(size_t)c * D.max_conn + rank % (unsigned)D.max_conn]);  // ChangeParent
            cv_st(W.mark + c, 2);
        }
        __syncthreads();
    }
    for (int j = tid; j < nch; j += kCvThreads) {
        const int c = cv_ld(W.child + j);
        if (cv_ld(W.mark + c) == 1) cv_st(D.parent + c, P);  // cc:578-584
        cv_st(W.mark + c, 0);
    }
    __syncthreads();
    if (tid == 0 && P >= 0) cv_st(W.mark + P, 0);
    __syncthreads();
    return 1;
}

__global__ __launch_bounds__(kCvThreads) void k_cull_walk(CovisDev D, orbx_map_tables M, CullWs W, int monocular, int cur,
                                                          int serial, int32_t* cand, int32_t* counts, int32_t* n_cand,
                                                          int32_t* culled, int32_t* n_culled, int32_t* n_new_bad, int32_t* status) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_dyn[];
    __shared__ CvScratch S;
    __shared__ CullShared C;
    const int tid = threadIdx.x;
    if (tid == 0) C.new_bad = C.status = 0;
    // the candidates are taken once (cc:714): the culls re-order the current keyframe's list
    const int nc = clampi(D.ord_n[cur], 0, D.max_conn);
    for (int j = tid; j < nc; j += kCvThreads) cv_st(cand + j, D.ord_kf[(size_t)cur * D.max_conn + j]);
    __syncthreads();
    bool live = serial != 0;
    int ncul = 0;
    for (int j = 0; j < nc; j++) {
        const int k = cv_ld(cand + j);
        int nmps = 0, nred = 0, res = 0;
        if (!cu_skipped(D, M, k, true)) {  // uniform
            if (live) {
                cu_eval<true>(D, M, monocular, k, S.w, nmps, nred);
            } else {
                nmps = counts[3 * j];
                nred = counts[3 * j + 1];
            }
            if (cu_verdict(nmps, nred)) res = cu_set_bad(D, M, W, k, s_dyn, S, C);
            if (res == 1) {
                live = true;
                if (tid == 0) culled[ncul] = k;
                ncul++;
            }
        }
        if (tid == 0) {
            counts[3 * j] = nmps;
            counts[3 * j + 1] = nred;
            counts[3 * j + 2] = res;
        }
    }
    __syncthreads();
    if (tid == 0) {
        *n_cand = nc;
        *n_culled = ncul;
        *n_new_bad = C.new_bad;
        *status = C.status;
    }
}

__global__ __launch_bounds__(kCvThreads) void k_set_bad(CovisDev D, orbx_map_tables M, CullWs W, const int32_t* ids, int Q,
                                                        int32_t* n_new_bad, int32_t* status) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_dyn[];
    __shared__ CvScratch S;
    __shared__ CullShared C;
    if (threadIdx.x == 0) C.new_bad = C.status = 0;
    __syncthreads();
    for (int b = 0; b < Q; b++) (void)cu_set_bad(D, M, W, ids[b], s_dyn, S, C);
    __syncthreads();
    if (threadIdx.x == 0) {
        *n_new_bad = C.new_bad;
        *status = C.status;
    }
}

__global__ __launch_bounds__(kCvThreads) void k_mp_cull(CovisDev D, orbx_map_tables M, int cur_id, int th_obs, int32_t* recent,
                                                        int32_t* n_recent, int max_recent, const int32_t* first_kf,
                                                        const int32_t* found, const int32_t* visible, int32_t* n_culled) {
    __shared__ int s_w[kCvWaves];
    const int tid = threadIdx.x;
    const int n = clampi(*n_recent, 0, max_recent);
    int base = 0, ncul = 0;
    for (int j0 = 0; j0 < n; j0 += kCvThreads) {
        const int j = j0 + tid;
        const int p = j < n ? recent[j] : -1;
        int act = 0;  // 0: dropped, 1: kept, 2: SetBadFlag and dropped
        if (p >= 0 && p < D.nm && !cu_ldb(M.mp_bad + p)) {  // cc:196-199
            const float ratio = (float)found[p] / (float)visible[p];  // MapPoint::GetFoundRatio: 0 / 0 does not compare less
            const int age = cur_id - first_kf[p];
            int cnt;
            if (ratio < 0.25f) act = 2;  // cc:200-204
            else if (age >= 2 && cu_nobs<false>(D, M, p, -1, 0, cnt) <= th_obs) act = 2;  // cc:205-209
            else act = age >= 3 ? 0 : 1;  // cc:210-213
        }
        int tk, tc;
        const int pos = cv_block_scan(act == 1, s_w, tk);  // its barrier: the pass has decided before it writes
        (void)cv_block_scan(act == 2, s_w, tc);
        if (act == 2) {
            cu_stb(M.mp_bad + p, 1);
            for (int o = D.obs_off[p]; o < D.obs_off[p + 1]; o++) {
                const int kf = D.obs_kf[o];
                if (M.kf_bad[kf]) continue;
                const size_t s = (size_t)kf * D.cap + D.obs_idx[o];
                D.clean[s] = -1;
                M.kf_mp[s] = -1;
            }
        }
        if (act == 1) recent[base + pos] = p;
        base += tk;
        ncul += tc;
        __syncthreads();
    }
    if (tid == 0) {
        *n_recent = base;
        *n_culled = ncul;
    }
}

__global__ void k_obs_count(CovisDev D, const float* u_right, int32_t* out) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= D.nm) return;
    int nobs = 0;
    if (!(D.mp_bad && D.mp_bad[p]))
        for (int o = D.obs_off[p]; o < D.obs_off[p + 1]; o++) {
            const int kf = D.obs_kf[o];
            if (D.kf_bad && D.kf_bad[kf]) continue;
            nobs += (u_right && u_right[(size_t)kf * D.cap + D.obs_idx[o]] >= 0.f) ? 2 : 1;
        }
    out[p] = nobs;
}

}  // namespace
}  // namespace orbx

namespace {

using namespace orbx;

// what every mutating call requires of the graph and the tables, before any device call
int check_tables(orbx_covis* h, const orbx_map_tables* m) {
    if (!h) return fail(ORBX_ERR_ARG, "null graph");
    if (!m) return fail(ORBX_ERR_ARG, "null map tables");
    if (!m->kf_mp || !m->kf_bad || !m->mp_bad) return fail(ORBX_ERR_ARG, "null kf_mp, kf_bad or mp_bad");
    if (!h->refreshed) return fail(ORBX_ERR_ARG, "no observations: call orbx_covis_refresh_observations_device first");
    if (h->host_form) return fail(ORBX_ERR_ARG, "the graph was refreshed through the host form and owns a copy of the map");
    if (m->kf_bad != h->D.kf_bad || m->mp_bad != h->D.mp_bad)
        return fail(ORBX_ERR_ARG, "kf_bad / mp_bad are not the arrays of the last refresh");
    return ORBX_OK;
}

int cull_ws(orbx_covis* h, hipStream_t s, CullWs* W) {
    if (!h->cull_ws) {
        const size_t K = (size_t)h->D.K;
        HIP_TRY(hipMalloc((void**)&h->cull_ws, 2 * K * 4));
        h->allocs.push_back(h->cull_ws);
        HIP_TRY(hipMemsetAsync(h->cull_ws, 0, 2 * K * 4, s));  // the marks start, and are left by every call, at 0
    }
    W->child = h->cull_ws;
    W->mark = h->cull_ws + h->D.K;
    return ORBX_OK;
}

template <class K>
int cull_lds(K kern) {
    HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)((size_t)kSortMaxKeys * 8 + (size_t)ORBX_COVIS_LDS_KEYFRAMES * 4)));
    return ORBX_OK;
}

int refresh_after(orbx_covis* h, const orbx_map_tables* m, void* stream) {
    const CovisDev& D = h->D;
    return orbx_covis_refresh_observations_device(h, D.nk, m->kf_mp, D.kf_n, D.kf_bad, D.nm, D.mp_bad, stream);
}

}  // namespace

extern "C" {

int orbx_keyframe_culling_device(orbx_covis* h, const orbx_map_tables* m, int cur_kf, int monocular, int32_t* cand,
                                 int32_t* cand_counts, int32_t* n_cand, int32_t* culled, int32_t* n_culled,
                                 int32_t* n_new_bad_mp, int32_t* status, void* stream) {
    int rc = check_tables(h, m);
    if (rc) return rc;
    if (!m->kf_keys_un) return fail(ORBX_ERR_ARG, "null kf_keys_un");
    if (!monocular && (!m->kf_depth || !m->kf_th_depth)) return fail(ORBX_ERR_ARG, "kf_depth and kf_th_depth are required unless monocular");
    if (!cand || !cand_counts || !n_cand || !culled || !n_culled || !n_new_bad_mp || !status) return fail(ORBX_ERR_ARG, "null result array");
    if (cur_kf < 0 || cur_kf >= h->D.K) return fail(ORBX_ERR_ARG, "keyframe id outside the graph");
    hipStream_t s;
    if ((rc = covis_enter(h, stream, &s))) return rc;
    CullWs W;
    if ((rc = cull_ws(h, s, &W))) return rc;
    static thread_local bool attr = false;
    if (!attr) {
        if ((rc = cull_lds(k_cull_walk))) return rc;
        attr = true;
    }
    const CovisDev& D = h->D;
    const int serial = tuning(Tune::CullSerial, 0) > 0;
    if (!serial) {
        k_cull_eval<<<std::min(D.max_conn, kCullGroups), kCvThreads, 0, s>>>(D, *m, monocular != 0, cur_kf, cand_counts);
        HIP_TRY(hipGetLastError());
    }
    k_cull_walk<<<1, kCvThreads, h->lds, s>>>(D, *m, W, monocular != 0, cur_kf, serial, cand, cand_counts, n_cand, culled, n_culled,
                                             n_new_bad_mp, status);
    HIP_TRY(hipGetLastError());
    return refresh_after(h, m, stream);
}

int orbx_covis_set_bad_flag_device(orbx_covis* h, const orbx_map_tables* m, const int32_t* ids, int Q, int32_t* n_new_bad_mp,
                                   int32_t* status, void* stream) {
    int rc = check_tables(h, m);
    if (rc) return rc;
    if (Q < 0 || (Q > 0 && !ids) || !n_new_bad_mp || !status) return fail(ORBX_ERR_ARG, "bad argument");
    std::vector<int32_t> sorted(ids, ids + Q);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(ORBX_ERR_ARG, "a repeated keyframe id");
    if (Q > 0 && (sorted.front() < 0 || sorted.back() >= h->D.K)) return fail(ORBX_ERR_ARG, "keyframe id outside the graph");
    hipStream_t s;
    if ((rc = covis_enter(h, stream, &s))) return rc;
    CullWs W;
    if ((rc = cull_ws(h, s, &W))) return rc;
    static thread_local bool attr = false;
    if (!attr) {
        if ((rc = cull_lds(k_set_bad))) return rc;
        attr = true;
    }
    h->h_ids.assign(ids, ids + Q);  // in the caller's order
    // pageable source: staged by the runtime before the call returns
    if (Q) HIP_TRY(hipMemcpyAsync(h->ids, h->h_ids.data(), (size_t)Q * 4, hipMemcpyHostToDevice, s));
    k_set_bad<<<1, kCvThreads, h->lds, s>>>(h->D, *m, W, h->ids, Q, n_new_bad_mp, status);
    HIP_TRY(hipGetLastError());
    return refresh_after(h, m, stream);
}

int orbx_map_point_culling_device(orbx_covis* h, const orbx_map_tables* m, int cur_kf_id, int monocular, int32_t* recent,
                                  int32_t* n_recent, int max_recent, const int32_t* mp_first_kf, const int32_t* mp_found,
                                  const int32_t* mp_visible, int32_t* n_culled, void* stream) {
    if (max_recent < 0) return fail(ORBX_ERR_ARG, "negative max_recent");
    int rc = check_tables(h, m);
    if (rc) return rc;
    if (!n_recent || (max_recent > 0 && !recent) || !mp_first_kf || !mp_found || !mp_visible || !n_culled)
        return fail(ORBX_ERR_ARG, "null argument");
    hipStream_t s;
    if ((rc = covis_enter(h, stream, &s))) return rc;
    k_mp_cull<<<1, kCvThreads, 0, s>>>(h->D, *m, cur_kf_id, monocular ? 2 : 3, recent, n_recent, max_recent, mp_first_kf, mp_found,
                                       mp_visible, n_culled);
    HIP_TRY(hipGetLastError());
    return refresh_after(h, m, stream);
}

int orbx_covis_observation_counts_device(orbx_covis* h, const float* kf_u_right, int32_t* out, void* stream) {
    if (!h) return fail(ORBX_ERR_ARG, "null graph");
    if (!out) return fail(ORBX_ERR_ARG, "null result array");
    if (!h->refreshed) return fail(ORBX_ERR_ARG, "no observations: call orbx_covis_refresh_observations_device first");
    hipStream_t s;
    int rc = covis_enter(h, stream, &s);
    if (rc) return rc;
    if (h->D.nm > 0) {
        k_obs_count<<<(h->D.nm + 255) / 256, 256, 0, s>>>(h->D, kf_u_right, out);
        HIP_TRY(hipGetLastError());
    }
    return ORBX_OK;
}

}  // extern "C"
