// orbx_pnp.hip -- device PnPsolver: EPnP under RANSAC for a batch of relocalisation candidates
// in HBM.
//
// Reference: include/PnPsolver.h, src/PnPsolver.cc:80-1345 (constructor 80-128,
// SetRansacParameters 141-190, find 193-197, iterate 200-323, Refine 326-378, CheckInliers
// 381-418, EPnP 426-1345), as driven by Tracking::Relocalization (Tracking.cc:1511-1684).
// DESIGN.md §4.21.  The algebra and its conventions are in orbx_epnp.h.
//
// Four kernels per solver:
//   k_pnp_set    one workgroup per candidate: the constructor.  Slots with a valid MapPoint id
//                are compacted in slot order (ballot + wave counts: the order is
//                mvKeyPointIndices); mvP2D, mvP3Dw and mvMaxError go to the workspace as
//                structure-of-arrays floats; the adjusted mRansacMinInliers and mRansacMaxIts
//                are looked up in the host's tables at N.
//   k_pnp_hyp    one lane per (candidate, iteration of this call's window): compute_pose on the
//                four drawn correspondences.  Every matrix with a runtime index lives in LDS,
//                lane-minor, so no two lanes share a bank and nothing goes to scratch.
//   k_pnp_count  one wave per (candidate, iteration): CheckInliers over the N correspondences,
//                counted by ballot + popcount.  One count per (candidate, iteration).
//   k_pnp_walk   one workgroup per candidate: one thread walks the window's counts with the
//                rules of cc:226-322.  When the best state changes the workgroup recomputes
//                its flags, one thread gathers the inliers in index order and runs
//                compute_pose on them (Refine, cc:326-378), the workgroup counts the refined
//                pose's inliers.  Refine is a pure function of mvbBestInliers: its result is
//                kept with the best state and reused by every later qualifying iteration.
//
// Float inputs are widened to double; everything after is double under -ffp-contract=off except
// CheckInliers' mixed precision; poses are rounded to float once per result.  There is no
// floating-point sum across lanes at all: every sum of Refine runs in index order in one
// thread (a deviation from a tree-shaped M^T M: simpler, and the same bytes by construction).
// A candidate's bytes depend neither on the batch around it nor on how its iterations are cut
// into calls.  The host reads nothing back between a set and the end of an iterate.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "orbx.h"
#include "orbx_epnp.h"
#include "orbx_host.h"

namespace orbx {

constexpr int kPnpThreads = 256;
constexpr int kPnpWaves = kPnpThreads / 64;
constexpr int kPnpHypLanes = 32;
constexpr int kPnpHypWork = epnp::kWork + 48;  // + pws 12, us 8, alphas 16, pcs 12
constexpr int kPnpState = 12;                  // ints per candidate
enum {
    kPsN = 0, kPsMinInliers, kPsMaxIts, kPsIterations, kPsBestInliers, kPsBestIteration, kPsStatus, kPsSlots,
    kPsRefValid, kPsRefInliers
};

struct PnpWork {
    float* pts;       // [B][6][cap]  mvP2D xy, mvP3Dw xyz, mvMaxError
    int32_t* idx;     // [B][cap]     mvKeyPointIndices
    int32_t* mpid;    // [B][cap]     the MapPoint id of each correspondence
    int32_t* state;   // [B][12]
    int32_t* counts;  // [B][max_draws] of the running call; -1: a draw out of range
    double* hyp;      // [B][max_draws][12] of the running call: R row-major, t
    double* pose;     // [B][2][12]   the best state's pose, the refined pose
    float* best_T;    // [B][12]      mBestTcw
    double* ref;      // [B][12][cap] Refine's pws, us, alphas, pcs
    uint8_t* flags;   // [B][cap]     mvbBestInliers when Refine gathers
    int cap, max_draws;
};

struct PnpSetArgs {
    const orbx_keypoint* kps;  // [B][cap]
    const int32_t* n;          // [B]
    const int32_t* matches;    // [B][cap]
    const float* pos;          // [n_mp][3]
    int n_mp, cap, nlevels;
    float sigma2[ORBX_MAX_LEVELS];
    float th2;
    const int32_t* min_inl;    // [cap + 1] mRansacMinInliers by N
    const int32_t* its;        // [cap + 1] mRansacMaxIts by N
    PnpWork W;
};

struct PnpRunArgs {
    PnpWork W;
    const int32_t* draws;  // [B][n_draws][4]
    int n_draws, n_iterations, out_cap;
    epnp::Camera K;
    orbx_pnp_result out;
};

// The iterations of this call that the reference would walk unless it returns (cc:226: an OR),
// and those of them that have draws.
__device__ __forceinline__ void pnp_window(const int32_t* st, int n_iterations, int n_draws, int* window, int* avail) {
    const int N = st[kPsN], it0 = st[kPsIterations];
    int w = st[kPsMaxIts] - it0;
    w = w > n_iterations ? w : n_iterations;
    if (N < st[kPsMinInliers]) w = 0;  // cc:210
    int a = n_draws - it0;
    a = a < 0 ? 0 : (a > w ? w : a);
    *window = w;
    *avail = a;
}

__global__ __launch_bounds__(kPnpThreads) void k_pnp_set(PnpSetArgs A) {
    __shared__ int s_cnt[kPnpWaves];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cap = A.cap, wcap = A.W.cap;
    int n = A.n[b];
    n = n < 0 ? 0 : (n > cap ? cap : n);
    const size_t row = (size_t)b * cap;
    float* pts = A.W.pts + (size_t)b * 6 * wcap;
    int32_t* idx = A.W.idx + (size_t)b * wcap;
    int32_t* mpid = A.W.mpid + (size_t)b * wcap;
    int total = 0;
    for (int base = 0; base < n; base += kPnpThreads) {
        const int i = base + tid;
        int a = -1;
        if (i < n) a = A.matches[row + i];
        const bool keep = a >= 0 && a < A.n_mp;  // cc:96-118 through the caller's ids
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_cnt[wave] = __popcll(m);
        __syncthreads();
        int off = total;
        for (int w = 0; w < wave; w++) off += s_cnt[w];
        int all = 0;
        for (int w = 0; w < kPnpWaves; w++) all += s_cnt[w];
        if (keep) {
            const int e = off + __popcll(m & ((1ull << lane) - 1ull));  // e <= i < cap
            const orbx_keypoint kp = A.kps[row + i];
            int o = kp.octave;
            o = o < 0 ? 0 : (o >= A.nlevels ? A.nlevels - 1 : o);
            const float* p = A.pos + (size_t)a * 3;
            pts[e] = kp.x;
            pts[(size_t)wcap + e] = kp.y;
            pts[(size_t)2 * wcap + e] = p[0];
            pts[(size_t)3 * wcap + e] = p[1];
            pts[(size_t)4 * wcap + e] = p[2];
            pts[(size_t)5 * wcap + e] = A.sigma2[o] * A.th2;  // cc:189: a float product
            idx[e] = i;
            mpid[e] = a;
        }
        total += all;
        __syncthreads();
    }
    if (tid == 0) {
        int32_t* st = A.W.state + (size_t)b * kPnpState;
        st[kPsN] = total;
        st[kPsMinInliers] = A.min_inl[total];  // total <= n <= cap
        st[kPsMaxIts] = A.its[total];
        st[kPsIterations] = 0;
        st[kPsBestInliers] = 0;
        st[kPsBestIteration] = -1;
        st[kPsStatus] = 0;
        st[kPsSlots] = n;
        st[kPsRefValid] = 0;
        st[kPsRefInliers] = 0;
        st[10] = st[11] = 0;
        float* bt = A.W.best_T + (size_t)b * 12;
        for (int i = 0; i < 12; i++) bt[i] = __builtin_nanf("");
    }
}

__global__ __launch_bounds__(kPnpHypLanes) void k_pnp_hyp(PnpRunArgs A) {
    __shared__ double s[kPnpHypWork * kPnpHypLanes];
    const int b = blockIdx.y, lane = threadIdx.x;
    const int j = blockIdx.x * kPnpHypLanes + lane;
    const int32_t* st = A.W.state + (size_t)b * kPnpState;
    int window, avail;
    pnp_window(st, A.n_iterations, A.n_draws, &window, &avail);
    if (j >= avail) return;
    const int N = st[kPsN], k = st[kPsIterations] + j;  // k < n_draws
    const int32_t* d = A.draws + ((size_t)b * A.n_draws + k) * 4;
    // the swap-with-last selection of cc:237-250 on an implicit identity array
    int id[4], pos[4], val[4];
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int r = d[q], last = N - 1 - q;
        ok = ok && r >= 0 && r <= last;
        int v = r, lv = last;
#pragma unroll
        for (int t = 0; t < q; t++) {
            if (pos[t] == r) v = val[t];
            if (pos[t] == last) lv = val[t];
        }
        id[q] = v;
        pos[q] = r;
        val[q] = lv;
    }
    double* H = A.W.hyp + ((size_t)b * A.W.max_draws + j) * 12;
    if (!ok) {  // N >= 4 here: the adjusted minimum is at least 4
        for (int i = 0; i < 12; i++) H[i] = __builtin_nan("");
        A.W.counts[(size_t)b * A.W.max_draws + j] = -1;
        return;
    }
    const epnp::Mem W{s + lane, kPnpHypLanes};
    const epnp::Mem pws = W.at(epnp::kWork), us = W.at(epnp::kWork + 12), alphas = W.at(epnp::kWork + 20),
                    pcs = W.at(epnp::kWork + 36);
    const float* pts = A.W.pts + (size_t)b * 6 * A.W.cap;
    const size_t c = (size_t)A.W.cap;
#pragma unroll
    for (int q = 0; q < 4; q++) {  // add_correspondence (cc:245)
        const int e = id[q];       // in [0, N)
        us(2 * q) = (double)pts[e];
        us(2 * q + 1) = (double)pts[c + e];
        pws(3 * q) = (double)pts[2 * c + e];
        pws(3 * q + 1) = (double)pts[3 * c + e];
        pws(3 * q + 2) = (double)pts[4 * c + e];
    }
    double R[9], t[3];
    epnp::compute_pose(4, pws, us, alphas, pcs, W, A.K, R, t);
#pragma unroll
    for (int i = 0; i < 9; i++) H[i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) H[9 + i] = t[i];
    A.W.counts[(size_t)b * A.W.max_draws + j] = 0;
}

__device__ __forceinline__ bool pnp_inlier(const epnp::Camera& K, const float* pts, size_t c, int i, const double* P) {
    return epnp::check_inlier(P, P + 9, K, pts[2 * c + i], pts[3 * c + i], pts[4 * c + i], pts[i], pts[c + i],
                              pts[5 * c + i]);
}

__global__ __launch_bounds__(kPnpThreads) void k_pnp_count(PnpRunArgs A) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int j = blockIdx.x * kPnpWaves + (threadIdx.x >> 6);
    const int32_t* st = A.W.state + (size_t)b * kPnpState;
    int window, avail;
    pnp_window(st, A.n_iterations, A.n_draws, &window, &avail);
    if (j >= avail) return;
    int32_t* cnt = A.W.counts + (size_t)b * A.W.max_draws + j;
    if (*cnt < 0) return;  // a bad draw
    const int N = st[kPsN];
    double P[12];
    const double* H = A.W.hyp + ((size_t)b * A.W.max_draws + j) * 12;
#pragma unroll
    for (int i = 0; i < 12; i++) P[i] = H[i];
    const float* pts = A.W.pts + (size_t)b * 6 * A.W.cap;
    int count = 0;
    for (int base = 0; base < N; base += 64) {
        const int i = base + lane;
        const bool in = i < N && pnp_inlier(A.K, pts, (size_t)A.W.cap, i, P);
        count += __popcll(__ballot(in));
    }
    if (lane == 0) *cnt = count;
}

__global__ __launch_bounds__(kPnpThreads) void k_pnp_walk(PnpRunArgs A) {
    __shared__ double s_W[epnp::kWork];
    __shared__ double s_P[12];
    __shared__ int s_ev[4];  // event (0 done, 1 refine), next j, a counter, the gathered count
    __shared__ int s_res[8];  // found, refined, n_inliers, iterations, best, best iteration, status, no_more
    const int b = blockIdx.x, tid = threadIdx.x;
    int32_t* st = A.W.state + (size_t)b * kPnpState;
    const int N = st[kPsN], min_inl = st[kPsMinInliers], max_its = st[kPsMaxIts], it0 = st[kPsIterations],
              slots = st[kPsSlots];
    int window, avail;
    pnp_window(st, A.n_iterations, A.n_draws, &window, &avail);
    const float* pts = A.W.pts + (size_t)b * 6 * A.W.cap;
    const size_t c = (size_t)A.W.cap;
    double* best_pose = A.W.pose + (size_t)b * 24;
    double* ref_pose = best_pose + 12;
    float* best_T = A.W.best_T + (size_t)b * 12;
    double* ref = A.W.ref + (size_t)b * 12 * c;
    uint8_t* flags = A.W.flags + (size_t)b * c;
    if (tid == 0) {
        s_ev[0] = 1;
        s_ev[1] = 0;
        s_res[0] = 0;
        s_res[1] = 0;
        s_res[2] = 0;
        s_res[3] = it0;
        s_res[4] = st[kPsBestInliers];
        s_res[5] = st[kPsBestIteration];
        s_res[6] = st[kPsStatus];
        s_res[7] = 0;
    }
    __syncthreads();
    for (;;) {
        if (tid == 0) {
            int ev = 0, j = s_ev[1], it = s_res[3], best = s_res[4], best_it = s_res[5], status = s_res[6];
            int ref_valid = st[kPsRefValid];
            for (; j < avail; j++) {  // cc:226-298
                const int k = it0 + j;
                it = k + 1;
                int inl = A.W.counts[(size_t)b * A.W.max_draws + j];
                if (inl < 0) {
                    status |= ORBX_PNP_STATUS_BAD_DRAW;
                    inl = 0;
                }
                if (inl < min_inl) continue;  // cc:261
                if (inl > best) {             // cc:265: a tie keeps the earlier iteration
                    best = inl;
                    best_it = k;
                    const double* H = A.W.hyp + ((size_t)b * A.W.max_draws + j) * 12;
                    for (int i = 0; i < 12; i++) best_pose[i] = H[i];
                    for (int r = 0; r < 3; r++) {  // cc:270-276
                        for (int q = 0; q < 3; q++) best_T[4 * r + q] = (float)H[3 * r + q];
                        best_T[4 * r + 3] = (float)H[9 + r];
                    }
                    ref_valid = 0;
                    st[kPsRefValid] = 0;
                }
                if (!ref_valid) {  // Refine() on the new best set: the workgroup's turn
                    ev = 1;
                    j++;
                    break;
                }
                if (st[kPsRefInliers] > min_inl) {  // cc:280, cc:364 with the stored result
                    s_res[0] = 1;
                    s_res[1] = 1;
                    s_res[2] = st[kPsRefInliers];
                    j++;
                    break;
                }
            }
            s_ev[0] = ev;
            s_ev[1] = j;
            s_ev[2] = 0;
            s_res[3] = it;
            s_res[4] = best;
            s_res[5] = best_it;
            s_res[6] = status;
        }
        __syncthreads();
        if (s_ev[0] == 0) break;
        // Refine (cc:326-378): mvbBestInliers from the best pose
        if (tid < 12) s_P[tid] = best_pose[tid];
        __syncthreads();
        for (int i = tid; i < N; i += kPnpThreads) flags[i] = pnp_inlier(A.K, pts, c, i, s_P) ? 1 : 0;
        __syncthreads();
        if (tid == 0) {
            const epnp::Mem pws{ref, 1}, us{ref + 3 * c, 1}, alphas{ref + 5 * c, 1}, pcs{ref + 9 * c, 1};
            int m = 0;
            for (int i = 0; i < N; i++)
                if (flags[i]) {  // cc:332-351
                    us(2 * m) = (double)pts[i];
                    us(2 * m + 1) = (double)pts[c + i];
                    pws(3 * m) = (double)pts[2 * c + i];
                    pws(3 * m + 1) = (double)pts[3 * c + i];
                    pws(3 * m + 2) = (double)pts[4 * c + i];
                    m++;
                }
            double R[9], t[3];
            if (m > 0) {
                epnp::compute_pose(m, pws, us, alphas, pcs, epnp::Mem{s_W, 1}, A.K, R, t);
            } else {
                for (int i = 0; i < 9; i++) R[i] = __builtin_nan("");
                for (int i = 0; i < 3; i++) t[i] = __builtin_nan("");
            }
            for (int i = 0; i < 9; i++) ref_pose[i] = s_P[i] = R[i];
            for (int i = 0; i < 3; i++) ref_pose[9 + i] = s_P[9 + i] = t[i];
        }
        __syncthreads();
        {
            int mine = 0;
            for (int i = tid; i < N; i += kPnpThreads) mine += pnp_inlier(A.K, pts, c, i, s_P) ? 1 : 0;
            if (mine) atomicAdd(&s_ev[2], mine);
        }
        __syncthreads();
        if (tid == 0) {
            st[kPsRefValid] = 1;
            st[kPsRefInliers] = s_ev[2];
            if (s_ev[2] > min_inl) {  // cc:364
                s_res[0] = 1;
                s_res[1] = 1;
                s_res[2] = s_ev[2];
                s_ev[0] = 0;
            }
        }
        __syncthreads();
        const bool done = s_ev[0] == 0;
        __syncthreads();  // before thread 0 writes the next event
        if (done) break;
    }
    if (tid == 0) {
        if (!s_res[0]) {
            if (N < min_inl) {
                s_res[7] = 1;  // cc:210-214
            } else if (avail < window) {
                s_res[7] = 1;  // the next iteration has no draws
                s_res[6] |= ORBX_PNP_STATUS_NO_DRAWS;
            } else if (s_res[3] >= max_its) {  // cc:302-319
                s_res[7] = 1;
                if (s_res[4] >= min_inl) {
                    s_res[0] = 1;
                    s_res[2] = s_res[4];
                }
            }
        }
    }
    __syncthreads();
    const int found = s_res[0], refined = s_res[1];
    const orbx_pnp_result& o = A.out;
    const size_t orow = (size_t)b * A.out_cap;
    for (int i = tid; i < slots; i += kPnpThreads) {
        if (o.inliers) o.inliers[orow + i] = 0;
        if (o.frame_mp) o.frame_mp[orow + i] = -1;
    }
    if (tid < 12) s_P[tid] = refined ? ref_pose[tid] : best_pose[tid];
    __syncthreads();
    if (found && (o.inliers || o.frame_mp)) {
        const int32_t* idx = A.W.idx + (size_t)b * c;
        const int32_t* mpid = A.W.mpid + (size_t)b * c;
        for (int i = tid; i < N; i += kPnpThreads)
            if (pnp_inlier(A.K, pts, c, i, s_P)) {  // cc:284-289, 311-316; Tracking.cc:1600-1612
                if (o.inliers) o.inliers[orow + idx[i]] = 1;
                if (o.frame_mp) o.frame_mp[orow + idx[i]] = mpid[i];
            }
    }
    if (tid == 0) {
        if (o.found) o.found[b] = found;
        if (o.no_more) o.no_more[b] = s_res[7];
        if (o.n_inliers) o.n_inliers[b] = s_res[2];
        if (o.refined) o.refined[b] = refined;
        if (o.Tcw) {
            float* T = o.Tcw + (size_t)b * 12;
            for (int r = 0; r < 3; r++) {
                for (int q = 0; q < 3; q++)
                    T[4 * r + q] = !found ? 0.0f : (refined ? (float)s_P[3 * r + q] : best_T[4 * r + q]);
                T[4 * r + 3] = !found ? 0.0f : (refined ? (float)s_P[9 + r] : best_T[4 * r + 3]);
            }
        }
        if (o.best_Tcw)
            for (int i = 0; i < 12; i++) o.best_Tcw[(size_t)b * 12 + i] = best_T[i];
        if (o.best_inliers) o.best_inliers[b] = s_res[4];
        if (o.best_iteration) o.best_iteration[b] = s_res[5];
        if (o.iterations) o.iterations[b] = s_res[3];
        if (o.n_corr) o.n_corr[b] = N;
        if (o.min_inliers_used) o.min_inliers_used[b] = min_inl;
        if (o.max_its_used) o.max_its_used[b] = max_its;
        if (o.status) o.status[b] = s_res[6];
        st[kPsIterations] = s_res[3];
        st[kPsBestInliers] = s_res[4];
        st[kPsBestIteration] = s_res[5];
        st[kPsStatus] = s_res[6];
    }
}

}  // namespace orbx

// ---------------------------------------------------------------------------------------
// Host side

struct orbx_pnp {
    orbx_matcher* matcher = nullptr;
    int device = 0, max_batch = 0, cap = 0, max_draws = 0;
    hipStream_t stream = nullptr;  // the matcher's
    char* work = nullptr;          // PnpWork arrays
    int32_t* tables = nullptr;     // [2][cap + 1]
    orbx::DeviceBuffer stage;      // the single host form's candidate and results
    orbx::PnpWork W{};
    std::vector<int32_t> h_tables;
    // the batch in force (set): what iterate needs
    bool is_set = false;
    int batch = 0, batch_cap = 0, n_draws = 0, max_iterations = 0;
    orbx::epnp::Camera K{};
    const int32_t* draws = nullptr;
    // the single host form's candidate (set): its result block, the device addresses in it,
    // and iterate's destinations
    orbx::HostStage host{orbx::up256};
    orbx_pnp_result host_dev{}, host_out{};
};

namespace {

using namespace orbx;

// SetRansacParameters (cc:141-183) for N = n with the host's libm: the adjusted
// mRansacMinInliers and mRansacMaxIts
void ransac_parameters(int n, const orbx_pnp_batch* in, int32_t* min_inliers, int32_t* max_its) {
    int nmin = (int)((float)n * in->epsilon);  // cc:161: a float product, truncated
    if (nmin < in->min_inliers) nmin = in->min_inliers;
    if (nmin < in->min_set) nmin = in->min_set;
    *min_inliers = nmin;
    *max_its = 1;
    if (n < nmin || n <= 0) return;  // never used: iterate answers "no more" first
    float eps = in->epsilon;
    if (eps < (float)nmin / n) eps = (float)nmin / n;  // cc:171-172
    int its;
    if (nmin == n) {
        its = 1;
    } else {
        const double v = std::log(1 - in->probability) / std::log(1 - std::pow((double)eps, 3.0));  // cc:181
        its = !(v <= (double)in->max_iterations) ? in->max_iterations : (int)std::ceil(v);
    }
    *max_its = std::max(1, std::min(its, in->max_iterations));
}

// the argument checks of orbx_pnp_set_batch_device and orbx_pnp_set, before any GPU work
int check_batch(const orbx_pnp* s, const orbx_pnp_batch* in) {
    const int B = in->batch, cap = in->cap;
    if (in->min_set != 4) return fail(ORBX_ERR_ARG, "min_set must be 4");
    if (B < 0 || B > s->max_batch || cap < 1 || cap > s->cap || in->n_mp < 0 || in->nlevels < 1 ||
        in->nlevels > ORBX_MAX_LEVELS || in->min_inliers < 0 || in->max_iterations < 1 || in->n_draws < 1 ||
        in->n_draws > s->max_draws || in->max_iterations > in->n_draws ||
        !(in->probability > 0.0 && in->probability < 1.0) || !(in->epsilon >= 0.0f && in->epsilon <= 1.0f) ||
        !(in->th2 >= 0.0f))
        return fail(ORBX_ERR_ARG, "bad argument");
    if (!in->level_sigma2) return fail(ORBX_ERR_ARG, "null host array");
    if (B > 0 && (!in->kps || !in->n || !in->matches || !in->draws || (in->n_mp > 0 && !in->mp_pos)))
        return fail(ORBX_ERR_ARG, "null buffer");
    return ORBX_OK;
}

}  // namespace

extern "C" {

int orbx_pnp_create(orbx_matcher* m, int max_batch, int cap, int max_draws, orbx_pnp** out) {
    if (!out) return fail(ORBX_ERR_ARG, "null argument");
    *out = nullptr;
    if (!m) return fail(ORBX_ERR_ARG, "null matcher");
    if (max_batch < 1 || cap < 1 || max_draws < 1 || max_draws > ORBX_PNP_MAX_DRAWS)
        return fail(ORBX_ERR_ARG, "bad argument");
    if ((size_t)max_batch * (size_t)cap * 12 >= ((size_t)1 << 31) ||
        (size_t)max_batch * (size_t)max_draws * 12 >= ((size_t)1 << 31))
        return fail(ORBX_ERR_ARG, "max_batch x cap or x max_draws too large");
    orbx_pnp* s = new (std::nothrow) orbx_pnp();
    if (!s) return fail(ORBX_ERR_ARG, "out of host memory");
    s->matcher = m;
    s->device = matcher_device(m);
    s->stream = matcher_stream(m);
    s->max_batch = max_batch;
    s->cap = cap;
    s->max_draws = max_draws;
    const size_t B = (size_t)max_batch, slots = B * cap, its = B * max_draws;
    Layout L(up256);
    const size_t o_hyp = L.take(its * 12 * 8), o_pose = L.take(B * 24 * 8), o_ref = L.take(slots * 12 * 8),
                 o_pts = L.take(slots * 6 * 4), o_best = L.take(B * 12 * 4), o_idx = L.take(slots * 4),
                 o_mpid = L.take(slots * 4), o_state = L.take(B * kPnpState * 4), o_counts = L.take(its * 4),
                 o_flags = L.take(slots);
    hipError_t e = hipSetDevice(s->device);
    if (e == hipSuccess) e = hipMalloc((void**)&s->work, L.total());
    if (e == hipSuccess) e = hipMalloc((void**)&s->tables, 2 * ((size_t)cap + 1) * 4);
    if (e != hipSuccess) {
        if (s->work) (void)hipFree(s->work);
        if (s->tables) (void)hipFree(s->tables);
        delete s;
        set_last_error(std::string("orbx_pnp_create: ") + hipGetErrorString(e));
        return ORBX_ERR_HIP;
    }
    s->W.hyp = (double*)(s->work + o_hyp);
    s->W.pose = (double*)(s->work + o_pose);
    s->W.ref = (double*)(s->work + o_ref);
    s->W.pts = (float*)(s->work + o_pts);
    s->W.best_T = (float*)(s->work + o_best);
    s->W.idx = (int32_t*)(s->work + o_idx);
    s->W.mpid = (int32_t*)(s->work + o_mpid);
    s->W.state = (int32_t*)(s->work + o_state);
    s->W.counts = (int32_t*)(s->work + o_counts);
    s->W.flags = (uint8_t*)(s->work + o_flags);
    s->W.cap = cap;
    s->W.max_draws = max_draws;
    *out = s;
    return ORBX_OK;
}

void orbx_pnp_destroy(orbx_pnp* s) {
    if (!s || orbx::unloading()) return;  // DESIGN.md §1 "Teardown"
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    if (s->work) (void)hipFree(s->work);
    if (s->tables) (void)hipFree(s->tables);
    s->stage.release();
    delete s;
}

int orbx_pnp_set_batch_device(orbx_pnp* s, const orbx_pnp_batch* in, void* stream) {
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
    PnpSetArgs A{};
    A.kps = in->kps;
    A.n = in->n;
    A.matches = in->matches;
    A.pos = in->mp_pos;
    A.n_mp = in->n_mp;
    A.cap = cap;
    A.nlevels = in->nlevels;
    for (int l = 0; l < in->nlevels; l++) A.sigma2[l] = in->level_sigma2[l];
    A.th2 = in->th2;
    s->h_tables.resize(2 * ((size_t)cap + 1));
    for (int n = 0; n <= cap; n++) ransac_parameters(n, in, &s->h_tables[n], &s->h_tables[(size_t)cap + 1 + n]);
    HIP_TRY(hipMemcpyAsync(s->tables, s->h_tables.data(), s->h_tables.size() * 4, hipMemcpyHostToDevice, st));
    A.min_inl = s->tables;
    A.its = s->tables + cap + 1;
    A.W = s->W;
    k_pnp_set<<<B, kPnpThreads, 0, st>>>(A);
    HIP_TRY(hipGetLastError());
    s->batch = B;
    s->batch_cap = cap;
    s->n_draws = in->n_draws;
    s->max_iterations = in->max_iterations;
    s->K = epnp::Camera{(double)in->fx, (double)in->fy, (double)in->cx, (double)in->cy};  // cc:121-124
    s->draws = in->draws;
    s->is_set = true;
    return ORBX_OK;
}

int orbx_pnp_iterate_device(orbx_pnp* s, int n_iterations, const orbx_pnp_result* out, void* stream) {
    if (!s || !out || n_iterations < 0) return fail(ORBX_ERR_ARG, "bad argument");
    if (!s->is_set) return fail(ORBX_ERR_STATE, "orbx_pnp_iterate before orbx_pnp_set");
    if (s->batch == 0) return ORBX_OK;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = stream ? (hipStream_t)stream : s->stream;
    PnpRunArgs A{};
    A.W = s->W;
    A.draws = s->draws;
    A.n_draws = s->n_draws;
    A.n_iterations = n_iterations;
    A.out_cap = s->batch_cap;
    A.K = s->K;
    A.out = *out;
    // no candidate's window is longer than this (cc:226: to the cap, or n_iterations more)
    const int widest = std::min(std::max(n_iterations, s->max_iterations), s->n_draws);
    if (widest > 0) {
        dim3 gh((unsigned)((widest + kPnpHypLanes - 1) / kPnpHypLanes), (unsigned)s->batch);
        k_pnp_hyp<<<gh, kPnpHypLanes, 0, st>>>(A);
        HIP_TRY(hipGetLastError());
        dim3 gc((unsigned)((widest + kPnpWaves - 1) / kPnpWaves), (unsigned)s->batch);
        k_pnp_count<<<gc, kPnpThreads, 0, st>>>(A);
        HIP_TRY(hipGetLastError());
    }
    k_pnp_walk<<<s->batch, kPnpThreads, 0, st>>>(A);
    HIP_TRY(hipGetLastError());
    return ORBX_OK;
}

int orbx_pnp_set(orbx_pnp* s, const orbx_pnp_batch* in) {
    if (!s || !in) return fail(ORBX_ERR_ARG, "null argument");
    if (in->batch != 1) return fail(ORBX_ERR_ARG, "the host form takes one candidate");
    int rc = check_batch(s, in);
    if (rc) return rc;
    const int cap = in->cap;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    int n = in->n[0];
    n = n < 0 ? 0 : (n > cap ? cap : n);
    const size_t N = (size_t)n, C = (size_t)cap, nd = (size_t)in->n_draws;
    orbx_pnp_batch d = *in;
    HostStage h(up256);
    h.in(&d.n, in->n, 1, 1);
    h.in(&d.kps, in->kps, N, C);
    h.in(&d.matches, in->matches, N, C);
    h.in(&d.mp_pos, in->mp_pos, 3 * (size_t)in->n_mp, 3 * (size_t)(in->n_mp > 0 ? in->n_mp : 1));
    h.in(&d.draws, in->draws, 4 * nd, 4 * nd);
    orbx_pnp_result& r = s->host_dev;
    const orbx_pnp_result& o = s->host_out;
    h.out(&r.found, &o.found, 1, 1);
    h.out(&r.no_more, &o.no_more, 1, 1);
    h.out(&r.n_inliers, &o.n_inliers, 1, 1);
    h.out(&r.refined, &o.refined, 1, 1);
    h.out(&r.best_inliers, &o.best_inliers, 1, 1);
    h.out(&r.best_iteration, &o.best_iteration, 1, 1);
    h.out(&r.iterations, &o.iterations, 1, 1);
    h.out(&r.n_corr, &o.n_corr, 1, 1);
    h.out(&r.min_inliers_used, &o.min_inliers_used, 1, 1);
    h.out(&r.max_its_used, &o.max_its_used, 1, 1);
    h.out(&r.status, &o.status, 1, 1);
    h.out(&r.Tcw, &o.Tcw, 12, 12);
    h.out(&r.best_Tcw, &o.best_Tcw, 12, 12);
    h.out(&r.frame_mp, &o.frame_mp, N, C);
    h.out(&r.inliers, &o.inliers, N, C);  // last: iterate downloads up to the n in use
    HIP_TRY(h.stage(s->stage, st));
    rc = orbx_pnp_set_batch_device(s, &d, st);
    if (rc) return rc;
    s->host = std::move(h);  // iterate reads the result entries only: they point into the handle
    return ORBX_OK;
}

int orbx_pnp_iterate(orbx_pnp* s, int n_iterations, const orbx_pnp_result* out) {
    if (!s || !out || n_iterations < 0) return fail(ORBX_ERR_ARG, "bad argument");
    if (!s->host.staged()) return fail(ORBX_ERR_STATE, "orbx_pnp_iterate before orbx_pnp_set");
    CallClock clock(s->matcher);
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    const int rc = orbx_pnp_iterate_device(s, n_iterations, &s->host_dev, st);
    if (rc) return rc;
    s->host_out = *out;
    HIP_TRY(s->host.download(st, s->host.results_in_use()));
    return ORBX_OK;
}

int orbx_pnp_draws(int32_t* draws, int n, int iterations) {
    if (!draws || n < 0 || iterations < 0) return fail(ORBX_ERR_ARG, "bad argument");
    for (int k = 0; k < iterations; k++)
        for (int j = 0; j < 4; j++) {
            const int d = n - j;  // RandomInt(0, vAvailableIndices.size() - 1), DUtils/Random.cpp:47-49
            draws[(size_t)k * 4 + j] = d > 0 ? (int)(((double)rand() / ((double)RAND_MAX + 1.0)) * d) : 0;
        }
    return ORBX_OK;
}

}  // extern "C"
