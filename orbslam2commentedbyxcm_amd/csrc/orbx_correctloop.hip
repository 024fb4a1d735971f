// orbx_correctloop.hip -- LoopClosing::CorrectLoop's work on the covisibility graph in HBM
// (LoopClosing.cc:482-571, 595-618), the assembly of Optimizer::OptimizeEssentialGraph's tables
// (Optimizer.cc:913-1089, 1125-1133) and MapPoint::UpdateNormalAndDepth (MapPoint.cc:386-439) in
// its general form.  DESIGN.md 4.27.
//
// The work is integer gathers over the graph's rows and the observation CSR plus a little double
// arithmetic per element: it is bound by latency and by the number of launches.  Every float sum
// has one owner and a fixed order (a point's thread walks its observers in ascending keyframe id);
// float inputs are widened to double, everything after is double, outputs are rounded to float
// once.  Integer atomics mark, count and take minima; every stored table
// is then laid out by scans, so its bytes do not depend on scheduling.  No workgroup waits on
// another.
//
// Propagation (orbx_correct_loop_propagate_device), after UpdateConnections(cur):
//   k_cl_members  one workgroup: the connected set without bad keyframes, then cur; per member the
//                 non-corrected pose bytes, CorrectedSim3 and its pose [R | t / s] (workspace)
//   k_cl_points   one thread per (member, slot of its cleaned row): the thread of the point's
//                 owner (the smallest member id among its observers) corrects the point and runs
//                 UpdateNormalAndDepth with the poses the reference has at that moment
//   k_cl_poses    the corrected poses into kf_Tcw
//   then UpdateConnections of every member from the device list
// Assembly (orbx_essential_graph_assemble_device):
//   k_eg_snapshot one workgroup per member: its ordered list, its rank among the members by id
//   UpdateConnections of every member
//   k_eg_lc       one workgroup per member in id order, twice (count, write): LoopConnections
//   k_eg_scan1    one workgroup: lc_off; the vertex rows
//   k_eg_edges    one thread per keyframe, twice (count, write): the kind-1 edges; the write
//                 launch also lays the kind-0 edges of one LoopConnections row per thread
//   k_eg_scan2    one workgroup: edge offsets; the envelope's numbering
//   k_eg_finish   pt_ref, the pose rows, the envelope's sum
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "orbx.h"
#include "orbx_covis.h"
#include "orbx_host.h"
#include "orbx_sim3.h"

namespace orbx {
namespace {

constexpr int kNdThreads = 256;
constexpr int kNdMaxLevels = 32;

struct NdArgs {
    const float* kf_Tcw;
    const orbx_keypoint* kf_keys_un;
    const int32_t* mp_ref_kf;
    const float* mp_pos;
    float* normal;
    float* max_distance;
    float* min_distance;
    const int32_t* ids;  // NULL: every MapPoint of the last refresh
    int n;               // entries of ids, or the MapPoints
    int nlevels;
    int32_t* status;
    float scale[kNdMaxLevels];
};

// GetCameraCenter() = -Rcw^T tcw of rows 0..2 of a pose (KeyFrame.cc:67-70), in double
__device__ __forceinline__ void nd_centre(const float* T, double (&Ow)[3]) {
    const double t0 = (double)T[3], t1 = (double)T[7], t2 = (double)T[11];
#pragma unroll
    for (int c = 0; c < 3; c++) Ow[c] = -(((double)T[c] * t0 + (double)T[4 + c] * t1) + (double)T[8 + c] * t2);
}

// MapPoint.cc:400-437 for point p at position P; pose(kf) gives the rows of keyframe kf's Tcw.
// Returns the status bits.  A point without observers is left untouched.
template <class Pose>
__device__ int nd_point(const CovisDev& D, const NdArgs& A, int p, const double (&P)[3], Pose pose) {
    const int o0 = D.obs_off[p], o1 = D.obs_off[p + 1];
    if (o1 <= o0) return 0;  // cc:400
    const int ref = A.mp_ref_kf[p];
    if (ref < 0 || ref >= D.nk) return ORBX_NORMAL_STATUS_BAD_INDEX;
    double nx = 0.0, ny = 0.0, nz = 0.0;
    int idx = -1;
    for (int o = o0; o < o1; o++) {  // cc:406-414, ascending keyframe id
        const int kf = D.obs_kf[o];
        if (kf == ref) idx = D.obs_idx[o];
        double Ow[3];
        nd_centre(pose(kf), Ow);
        const double x = P[0] - Ow[0], y = P[1] - Ow[1], z = P[2] - Ow[2];
        const double d = sqrt((x * x + y * y) + z * z);
        nx += x / d;
        ny += y / d;
        nz += z / d;
    }
    int st = 0;
    if (idx < 0) {  // observations[pRefKF] inserts index 0 (cc:426)
        idx = 0;
        st = ORBX_NORMAL_STATUS_REF_NOT_OBSERVER;
    }
    double Or[3];
    nd_centre(pose(ref), Or);
    const double x = P[0] - Or[0], y = P[1] - Or[1], z = P[2] - Or[2];
    const double dist = sqrt((x * x + y * y) + z * z);
    const int level = clampi(A.kf_keys_un[(size_t)ref * D.cap + idx].octave, 0, A.nlevels - 1);
    const double dmax = dist * (double)A.scale[level];
    const double n = (double)(o1 - o0);
    A.normal[3 * (size_t)p] = (float)(nx / n);
    A.normal[3 * (size_t)p + 1] = (float)(ny / n);
    A.normal[3 * (size_t)p + 2] = (float)(nz / n);
    A.max_distance[p] = (float)dmax;
    A.min_distance[p] = (float)(dmax / (double)A.scale[A.nlevels - 1]);
    return st;
}

__global__ __launch_bounds__(kNdThreads) void k_normal_depth(CovisDev D, NdArgs A) {
    const int j = blockIdx.x * kNdThreads + threadIdx.x;
    int st = 0;
    if (j < A.n) {
        const int p = A.ids ? A.ids[j] : j;
        if (p < 0 || p >= D.nm) {
            st = ORBX_NORMAL_STATUS_BAD_INDEX;
        } else if (!(D.mp_bad && D.mp_bad[p])) {  // cc:393
            const double P[3] = {(double)A.mp_pos[3 * (size_t)p], (double)A.mp_pos[3 * (size_t)p + 1], (double)A.mp_pos[3 * (size_t)p + 2]};
            st = nd_point(D, A, p, P, [&](int kf) { return A.kf_Tcw + (size_t)kf * 12; });
        }
    }
    // one integer atomic per wave that has a bit to report
    for (int d = 32; d > 0; d >>= 1) st |= __shfl_xor(st, d, 64);
    if (st && (threadIdx.x & 63) == 0) atomicOr(A.status, st);
}

// ---- LoopClosing.cc:482-571 ----
struct ClArgs {
    int cur, matched;  // matched < 0: Scw is given
    const double* Scw;
    const float *sim3_R, *sim3_t, *sim3_s;
    float* kf_Tcw;
    float* mp_pos;
    int32_t* by_kf;
    int32_t* corr_ref;
    int32_t* conn;
    int32_t* n_conn;
    double* corr_S;
    int32_t* kf_corr;
    float* kf_Tcw_nc;
    float* Tc;  // [max_conn + 1][12] the corrected poses
    NdArgs nd;
};

// g2o::Sim3(R, t, s) of float arrays (LoopClosing.cc:359): Quaterniond(R), not normalised
__device__ __forceinline__ S3 s3_from_rts(const float* Rf, const float* t, double s) {
    double R[3][3], q[4];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) R[r][c] = (double)Rf[3 * r + c];
    lm::quat_from_matrix(R, q);
    return S3{q[0], q[1], q[2], q[3], (double)t[0], (double)t[1], (double)t[2], s};
}

// member j of the connected set is keyframe i (cc:501-523)
__device__ void cl_member(const ClArgs& A, int j, int i, const S3& Scw, const double* Twc) {
    A.conn[j] = i;
    A.kf_corr[i] = j;
    const float* Tiw = A.kf_Tcw + (size_t)i * 12;
    for (int c = 0; c < 12; c++) A.kf_Tcw_nc[(size_t)j * 12 + c] = Tiw[c];
    S3 corr = Scw;
    if (i != A.cur) {  // Tic = Tiw * Twc (cc:508), Sim3(Ric, tic, 1) * Scw (cc:511-513)
        double R[3][3], q[4], t[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const double a0 = (double)Tiw[4 * r], a1 = (double)Tiw[4 * r + 1], a2 = (double)Tiw[4 * r + 2];
#pragma unroll
            for (int c = 0; c < 3; c++) R[r][c] = (a0 * Twc[c] + a1 * Twc[4 + c]) + a2 * Twc[8 + c];
            t[r] = ((a0 * Twc[3] + a1 * Twc[7]) + a2 * Twc[11]) + (double)Tiw[4 * r + 3];
        }
        lm::quat_from_matrix(R, q);
        corr = s3_mul(S3{q[0], q[1], q[2], q[3], t[0], t[1], t[2], 1.0}, Scw);
    }
    s3_store(A.corr_S + (size_t)j * 8, corr);
    s3_to_tcw(corr, A.Tc + (size_t)j * 12);  // cc:558-564
}

__global__ __launch_bounds__(kCvThreads) void k_cl_members(CovisDev D, ClArgs A) {
    __shared__ int s_w[kCvWaves];
    __shared__ S3 s_Scw;
    __shared__ double s_Twc[12];
    const int tid = threadIdx.x;
    if (tid == 0) {
        s_Scw = A.matched < 0 ? s3_load(A.Scw)
                              : s3_mul(s3_from_rts(A.sim3_R, A.sim3_t, (double)A.sim3_s[0]), s3_from_tcw(A.kf_Tcw + (size_t)A.matched * 12));
        // GetPoseInverse() (KeyFrame.cc:59-70): [Rcw^T | -Rcw^T tcw]
        const float* T = A.kf_Tcw + (size_t)A.cur * 12;
        double Ow[3];
        nd_centre(T, Ow);
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) s_Twc[4 * r + c] = (double)T[4 * c + r];
            s_Twc[4 * r + 3] = Ow[r];
        }
    }
    __syncthreads();
    const S3 Scw = s_Scw;
    const int nn = clampi(D.ord_n[A.cur], 0, D.max_conn);
    const size_t c0 = (size_t)A.cur * D.max_conn;
    int n = 0;
    for (int j0 = 0; j0 < nn; j0 += kCvThreads) {  // cc:488, without the bad keyframes
        const int j = j0 + tid;
        const int kf = j < nn ? D.ord_kf[c0 + j] : -1;
        const bool good = kf >= 0 && kf < D.nk && kf != A.cur && !(D.kf_bad && D.kf_bad[kf]);
        int tot;
        const int pos = cv_block_scan(good, s_w, tot);
        if (good) cl_member(A, n + pos, kf, Scw, s_Twc);
        n += tot;
    }
    if (tid == 0) {  // cc:489
        cl_member(A, n, A.cur, Scw, s_Twc);
        *A.n_conn = n + 1;
    }
}

__global__ __launch_bounds__(kNdThreads) void k_cl_points(CovisDev D, ClArgs A) {
    const long long s = (long long)blockIdx.x * kNdThreads + threadIdx.x;
    const int j = (int)(s / D.cap), slot = (int)(s - (long long)j * D.cap);
    if (j >= *A.n_conn) return;
    const int i = A.conn[j];
    if ((D.kf_bad && D.kf_bad[i]) || slot >= clampi(D.kf_n[i], 0, D.cap)) return;
    const int p = D.clean[(size_t)i * D.cap + slot];
    if (p < 0 || (D.mp_bad && D.mp_bad[p]) || A.by_kf[p] == A.cur) return;  // cc:537-542
    // the first member in key order that holds the point corrects it (cc:526, 541)
    const int o0 = D.obs_off[p], o1 = D.obs_off[p + 1];
    int owner = -1;
    for (int o = o0; o < o1 && owner < 0; o++)
        if (A.kf_corr[D.obs_kf[o]] >= 0) owner = D.obs_kf[o];
    if (owner != i) return;
    const S3 Siw = s3_from_tcw(A.kf_Tcw + (size_t)i * 12), Swi = s3_inverse(s3_load(A.corr_S + (size_t)j * 8));
    double x, y, z, X, Y, Z;
    s3_map(Siw, (double)A.mp_pos[3 * (size_t)p], (double)A.mp_pos[3 * (size_t)p + 1], (double)A.mp_pos[3 * (size_t)p + 2], x, y, z);
    s3_map(Swi, x, y, z, X, Y, Z);  // cc:547
    const float Pf[3] = {(float)X, (float)Y, (float)Z};
    for (int c = 0; c < 3; c++) A.mp_pos[3 * (size_t)p + c] = Pf[c];
    A.by_kf[p] = A.cur;
    A.corr_ref[p] = i;
    // cc:554: the members before i in key order have their corrected pose (cc:566), the others not yet
    const double P[3] = {(double)Pf[0], (double)Pf[1], (double)Pf[2]};
    const int st = nd_point(D, A.nd, p, P, [&](int kf) -> const float* {
        const int r = A.kf_corr[kf];
        return r >= 0 && kf < i ? A.Tc + (size_t)r * 12 : A.kf_Tcw + (size_t)kf * 12;
    });
    if (st) atomicOr(A.nd.status, st);
}

__global__ void k_cl_poses(ClArgs A) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = t / 12, c = t - 12 * j;
    if (j < *A.n_conn) A.kf_Tcw[(size_t)A.conn[j] * 12 + c] = A.Tc[(size_t)j * 12 + c];  // cc:566
}

// ---- LoopClosing.cc:595-618 and the tables of Optimizer.cc:913-1089, 1125-1133 ----
struct EgWs {
    int32_t* prev;     // [max_conn + 1][max_conn] the members' ordered lists at entry
    int32_t* prev_n;   // [max_conn + 1]
    int32_t* prow_kf;  // [max_conn + 1][max_conn] the members' rows at entry
    int32_t* prow_w;   // [max_conn + 1][max_conn]
    int32_t* prow_n;   // [max_conn + 1]
    int32_t* srt;      // [max_conn + 1] rank by id -> position in conn
    int32_t* rank_of;  // [max_conn + 1] position in conn -> rank by id
    int32_t* lc_cnt;   // [max_conn + 1] by rank
    int32_t* a0_cnt;   // [max_conn + 1] admitted kind-0 edges by rank
    int32_t* a0_off;   // [max_conn + 2]
    int32_t* e_cnt;    // [K] kind-1 edges by row
    int32_t* e_off;    // [K + 1]
    int32_t* has;      // [K] the row has an edge
    int32_t* eidx;     // [K] the row's number in the envelope, or -1
    int32_t* first;    // [K] by envelope number
    int32_t* misc;     // {F, lc_over}
};

__device__ __forceinline__ int eg_members(const CovisDev& D, const orbx_essential_graph_assembly& A) {
    return clampi(*A.n_conn, 0, D.max_conn + 1);
}

__global__ __launch_bounds__(kNdThreads) void k_eg_snapshot(CovisDev D, orbx_essential_graph_assembly A, EgWs W) {
    __shared__ int s_rank;
    const int j = blockIdx.x, tid = threadIdx.x, n = eg_members(D, A);
    if (j >= n) return;
    if (tid == 0) s_rank = 0;
    __syncthreads();
    const int i = A.conn[j];
    const int m = clampi(D.ord_n[i], 0, D.max_conn);
    const int mr = clampi(D.row_n[i], 0, D.max_conn);
    for (int e = tid; e < m; e += kNdThreads) W.prev[(size_t)j * D.max_conn + e] = D.ord_kf[(size_t)i * D.max_conn + e];
    for (int e = tid; e < mr; e += kNdThreads) {
        W.prow_kf[(size_t)j * D.max_conn + e] = D.row_kf[(size_t)i * D.max_conn + e];
        W.prow_w[(size_t)j * D.max_conn + e] = D.row_w[(size_t)i * D.max_conn + e];
    }
    int r = 0;
    for (int k = tid; k < n; k += kNdThreads) r += A.conn[k] < i;
    if (r) atomicAdd(&s_rank, r);
    __syncthreads();
    if (tid == 0) {
        W.prev_n[j] = m;
        W.prow_n[j] = mr;
        W.srt[s_rank] = j;
        W.rank_of[j] = s_rank;
        A.lc_member[s_rank] = i;
    }
}

__device__ __forceinline__ bool eg_admitted(const orbx_essential_graph_assembly& A, int mi, int mj, int w) {
    return (mi == A.cur_kf && mj == A.loop_kf) || w >= A.min_feat;  // cc:966-968
}

__global__ __launch_bounds__(kCvThreads) void k_eg_lc(CovisDev D, orbx_essential_graph_assembly A, EgWs W, int write) {
    __shared__ int s_w[kCvWaves];
    __shared__ int s_adm;
    const int r = blockIdx.x, tid = threadIdx.x;
    if (r >= eg_members(D, A)) return;
    const int j = W.srt[r], i = A.conn[j];
    if (tid == 0) s_adm = 0;
    const int m = clampi(D.row_n[i], 0, D.max_conn);
    const size_t r0 = (size_t)i * D.max_conn;
    const int32_t* prow_kf = W.prow_kf + (size_t)j * D.max_conn;
    const int nr = W.prow_n[j];
    auto old_weight = [&](int kf) {  // keyframe kf in i's row at entry, 0 if absent
        int lo = 0, hi = nr;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (prow_kf[mid] < kf) lo = mid + 1;
            else hi = mid;
        }
        return lo < nr && prow_kf[lo] == kf ? W.prow_w[(size_t)j * D.max_conn + lo] : 0;
    };
    // vpPreviousNeighbors is taken inside the sequential loop (cc:598-600): when the UpdateConnections
    // of a member before i in the list added or changed its entry in i's row (KeyFrame.cc:139-153),
    // UpdateBestCovisibles had re-ordered i's whole row, entries below 15 included
    int resorted = 0;
    for (int e = tid; e < m; e += kCvThreads) {
        const int kf = D.row_kf[r0 + e], w = D.row_w[r0 + e];
        const int jj = A.kf_corr[kf];
        if (jj >= 0 && jj < j && (w >= kCvTh || D.kmax[kf] == i) && old_weight(kf) != w) resorted = 1;
    }
    resorted = __syncthreads_or(resorted);
    const int32_t* prev = resorted ? prow_kf : W.prev + (size_t)j * D.max_conn;
    const int base0 = write ? A.lc_off[r] : 0;
    const int np = resorted ? nr : W.prev_n[j];
    int base = 0, adm = 0, bad = 0;
    for (int e0 = 0; e0 < m; e0 += kCvThreads) {
        const int e = e0 + tid;
        const int kf = e < m ? D.row_kf[r0 + e] : -1;
        bool in = kf >= 0 && A.kf_corr[kf] < 0;  // cc:611-613: without the members
        for (int k = 0; k < np && in; k++) in = prev[k] != kf;  // cc:607-609: without the previous neighbours
        int tot;
        const int pos = cv_block_scan(in, s_w, tot);
        if (in && write) {
            const int w = D.row_w[r0 + e];
            const long long at = (long long)base0 + base + pos;
            if (at < A.max_lc) {
                A.lc_kf[at] = kf;
                A.lc_w[at] = w;
            }
            if (eg_admitted(A, i, kf, w)) {
                const int a = A.kf_row[i], b = kf < D.nk ? A.kf_row[kf] : -1;
                if (a >= 0 && b >= 0) {
                    adm++;
                    W.has[a] = 1;
                    W.has[b] = 1;
                } else {
                    bad = 1;
                }
            }
        }
        base += tot;
    }
    if (!write) {
        if (tid == 0) W.lc_cnt[r] = base;
        return;
    }
    if (adm) atomicAdd(&s_adm, adm);
    if (bad) atomicOr(A.status, ORBX_ASSEMBLY_STATUS_BAD_KEYFRAME);
    __syncthreads();
    if (tid == 0) W.a0_cnt[r] = s_adm;
}

// exclusive scan of cnt[0 .. n) into off[0 .. n], by one workgroup; returns the total
__device__ int eg_scan(const int32_t* cnt, int32_t* off, int n, int add, int* s_w) {
    int base = add;
    for (int k0 = 0; k0 < n; k0 += kCvThreads) {
        const int k = k0 + threadIdx.x;
        int tot;
        const int pos = cv_block_scan(k < n ? cnt[k] : 0, s_w, tot);
        if (k < n) off[k] = base + pos;
        base += tot;
    }
    if (threadIdx.x == 0) off[n] = base;
    return base;
}

__global__ __launch_bounds__(kCvThreads) void k_eg_scan1(CovisDev D, orbx_essential_graph_assembly A, EgWs W) {
    __shared__ int s_w[kCvWaves];
    const int tid = threadIdx.x;
    const int total = eg_scan(W.lc_cnt, A.lc_off, eg_members(D, A), 0, s_w);
    if (tid == 0 && total > A.max_lc) {
        atomicOr(A.status, ORBX_ASSEMBLY_STATUS_CAPACITY);
        W.misc[1] = 1;
    }
    // the vertices: the keyframes that are not bad, ascending id (cc:913-916)
    int rows = 0;
    for (int k0 = 0; k0 < D.K; k0 += kCvThreads) {
        const int k = k0 + tid;
        const bool good = k < D.nk && !(D.kf_bad && D.kf_bad[k]);
        int tot;
        const int row = rows + cv_block_scan(good, s_w, tot);
        if (k < D.K) A.kf_row[k] = good ? row : -1;
        if (good) {
            A.kf_ids[row] = k;
            A.kf_corr_rows[row] = A.kf_corr[k];
            if (k == A.loop_kf) *A.loop_row = row;
        }
        rows += tot;
    }
    if (tid == 0) {
        *A.n_rows = rows;
        A.kf_off[0] = 0;
        A.kf_off[1] = rows;
        if (D.kf_bad && D.kf_bad[A.loop_kf]) *A.loop_row = -1;
    }
}

// does LoopConnections[a] hold b as an inserted kind-0 edge (cc:984)?
__device__ bool eg_inserted(const CovisDev& D, const orbx_essential_graph_assembly& A, const EgWs& W, int a, int b) {
    const int j = A.kf_corr[a];
    if (j < 0) return false;
    const int r = W.rank_of[j];
    int lo = A.lc_off[r], hi = A.lc_off[r + 1];
    const int end = hi;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (A.lc_kf[mid] < b) lo = mid + 1;
        else hi = mid;
    }
    return lo < end && A.lc_kf[lo] == b && eg_admitted(A, a, b, A.lc_w[lo]) && A.kf_row[a] >= 0 && b < D.nk && A.kf_row[b] >= 0;
}

// an edge between rows v0 and v1 at position at (cc:974-984, 1019-1025)
__device__ __forceinline__ void eg_emit(const orbx_essential_graph_assembly& A, const EgWs& W, int at, int v0, int v1, int kind) {
    if (at < A.max_edges) {
        A.edge_v[2 * (size_t)at] = v0;
        A.edge_v[2 * (size_t)at + 1] = v1;
        A.edge_kind[at] = kind;
    }
    const int a = W.eidx[v0], b = W.eidx[v1];
    if (v0 != v1 && a >= 0 && b >= 0) atomicMin(&W.first[a > b ? a : b], a < b ? a : b);
}

// the kind-1 edges of keyframe mi (cc:989-1089); returns their number
__device__ int eg_keyframe_edges(const CovisDev& D, const orbx_essential_graph_assembly& A, const EgWs& W, int mi, bool write) {
    const int k = A.kf_row[mi];
    int at = write ? W.e_off[k] : 0, n = 0, bad = 0;
    auto edge = [&](int other) {
        const int v1 = other >= 0 && other < D.nk ? A.kf_row[other] : -1;
        if (v1 < 0) {
            bad = 1;
            return;
        }
        if (write) eg_emit(A, W, at + n, k, v1, 1);
        else if (k != v1) W.has[k] = W.has[v1] = 1;
        n++;
    };
    const int par = D.parent[mi];
    if (par >= 0) edge(par);  // cc:1002-1026
    const int l0 = A.loop_off[mi], l1 = A.loop_off[mi + 1];
    for (int l = l0; l < l1; l++)  // cc:1030-1053
        if (A.loop_kf_ids[l] < mi) edge(A.loop_kf_ids[l]);
    const size_t r0 = (size_t)mi * D.max_conn;
    const int m = clampi(D.ord_n[mi], 0, D.max_conn);
    for (int e = 0; e < m && D.ord_w[r0 + e] >= A.min_feat; e++) {  // GetCovisiblesByWeight(minFeat), cc:1057
        const int mn = D.ord_kf[r0 + e];
        if (mn == par || mn >= mi || mn < 0 || A.kf_row[mn] < 0) continue;  // cc:1061-1063
        if (D.parent[mn] == mi) continue;  // hasChild: a good keyframe whose parent is mi
        bool loop = false;
        for (int l = l0; l < l1 && !loop; l++) loop = A.loop_kf_ids[l] == mn;
        if (loop || eg_inserted(D, A, W, mi, mn) || eg_inserted(D, A, W, mn, mi)) continue;  // cc:1061, 1065
        edge(mn);
    }
    if (bad) atomicOr(A.status, ORBX_ASSEMBLY_STATUS_BAD_KEYFRAME);
    return n;
}

__global__ __launch_bounds__(kNdThreads) void k_eg_edges(CovisDev D, orbx_essential_graph_assembly A, EgWs W, int write) {
    if (W.misc[1]) return;  // the LoopConnections did not fit: no edges
    int t = blockIdx.x * kNdThreads + threadIdx.x;
    if (write) {
        if (t <= D.max_conn) {  // the kind-0 edges of LoopConnections row t, in the row's order (cc:954-986)
            if (t >= eg_members(D, A)) return;
            const int mi = A.lc_member[t], a = A.kf_row[mi];
            int at = W.a0_off[t];
            for (int e = A.lc_off[t]; e < A.lc_off[t + 1]; e++) {
                const int mj = A.lc_kf[e];
                const int b = mj < D.nk ? A.kf_row[mj] : -1;
                if (eg_admitted(A, mi, mj, A.lc_w[e]) && a >= 0 && b >= 0) eg_emit(A, W, at++, a, b, 0);
            }
            return;
        }
        t -= D.max_conn + 1;
    }
    if (t >= D.nk || A.kf_row[t] < 0) return;
    const int n = eg_keyframe_edges(D, A, W, t, write != 0);
    if (!write) W.e_cnt[A.kf_row[t]] = n;
}

__global__ __launch_bounds__(kCvThreads) void k_eg_scan2(CovisDev D, orbx_essential_graph_assembly A, EgWs W) {
    __shared__ int s_w[kCvWaves];
    const int tid = threadIdx.x;
    if (W.misc[1]) {
        if (tid == 0) *A.n_edges = A.edge_off[0] = A.edge_off[1] = 0;
        return;
    }
    const int rows = *A.n_rows;
    const int n0 = eg_scan(W.a0_cnt, W.a0_off, eg_members(D, A), 0, s_w);
    const int total = eg_scan(W.e_cnt, W.e_off, rows, n0, s_w);
    if (tid == 0) {
        *A.n_edges = total;
        A.edge_off[0] = 0;
        A.edge_off[1] = total < A.max_edges ? total : A.max_edges;
        if (total > A.max_edges) atomicOr(A.status, ORBX_ASSEMBLY_STATUS_CAPACITY);
    }
    // the envelope's numbering: the rows other than the fixed one that have an edge, in order
    const int fixed = *A.loop_row;
    int F = 0;
    for (int v0 = 0; v0 < rows; v0 += kCvThreads) {
        const int v = v0 + tid;
        const bool in = v < rows && v != fixed && W.has[v];
        int tot;
        const int f = F + cv_block_scan(in, s_w, tot);
        if (v < rows) W.eidx[v] = in ? f : -1;
        if (in) W.first[f] = f;
        F += tot;
    }
    if (tid == 0) W.misc[0] = F;
}

__global__ __launch_bounds__(kNdThreads) void k_eg_finish(CovisDev D, orbx_essential_graph_assembly A, EgWs W) {
    const int t = blockIdx.x * kNdThreads + threadIdx.x;
    if (t < D.nm) {  // cc:1122-1133
        int ref = -1;
        if (!(D.mp_bad && D.mp_bad[t])) ref = A.mp_corrected_by_kf[t] == A.cur_kf ? A.mp_corrected_ref[t] : A.mp_ref_kf[t];
        A.pt_ref[t] = ref >= 0 && ref < D.nk ? A.kf_row[ref] : -1;
    }
    const int row = t / 12, c = t - 12 * row;
    if (row < *A.n_rows) {
        const int id = A.kf_ids[row], j = A.kf_corr[id];
        A.kf_Tcw_rows[(size_t)row * 12 + c] = j >= 0 ? A.kf_Tcw_nc[(size_t)j * 12 + c] : A.kf_Tcw[(size_t)id * 12 + c];
    }
    if (t == 0) {
        A.pt_off[0] = 0;
        A.pt_off[1] = D.nm;
    }
    if (!W.misc[1] && t < W.misc[0]) atomicAdd((unsigned long long*)A.env_blocks, (unsigned long long)(t - W.first[t] + 1));
}

}  // namespace
}  // namespace orbx

extern "C" {

int orbx_update_normal_and_depth_device(orbx_covis* h, const orbx_normal_depth* a, const int32_t* ids, int n_ids, int32_t* status,
                                        void* stream) {
    using namespace orbx;
    if (!h) return fail(ORBX_ERR_ARG, "null graph");
    if (!a) return fail(ORBX_ERR_ARG, "null argument");
    if (n_ids < 0) return fail(ORBX_ERR_ARG, "negative n_ids");
    if (!a->kf_Tcw || !a->kf_keys_un || !a->mp_ref_kf || !a->mp_pos || !a->scale_factors || !a->normal || !a->max_distance ||
        !a->min_distance || !status)
        return fail(ORBX_ERR_ARG, "null table");
    if (a->nlevels < 1 || a->nlevels > kNdMaxLevels) return fail(ORBX_ERR_ARG, "nlevels outside 1..32");
    if (!h->refreshed) return fail(ORBX_ERR_ARG, "no observations: call orbx_covis_refresh_observations_device first");
    hipStream_t s;
    int rc = covis_enter(h, stream, &s);
    if (rc) return rc;
    NdArgs A{};
    A.kf_Tcw = a->kf_Tcw;
    A.kf_keys_un = a->kf_keys_un;
    A.mp_ref_kf = a->mp_ref_kf;
    A.mp_pos = a->mp_pos;
    A.normal = a->normal;
    A.max_distance = a->max_distance;
    A.min_distance = a->min_distance;
    A.ids = ids;
    A.n = ids ? n_ids : h->D.nm;
    A.nlevels = a->nlevels;
    A.status = status;
    for (int l = 0; l < a->nlevels; l++) A.scale[l] = a->scale_factors[l];
    HIP_TRY(hipMemsetAsync(status, 0, 4, s));
    if (A.n > 0) {
        k_normal_depth<<<(A.n + kNdThreads - 1) / kNdThreads, kNdThreads, 0, s>>>(h->D, A);
        HIP_TRY(hipGetLastError());
    }
    return ORBX_OK;
}

int orbx_correct_loop_propagate_device(orbx_covis* h, const orbx_correct_loop_propagate* a, void* stream) {
    using namespace orbx;
    if (!h) return fail(ORBX_ERR_ARG, "null graph");
    if (!a) return fail(ORBX_ERR_ARG, "null argument");
    if (!a->kf_Tcw || !a->mp_pos || !a->mp_corrected_by_kf || !a->mp_corrected_ref || !a->mp_ref_kf || !a->kf_keys_un ||
        !a->scale_factors || !a->normal || !a->max_distance || !a->min_distance)
        return fail(ORBX_ERR_ARG, "null map table");
    if (!a->conn || !a->n_conn || !a->corr_S || !a->kf_corr || !a->kf_Tcw_nc || !a->status) return fail(ORBX_ERR_ARG, "null result array");
    if (!a->Scw && (!a->sim3_R || !a->sim3_t || !a->sim3_s)) return fail(ORBX_ERR_ARG, "neither Scw nor sim3_R / sim3_t / sim3_s");
    if (a->nlevels < 1 || a->nlevels > kNdMaxLevels) return fail(ORBX_ERR_ARG, "nlevels outside 1..32");
    if (!h->refreshed) return fail(ORBX_ERR_ARG, "no observations: call orbx_covis_refresh_observations_device first");
    const CovisDev& D = h->D;
    if (a->cur_kf < 0 || a->cur_kf >= D.nk || (!a->Scw && (a->matched_kf < 0 || a->matched_kf >= D.nk)))
        return fail(ORBX_ERR_ARG, "keyframe id outside the graph");
    const int32_t cur = a->cur_kf;
    int rc = orbx_covis_update_connections_device(h, &cur, 1, stream);  // cc:482
    if (rc) return rc;
    hipStream_t s;
    if ((rc = covis_enter(h, stream, &s))) return rc;
    const int slots = D.max_conn + 1;
    if (!h->cl_pose_ws) {
        HIP_TRY(hipMalloc((void**)&h->cl_pose_ws, (size_t)slots * 12 * 4));
        h->allocs.push_back(h->cl_pose_ws);
    }
    ClArgs A{};
    A.cur = cur;
    A.matched = a->Scw ? -1 : a->matched_kf;
    A.Scw = a->Scw;
    A.sim3_R = a->sim3_R;
    A.sim3_t = a->sim3_t;
    A.sim3_s = a->sim3_s;
    A.kf_Tcw = a->kf_Tcw;
    A.mp_pos = a->mp_pos;
    A.by_kf = a->mp_corrected_by_kf;
    A.corr_ref = a->mp_corrected_ref;
    A.conn = a->conn;
    A.n_conn = a->n_conn;
    A.corr_S = a->corr_S;
    A.kf_corr = a->kf_corr;
    A.kf_Tcw_nc = a->kf_Tcw_nc;
    A.Tc = h->cl_pose_ws;
    A.nd.kf_Tcw = a->kf_Tcw;
    A.nd.kf_keys_un = a->kf_keys_un;
    A.nd.mp_ref_kf = a->mp_ref_kf;
    A.nd.mp_pos = a->mp_pos;
    A.nd.normal = a->normal;
    A.nd.max_distance = a->max_distance;
    A.nd.min_distance = a->min_distance;
    A.nd.nlevels = a->nlevels;
    A.nd.status = a->status;
    for (int l = 0; l < a->nlevels; l++) A.nd.scale[l] = a->scale_factors[l];
    HIP_TRY(hipMemsetAsync(a->status, 0, 4, s));
    HIP_TRY(hipMemsetAsync(a->kf_corr, 0xFF, (size_t)D.K * 4, s));
    k_cl_members<<<1, kCvThreads, 0, s>>>(D, A);
    HIP_TRY(hipGetLastError());
    const long long threads = (long long)slots * D.cap;
    k_cl_points<<<(int)((threads + kNdThreads - 1) / kNdThreads), kNdThreads, 0, s>>>(D, A);
    HIP_TRY(hipGetLastError());
    k_cl_poses<<<(slots * 12 + 255) / 256, 256, 0, s>>>(A);  // behind the points, which read the input poses
    HIP_TRY(hipGetLastError());
    return covis_update_ids_device(h, a->conn, a->n_conn, slots, s);  // cc:570
}

int orbx_essential_graph_assemble_device(orbx_covis* h, const orbx_essential_graph_assembly* a, void* stream) {
    using namespace orbx;
    if (!h) return fail(ORBX_ERR_ARG, "null graph");
    if (!a) return fail(ORBX_ERR_ARG, "null argument");
    if (a->max_lc < 0 || a->max_edges < 0) return fail(ORBX_ERR_ARG, "negative capacity");
    if (!a->conn || !a->n_conn || !a->kf_corr || !a->kf_Tcw_nc || !a->kf_Tcw || !a->loop_off || !a->mp_corrected_by_kf ||
        !a->mp_corrected_ref || !a->mp_ref_kf)
        return fail(ORBX_ERR_ARG, "null input table");
    if (!a->lc_off || !a->lc_member || (a->max_lc > 0 && (!a->lc_kf || !a->lc_w)) || !a->kf_ids || !a->kf_row || !a->n_rows ||
        !a->kf_off || !a->loop_row || !a->kf_corr_rows || !a->kf_Tcw_rows || (a->max_edges > 0 && (!a->edge_v || !a->edge_kind)) ||
        !a->n_edges || !a->edge_off || !a->pt_ref || !a->pt_off || !a->env_blocks || !a->status)
        return fail(ORBX_ERR_ARG, "null result array");
    if (!h->refreshed) return fail(ORBX_ERR_ARG, "no observations: call orbx_covis_refresh_observations_device first");
    const CovisDev& D = h->D;
    if (a->cur_kf < 0 || a->cur_kf >= D.nk || a->loop_kf < 0 || a->loop_kf >= D.nk) return fail(ORBX_ERR_ARG, "keyframe id outside the graph");
    hipStream_t s;
    int rc = covis_enter(h, stream, &s);
    if (rc) return rc;
    const size_t slots = (size_t)D.max_conn + 1, K = (size_t)D.K;
    const size_t zeroed = K + 2;  // has, misc
    const size_t words = zeroed + 3 * slots * D.max_conn + 6 * slots + (slots + 1) + 2 * K + (K + 1) + K;
    if (!h->eg_ws) {
        HIP_TRY(hipMalloc((void**)&h->eg_ws, words * 4));
        h->allocs.push_back(h->eg_ws);
    }
    EgWs W{};
    int32_t* p = h->eg_ws;
    W.has = p, p += K;
    W.misc = p, p += 2;
    W.prev = p, p += slots * D.max_conn;
    W.prev_n = p, p += slots;
    W.prow_kf = p, p += slots * D.max_conn;
    W.prow_w = p, p += slots * D.max_conn;
    W.prow_n = p, p += slots;
    W.srt = p, p += slots;
    W.rank_of = p, p += slots;
    W.lc_cnt = p, p += slots;
    W.a0_cnt = p, p += slots;
    W.a0_off = p, p += slots + 1;
    W.e_cnt = p, p += K;
    W.e_off = p, p += K + 1;
    W.eidx = p, p += K;
    W.first = p;
    HIP_TRY(hipMemsetAsync(h->eg_ws, 0, zeroed * 4, s));
    HIP_TRY(hipMemsetAsync(a->status, 0, 4, s));
    HIP_TRY(hipMemsetAsync(a->env_blocks, 0, 8, s));
    k_eg_snapshot<<<(int)slots, kNdThreads, 0, s>>>(D, *a, W);
    HIP_TRY(hipGetLastError());
    if ((rc = covis_update_ids_device(h, a->conn, a->n_conn, (int)slots, s))) return rc;  // cc:601
    k_eg_lc<<<(int)slots, kCvThreads, 0, s>>>(D, *a, W, 0);
    HIP_TRY(hipGetLastError());
    k_eg_scan1<<<1, kCvThreads, 0, s>>>(D, *a, W);
    HIP_TRY(hipGetLastError());
    k_eg_lc<<<(int)slots, kCvThreads, 0, s>>>(D, *a, W, 1);
    HIP_TRY(hipGetLastError());
    if (D.nk > 0) {
        k_eg_edges<<<(D.nk + kNdThreads - 1) / kNdThreads, kNdThreads, 0, s>>>(D, *a, W, 0);
        HIP_TRY(hipGetLastError());
    }
    k_eg_scan2<<<1, kCvThreads, 0, s>>>(D, *a, W);
    HIP_TRY(hipGetLastError());
    k_eg_edges<<<(int)((slots + D.nk + kNdThreads - 1) / kNdThreads), kNdThreads, 0, s>>>(D, *a, W, 1);
    HIP_TRY(hipGetLastError());
    const long long most = std::max<long long>(std::max<long long>(D.nm, (long long)D.nk * 12), 1);
    k_eg_finish<<<(int)((most + kNdThreads - 1) / kNdThreads), kNdThreads, 0, s>>>(D, *a, W);
    HIP_TRY(hipGetLastError());
    return ORBX_OK;
}

}  // extern "C"
