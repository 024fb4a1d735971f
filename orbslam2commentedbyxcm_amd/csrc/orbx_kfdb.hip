// orbx_kfdb.hip -- device-resident KeyFrameDatabase: DBoW2's L1 score and the candidate
// detection of relocalisation and loop closing.
//
// Reference: src/KeyFrameDatabase.cc:31-307 (add / erase / clear, DetectLoopCandidates
// 79-195, DetectRelocalizationCandidates 206-307) and Thirdparty/DBoW2/DBoW2/
// ScoringObject.cpp:23-68 (L1Scoring::score).  DESIGN.md §4.14.
//
// The reference walks an inverted file of std::lists; here every stored keyframe's sorted
// BowVector lies in an HBM slab and a query is intersected with all of them at once (waves
// over the (query, keyframe) pairs, the query's words in LDS).  The reference's list order --
// first encounter while walking the query's words upwards, each word's list in add() order
// -- is the order key (smallest shared word, add rank), sorted by one workgroup per query.
//
// fp64 sums are order-sensitive: the L1 terms of one pair are computed 64 at a time and then
// added one by one, in ascending word order, from 0.0 -- no tree or wave reduction.  The
// float group sums (accScore) follow the covisibility list's order in one thread.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "orbx.h"
#include "orbx_block_sort.h"
#include "orbx_host.h"

namespace orbx {

int vocabulary_device(const orbx_vocabulary* v);  // orbx_vocab.hip

constexpr int kKfdbMaxKeyframes = ORBX_KFDB_MAX_KEYFRAMES;  // one workgroup sorts a query's candidates
constexpr int kKfdbMaxCap = 8192;                           // BowVector entries per keyframe / query
constexpr int kKfdbCovis = ORBX_KFDB_COVIS;
constexpr int kPairThreads = 1024;                          // 16 waves = 16 keyframes per workgroup
constexpr int kPairWaves = kPairThreads / 64;
constexpr int kFlagScored = 1, kFlagListed = 2;
constexpr int kShareBitmapBits = 1 << 18;                   // k_kfdb_share's filter: 32 KB of LDS
constexpr int kShareKfPerWave = 4;                          // keyframes per wave: 64 per workgroup
constexpr int kShareUnroll = 4;                             // 64-word chunks in flight per wave
constexpr size_t groups_lds(int np) { return (size_t)np * 12 + kSortThreads * 4 + 128; }

struct KfdbDev {
    const int32_t* words;   // [max_kf][cap] ascending
    const double* values;   // [max_kf][cap]
    const int32_t* count;   // [max_kf]
    const int32_t* alive;   // [max_kf]
    const int32_t* rank;    // [max_kf] position in add order among the live keyframes
    const int32_t* order;   // [max_kf] rank -> id
    const int32_t* covis;   // [max_kf][10] GetBestCovisibilityKeyFrames(10), -1 = no entry
    float* reloc;           // [max_kf] mRelocScore
    int max_kf, cap;
};

// first position p in the ascending s[0, n) with s[p] >= w
__device__ __forceinline__ int lower_bound_i32(const int32_t* s, int n, int32_t w) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s[mid] < w)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// L1Scoring::score(v1 = query, v2 = keyframe), ScoringObject.cpp:23-68, by one wave: the
// keyframe's words 64 at a time, each lane looking its word up in the query and forming the
// term; the terms are then added in lane order (= ascending word order), one at a time.
// Every lane returns the same value.
__device__ double wave_l1_score(const int32_t* qw, const double* qv, int qn, const int32_t* kw, const double* kv,
                                int kn) {
    const int lane = threadIdx.x & 63;
    double score = 0.0;
    for (int base = 0; base < kn; base += 64) {
        const int i = base + lane;
        double term = 0.0;
        bool hit = false;
        if (i < kn) {
            const int32_t w = kw[i];
            const int p = lower_bound_i32(qw, qn, w);
            if (p < qn && qw[p] == w) {
                const double vi = qv[p], wi = kv[i];
                term = fabs(vi - wi) - fabs(vi) - fabs(wi);  // cpp:41
                hit = true;
            }
        }
        unsigned long long m = __ballot(hit);
        while (m) {
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1;
            score += __shfl(term, l, 64);
        }
    }
    return -score / 2.0;  // cpp:65; no shared word: -0.0
}

__device__ __forceinline__ void load_query_words(int32_t* s_q, const int32_t* qword, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) s_q[i] = qword[i];
    __syncthreads();
}

// Sharing stage (KeyFrameDatabase.cc:88-106, 213-228) for query blockIdx.y and, per wave,
// kShareKfPerWave consecutive keyframes: the number of shared words (0 for a dead, empty or connected
// keyframe) and the smallest shared word; the query's maximum goes to maxwords[b].  Beside
// the query's sorted words the workgroup keeps a 2^18-bit map of them (word mod 2^18) in
// LDS: a keyframe word whose bit is clear is not shared (one LDS read); only the others,
// the shared ones and ~0.4 % false hits at 1000 query words, take the binary search.
__global__ __launch_bounds__(kPairThreads) void k_kfdb_share(KfdbDev D, const int32_t* qword, const int32_t* qn,
                                                             int qcap, const int32_t* conn, int32_t* words,
                                                             int32_t* minword, int32_t* maxwords) {
    extern __shared__ int32_t s_q[];
    uint32_t* s_bits = (uint32_t*)(s_q + qcap);
    const int b = blockIdx.y;
    const int n = clampi(qn[b], 0, qcap);
    for (int i = threadIdx.x; i < kShareBitmapBits / 32; i += blockDim.x) s_bits[i] = 0;
    load_query_words(s_q, qword + (size_t)b * qcap, n);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const unsigned h = (unsigned)s_q[i] & (kShareBitmapBits - 1);
        atomicOr(&s_bits[h >> 5], 1u << (h & 31));
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    int local_max = 0;
    for (int r = 0; r < kShareKfPerWave; r++) {
        const int kf = (blockIdx.x * kPairWaves + (threadIdx.x >> 6)) * kShareKfPerWave + r;
        if (kf >= D.max_kf) break;
        const size_t o = (size_t)b * D.max_kf + kf;
        int cnt = 0, mw = -1;
        if (n > 0 && D.alive[kf] && !(conn && conn[o])) {
            const int kn = clampi(D.count[kf], 0, D.cap);
            const int32_t* kw = D.words + (size_t)kf * D.cap;
            // four 64-word chunks per round: their loads and bitmap reads are in flight together
            for (int base = 0; base < kn; base += 64 * kShareUnroll) {
                int32_t w[kShareUnroll];
                bool maybe[kShareUnroll];
#pragma unroll
                for (int u = 0; u < kShareUnroll; u++) {
                    const int i = base + u * 64 + lane;
                    w[u] = i < kn ? kw[i] : -1;
                }
#pragma unroll
                for (int u = 0; u < kShareUnroll; u++) {
                    const unsigned h = (unsigned)w[u] & (kShareBitmapBits - 1);
                    maybe[u] = base + u * 64 + lane < kn && ((s_bits[h >> 5] >> (h & 31)) & 1u);
                }
#pragma unroll
                for (int u = 0; u < kShareUnroll; u++) {  // ascending words: the first hit is the smallest
                    bool hit = false;
                    if (maybe[u]) {  // most words of most keyframes stop at the bitmap
                        const int p = lower_bound_i32(s_q, n, w[u]);
                        hit = p < n && s_q[p] == w[u];
                    }
                    const unsigned long long m = __ballot(hit);
                    if (m) {
                        if (cnt == 0) mw = __shfl(w[u], __ffsll((long long)m) - 1, 64);
                        cnt += __popcll(m);
                    }
                }
            }
        }
        if (lane == 0) {
            words[o] = cnt;
            minword[o] = mw;
        }
        if (cnt > local_max) local_max = cnt;
    }
    if (lane == 0 && local_max > 0) atomicMax(&maxwords[b], local_max);
}

// Threshold and scoring (cc:122-138, 240-255): pairs with words > minCommonWords get
// float si = score(query, keyframe); loop form: listed only if si >= minScore.
__global__ __launch_bounds__(kPairThreads) void k_kfdb_score(KfdbDev D, const int32_t* qword, const double* qvalue,
                                                             const int32_t* qn, int qcap, const int32_t* words,
                                                             const int32_t* maxwords, const float* min_score,
                                                             float* score, int32_t* flags) {
    extern __shared__ int32_t s_q[];
    const int b = blockIdx.y;
    const int n = clampi(qn[b], 0, qcap);
    load_query_words(s_q, qword + (size_t)b * qcap, n);
    const int kf = blockIdx.x * kPairWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (kf >= D.max_kf) return;
    const size_t o = (size_t)b * D.max_kf + kf;
    const int min_common = (int)((float)maxwords[b] * 0.8f);  // cc:122, 240
    float si = -1.0f;
    int fl = 0;
    if (words[o] > min_common) {
        const int kn = clampi(D.count[kf], 0, D.cap);
        si = (float)wave_l1_score(s_q, qvalue + (size_t)b * qcap, n, D.words + (size_t)kf * D.cap,
                                  D.values + (size_t)kf * D.cap, kn);
        fl = kFlagScored | ((!min_score || si >= min_score[b]) ? kFlagListed : 0);
    }
    if (lane == 0) {
        score[o] = si;
        flags[o] = fl;
    }
}

// Relocalisation only: mRelocScore persists between queries (cc:252, 277).  One thread per
// keyframe walks the batch in query order: eff[b][kf] is the score as query b sees it.
__global__ void k_kfdb_resolve(KfdbDev D, int batch, const float* score, const int32_t* flags, float* eff) {
    const int kf = blockIdx.x * blockDim.x + threadIdx.x;
    if (kf >= D.max_kf) return;
    float cur = D.reloc[kf];
    for (int b = 0; b < batch; b++) {
        const size_t o = (size_t)b * D.max_kf + kf;
        if (flags[o] & kFlagScored) cur = score[o];
        eff[o] = cur;
    }
    D.reloc[kf] = cur;
}

// spConnectedKeyFrames as a mask: conn[b][id] = 1 for the ids of query b's CSR row.
__global__ void k_kfdb_connected(int max_kf, const int32_t* conn_off, const int32_t* conn_ids, int32_t* conn) {
    const int b = blockIdx.x;
    const int lo = conn_off[b], hi = conn_off[b + 1];
    for (int i = lo + (int)threadIdx.x; i < hi; i += blockDim.x) {
        const int id = conn_ids[i];
        if (id >= 0 && id < max_kf) conn[(size_t)b * max_kf + id] = 1;
    }
}

// Groups, selection and the ordered compaction (cc:149-194, 265-306), one workgroup per
// query.  LDS (groups_lds): np sort keys, np first-position slots, 1024 scan words, 16 + 1
// reduction words.
__global__ __launch_bounds__(kSortThreads) void k_kfdb_groups(KfdbDev D, int np, int loop, const int32_t* words,
                                                              const int32_t* minword, const int32_t* maxwords,
                                                              const float* eff, const int32_t* flags,
                                                              const float* min_score, int32_t* cand, int max_cand,
                                                              int32_t* ncand) {
    // everything in the dynamic region: a static array in front of it would move s_key
    // off its 8-byte alignment
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_mem[];
    unsigned long long* s_key = s_mem;
    int* s_first = (int*)(s_key + np);
    int* s_scan = s_first + np;
    float* s_red = (float*)(s_scan + kSortThreads);
    int& s_nlist = *(int*)(s_red + kSortThreads / 64);
    const int b = blockIdx.x, t = threadIdx.x, ne = np / kSortThreads;
    const size_t row = (size_t)b * D.max_kf;
    if (t == 0) s_nlist = 0;
    __syncthreads();
    // lScoreAndMatch in list order: sort the listed keyframes by (smallest shared word, add rank)
    unsigned long long r[kSortPer];
    int mine = 0;
#pragma unroll
    for (int e = 0; e < kSortPer; e++) {
        r[e] = ~0ull;
        const int kf = e * kSortThreads + t;
        if (e < ne && kf < D.max_kf && (flags[row + kf] & kFlagListed)) {
            r[e] = (unsigned long long)(unsigned)minword[row + kf] << 32 | (unsigned)D.rank[kf];
            mine++;
        }
    }
    if (mine) atomicAdd(&s_nlist, mine);
    block_bitonic_sort64(r, ne, s_key);
    const int nlist = s_nlist;
    const int min_common = (int)((float)maxwords[b] * 0.8f);
    float best_acc = loop ? min_score[b] : 0.0f;  // cc:145, 261
    for (int e = 0; e < ne; e++) {
        const int i = t * ne + e;
        if (i >= nlist) break;
        const int kf = D.order[clampi((int)(unsigned)s_key[i], 0, D.max_kf - 1)];
        float best_score = eff[row + kf], acc = best_score;
        int best_kf = kf;
        for (int j = 0; j < kKfdbCovis; j++) {
            const int k2 = D.covis[kf * kKfdbCovis + j];
            if (k2 < 0 || k2 >= D.max_kf || !D.alive[k2]) continue;
            // candidate of this query (cc:275-276); loop form: and over the threshold (cc:161)
            if (words[row + k2] <= (loop ? min_common : 0)) continue;
            const float s2 = eff[row + k2];
            acc += s2;
            if (s2 > best_score) {
                best_kf = k2;
                best_score = s2;
            }
        }
        s_key[i] = (unsigned long long)__float_as_uint(acc) << 32 | (unsigned)best_kf;
        if (acc > best_acc) best_acc = acc;
    }
    for (int i = t; i < np; i += kSortThreads) s_first[i] = INT_MAX;
    // bestAccScore: a maximum, so the order of the comparisons does not matter
    for (int j = 32; j > 0; j >>= 1) {
        const float o = __shfl_xor(best_acc, j, 64);
        if (o > best_acc) best_acc = o;
    }
    if ((t & 63) == 0) s_red[t >> 6] = best_acc;
    __syncthreads();
    for (int w = 0; w < kSortThreads / 64; w++)
        if (s_red[w] > best_acc) best_acc = s_red[w];
    const float retain = 0.75f * best_acc;  // cc:176, 289
    for (int e = 0; e < ne; e++) {
        const int i = t * ne + e;
        if (i >= nlist) break;
        const unsigned long long v = s_key[i];
        if (__uint_as_float((unsigned)(v >> 32)) > retain) atomicMin(&s_first[(unsigned)v], i);
    }
    __syncthreads();
    // spAlreadyAddedKF: a group's best keyframe is emitted at its first retained position
    int cnt = 0;
    for (int e = 0; e < ne; e++) {
        const int i = t * ne + e;
        if (i >= nlist) break;
        const unsigned long long v = s_key[i];
        if (__uint_as_float((unsigned)(v >> 32)) > retain && s_first[(unsigned)v] == i) cnt++;
    }
    s_scan[t] = cnt;
    __syncthreads();
    for (int d = 1; d < kSortThreads; d <<= 1) {
        const int add = t >= d ? s_scan[t - d] : 0;
        __syncthreads();
        s_scan[t] += add;
        __syncthreads();
    }
    int pos = s_scan[t] - cnt;
    for (int e = 0; e < ne; e++) {
        const int i = t * ne + e;
        if (i >= nlist) break;
        const unsigned long long v = s_key[i];
        if (__uint_as_float((unsigned)(v >> 32)) > retain && s_first[(unsigned)v] == i) {
            if (pos < max_cand) cand[(size_t)b * max_cand + pos] = (int32_t)(unsigned)v;
            pos++;
        }
    }
    if (t == kSortThreads - 1) ncand[b] = s_scan[t];
}

// orbx_kfdb_score_device: one wave per listed id; an id that is not stored gives NaN.
__global__ __launch_bounds__(kPairThreads) void k_kfdb_score_ids(KfdbDev D, const int32_t* qword,
                                                                 const double* qvalue, const int32_t* qn, int qcap,
                                                                 const int32_t* ids, int nids, float* out) {
    extern __shared__ int32_t s_q[];
    const int n = clampi(qn[0], 0, qcap);
    load_query_words(s_q, qword, n);
    const int k = blockIdx.x * kPairWaves + (threadIdx.x >> 6);
    if (k >= nids) return;
    const int kf = ids[k];
    float si = __uint_as_float(0x7fc00000u);
    if (kf >= 0 && kf < D.max_kf && D.alive[kf]) {
        const int kn = clampi(D.count[kf], 0, D.cap);
        si = (float)wave_l1_score(s_q, qvalue, n, D.words + (size_t)kf * D.cap, D.values + (size_t)kf * D.cap, kn);
    }
    if ((threadIdx.x & 63) == 0) out[k] = si;
}

// add(): keyframe ids[i] <- BowVector i of the transform layout; mRelocScore pinned to 0.
__global__ void k_kfdb_add(int32_t* words, double* values, int32_t* count, float* reloc, int max_kf, int cap,
                           const int32_t* ids, const int32_t* src_word, const double* src_value,
                           const int32_t* src_n, int src_cap) {
    const int i = blockIdx.x;
    const int id = ids[i];
    if (id < 0 || id >= max_kf) return;
    const int n = clampi(src_n[i], 0, cap < src_cap ? cap : src_cap);
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        words[(size_t)id * cap + j] = src_word[(size_t)i * src_cap + j];
        values[(size_t)id * cap + j] = src_value[(size_t)i * src_cap + j];
    }
    if (threadIdx.x == 0) {
        count[id] = n;
        reloc[id] = 0.0f;
    }
}

}  // namespace orbx

// ---------------------------------------------------------------------------------------
// Host side

struct orbx_kfdb {
    int device = 0, nwords = 0, max_kf = 0, cap = 0;
    hipStream_t stream = nullptr, last = nullptr;
    int32_t* words = nullptr;
    double* values = nullptr;
    int32_t* count = nullptr;
    float* reloc = nullptr;
    int32_t* meta = nullptr;  // alive, rank, order [max_kf] each, covis [max_kf][10]
    orbx::DeviceBuffer work;
    orbx::DeviceBuffer stage;      // host-form staging
    orbx::DeviceBuffer stage_add;  // orbx_kfdb_add's BowVector
    // membership lives on the host (ids are the caller's) and is uploaded before use
    std::vector<int32_t> h_meta;
    std::vector<long long> seq;
    long long next_seq = 0;
    int live = 0;
    bool dirty = true;
};

namespace {

using namespace orbx;

int32_t* h_alive(orbx_kfdb* d) { return d->h_meta.data(); }
int32_t* h_rank(orbx_kfdb* d) { return d->h_meta.data() + d->max_kf; }
int32_t* h_order(orbx_kfdb* d) { return d->h_meta.data() + 2 * (size_t)d->max_kf; }
int32_t* h_covis(orbx_kfdb* d) { return d->h_meta.data() + 3 * (size_t)d->max_kf; }

KfdbDev view(orbx_kfdb* d) {
    return KfdbDev{d->words, d->values, d->count, d->meta, d->meta + d->max_kf, d->meta + 2 * (size_t)d->max_kf,
                   d->meta + 3 * (size_t)d->max_kf, d->reloc, d->max_kf, d->cap};
}

void free_db(orbx_kfdb* d) {
    void* ptrs[] = {d->words, d->values, d->count, d->reloc, d->meta};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    for (DeviceBuffer* b : {&d->work, &d->stage, &d->stage_add}) b->release();
    if (d->stream) (void)hipStreamDestroy(d->stream);
}

// One database, one stream at a time: a call on another stream first waits for the last one.
int enter(orbx_kfdb* d, void* stream, hipStream_t* s) {
    HIP_TRY(hipSetDevice(d->device));
    *s = stream ? (hipStream_t)stream : d->stream;
    if (d->last && d->last != *s) HIP_TRY(hipStreamSynchronize(d->last));
    d->last = *s;
    return ORBX_OK;
}

// The add order of the live keyframes as ranks (erase keeps the others' relative order, a
// keyframe added again goes to the end), then alive / rank / order / covisibility to HBM.
int flush_meta(orbx_kfdb* d, hipStream_t s) {
    if (!d->dirty) return ORBX_OK;
    std::vector<std::pair<long long, int>> by_seq;
    by_seq.reserve((size_t)d->live);
    for (int id = 0; id < d->max_kf; id++) {
        h_rank(d)[id] = 0;
        h_order(d)[id] = 0;
        if (h_alive(d)[id]) by_seq.emplace_back(d->seq[id], id);
    }
    std::sort(by_seq.begin(), by_seq.end());
    for (size_t r = 0; r < by_seq.size(); r++) {
        h_rank(d)[by_seq[r].second] = (int32_t)r;
        h_order(d)[r] = by_seq[r].second;
    }
    // pageable source: staged by the runtime before the call returns
    HIP_TRY(hipMemcpyAsync(d->meta, d->h_meta.data(), d->h_meta.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    d->dirty = false;
    return ORBX_OK;
}

int next_pow2(int x) {
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

int detect(orbx_kfdb* d, int loop, int batch, const int32_t* d_qword, const double* d_qvalue, const int32_t* d_qn,
           int qcap, const int32_t* d_conn_off, const int32_t* d_conn_ids, const float* d_min_score, int32_t* d_cand,
           int max_cand, int32_t* d_ncand, int32_t* d_words, float* d_score, void* stream) {
    if (!d || batch < 0 || qcap < 0 || max_cand < 0) return fail(ORBX_ERR_ARG, "bad argument");
    if (batch == 0) return ORBX_OK;
    if (!d_qword || !d_qvalue || !d_qn || !d_ncand || (max_cand && !d_cand))
        return fail(ORBX_ERR_ARG, "null argument");
    if (loop && (!d_conn_off || !d_min_score)) return fail(ORBX_ERR_ARG, "null connected set or min_score");
    if (qcap > kKfdbMaxCap) return fail(ORBX_ERR_UNSUPPORTED, "more than 8192 words per query");
    if (batch > 65535) return fail(ORBX_ERR_UNSUPPORTED, "more than 65535 queries per call");
    hipStream_t s;
    int rc = enter(d, stream, &s);
    if (rc) return rc;
    rc = flush_meta(d, s);
    if (rc) return rc;
    const size_t cells = (size_t)batch * d->max_kf, b_c = up256(cells * 4);
    HIP_TRY(d->work.reserve(6 * b_c + up256((size_t)batch * 4), s));
    char* w = d->work.p;
    int32_t* words = d_words ? d_words : (int32_t*)w;
    int32_t* minword = (int32_t*)(w + b_c);
    float* score = d_score ? d_score : (float*)(w + 2 * b_c);
    float* eff = (float*)(w + 3 * b_c);
    int32_t* flags = (int32_t*)(w + 4 * b_c);
    int32_t* conn = (int32_t*)(w + 5 * b_c);
    int32_t* maxwords = (int32_t*)(w + 6 * b_c);
    const KfdbDev D = view(d);
    HIP_TRY(hipMemsetAsync(maxwords, 0, (size_t)batch * 4, s));
    if (loop) {
        HIP_TRY(hipMemsetAsync(conn, 0, cells * 4, s));
        if (d_conn_ids) {
            k_kfdb_connected<<<batch, 256, 0, s>>>(d->max_kf, d_conn_off, d_conn_ids, conn);
            HIP_TRY(hipGetLastError());
        }
    }
    const dim3 grid((d->max_kf + kPairWaves - 1) / kPairWaves, batch);
    const size_t qlds = (size_t)(qcap > 0 ? qcap : 1) * 4;
    static thread_local bool share_attr = false;
    if (!share_attr) {
        HIP_TRY(hipFuncSetAttribute((const void*)k_kfdb_share, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    kKfdbMaxCap * 4 + kShareBitmapBits / 8));
        share_attr = true;
    }
    const int per_group = kPairWaves * kShareKfPerWave;
    const dim3 grid_share((d->max_kf + per_group - 1) / per_group, batch);
    k_kfdb_share<<<grid_share, kPairThreads, qlds + kShareBitmapBits / 8, s>>>(D, d_qword, d_qn, qcap, loop ? conn : nullptr, words, minword,
                                                  maxwords);
    HIP_TRY(hipGetLastError());
    k_kfdb_score<<<grid, kPairThreads, qlds, s>>>(D, d_qword, d_qvalue, d_qn, qcap, words, maxwords,
                                                  loop ? d_min_score : nullptr, score, flags);
    HIP_TRY(hipGetLastError());
    if (!loop) {
        k_kfdb_resolve<<<(d->max_kf + 255) / 256, 256, 0, s>>>(D, batch, score, flags, eff);
        HIP_TRY(hipGetLastError());
    }
    const int np = next_pow2(d->max_kf < kSortThreads ? kSortThreads : d->max_kf);
    static thread_local bool attr = false;
    if (!attr) {
        HIP_TRY(hipFuncSetAttribute((const void*)k_kfdb_groups, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)groups_lds(kKfdbMaxKeyframes)));
        attr = true;
    }
    k_kfdb_groups<<<batch, kSortThreads, groups_lds(np), s>>>(
        D, np, loop, words, minword, maxwords, loop ? score : eff, flags, d_min_score, d_cand, max_cand, d_ncand);
    HIP_TRY(hipGetLastError());
    return ORBX_OK;
}

// The host-pointer single-query forms: stage, run the device form, copy back.
int detect_host(orbx_kfdb* d, int loop, const int32_t* word, const double* value, int n, const int32_t* connected,
                int nconnected, float min_score, int32_t* cand, int max_cand, int* ncand) {
    if (!d || n < 0 || nconnected < 0 || max_cand < 0 || !ncand || (n && (!word || !value)) ||
        (nconnected && !connected) || (max_cand && !cand))
        return fail(ORBX_ERR_ARG, "bad argument");
    if (n > kKfdbMaxCap) return fail(ORBX_ERR_UNSUPPORTED, "more than 8192 words per query");
    *ncand = 0;
    hipStream_t s;
    int rc = enter(d, nullptr, &s);
    if (rc) return rc;
    const int qcap = n > 0 ? n : 1;
    const size_t b_w = up256((size_t)qcap * 4), b_v = up256((size_t)qcap * 8),
                 b_conn = up256((size_t)(nconnected > 0 ? nconnected : 1) * 4),
                 b_cand = up256((size_t)(max_cand > 0 ? max_cand : 1) * 4);
    HIP_TRY(d->stage.reserve(b_w + b_v + b_conn + b_cand + 256, s));
    char* p = d->stage.p;
    int32_t* d_w = (int32_t*)p;
    double* d_v = (double*)(p + b_w);
    int32_t* d_conn = (int32_t*)(p + b_w + b_v);
    int32_t* d_cand = (int32_t*)(p + b_w + b_v + b_conn);
    int32_t* d_small = (int32_t*)(p + b_w + b_v + b_conn + b_cand);  // [0] n, [1..2] conn_off, [3] min_score, [4] ncand
    int32_t small[5] = {n, 0, nconnected, 0, 0};
    std::memcpy(&small[3], &min_score, 4);
    if (n) {
        HIP_TRY(hipMemcpyAsync(d_w, word, (size_t)n * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_v, value, (size_t)n * 8, hipMemcpyHostToDevice, s));
    }
    if (nconnected) HIP_TRY(hipMemcpyAsync(d_conn, connected, (size_t)nconnected * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_small, small, sizeof(small), hipMemcpyHostToDevice, s));
    rc = detect(d, loop, 1, d_w, d_v, d_small, qcap, d_small + 1, d_conn, (const float*)(d_small + 3), d_cand,
                max_cand, d_small + 4, nullptr, nullptr, nullptr);
    if (rc) return rc;
    int32_t got = 0;
    HIP_TRY(hipMemcpyAsync(&got, d_small + 4, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *ncand = got;
    const int m = got < max_cand ? got : max_cand;
    if (m > 0) {
        HIP_TRY(hipMemcpyAsync(cand, d_cand, (size_t)m * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (got > max_cand) return fail(ORBX_ERR_CAPACITY, "more candidates than max_cand (*ncand holds the count)");
    return ORBX_OK;
}

}  // namespace

extern "C" {

int orbx_bow_score(const int32_t* w1, const double* v1, int n1, const int32_t* w2, const double* v2, int n2,
                   double* score) {
    if (!score || n1 < 0 || n2 < 0 || (n1 && (!w1 || !v1)) || (n2 && (!w2 || !v2)))
        return fail(ORBX_ERR_ARG, "bad argument");
    double sum = 0.0;
    int i = 0, j = 0;
    while (i < n1 && j < n2) {  // ScoringObject.cpp:34-59
        if (w1[i] == w2[j]) {
            const double vi = v1[i], wi = v2[j];
            sum += std::fabs(vi - wi) - std::fabs(vi) - std::fabs(wi);
            i++;
            j++;
        } else if (w1[i] < w2[j]) {
            i++;
        } else {
            j++;
        }
    }
    *score = -sum / 2.0;
    return ORBX_OK;
}

int orbx_kfdb_create(const orbx_vocabulary* voc, int max_keyframes, int cap, orbx_kfdb** out) {
    if (!out) return fail(ORBX_ERR_ARG, "null argument");
    *out = nullptr;
    if (max_keyframes < 1 || cap < 1) return fail(ORBX_ERR_ARG, "bad argument");
    if (max_keyframes > kKfdbMaxKeyframes) return fail(ORBX_ERR_UNSUPPORTED, "more than 8192 keyframes");
    if (cap > kKfdbMaxCap) return fail(ORBX_ERR_UNSUPPORTED, "more than 8192 words per keyframe");
    if (!voc) return fail(ORBX_ERR_ARG, "null vocabulary");
    int scoring = 0, nwords = 0;
    int rc = orbx_vocabulary_info(voc, nullptr, nullptr, &scoring, nullptr, nullptr, &nwords);
    if (rc) return rc;
    if (scoring != 0) return fail(ORBX_ERR_UNSUPPORTED, "only L1_NORM scoring is built (ORB-SLAM2's vocabulary)");
    orbx_kfdb* d = new (std::nothrow) orbx_kfdb();
    if (!d) return fail(ORBX_ERR_ARG, "out of host memory");
    d->device = vocabulary_device(voc);
    d->nwords = nwords;
    d->max_kf = max_keyframes;
    d->cap = cap;
    const size_t nmeta = (size_t)max_keyframes * (3 + kKfdbCovis);
    d->h_meta.assign(nmeta, 0);
    std::fill(h_covis(d), h_covis(d) + (size_t)max_keyframes * kKfdbCovis, -1);
    d->seq.assign((size_t)max_keyframes, 0);
    const size_t slots = (size_t)max_keyframes * cap;
    hipError_t e = hipSetDevice(d->device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void**)&d->words, slots * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&d->values, slots * 8);
    if (e == hipSuccess) e = hipMalloc((void**)&d->count, (size_t)max_keyframes * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&d->reloc, (size_t)max_keyframes * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&d->meta, nmeta * 4);
    if (e == hipSuccess) e = hipMemsetAsync(d->count, 0, (size_t)max_keyframes * 4, d->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d->reloc, 0, (size_t)max_keyframes * 4, d->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(d->stream);
    if (e != hipSuccess) {
        free_db(d);
        delete d;
        set_last_error(std::string("orbx_kfdb_create: ") + hipGetErrorString(e));
        return ORBX_ERR_HIP;
    }
    *out = d;
    return ORBX_OK;
}

void orbx_kfdb_destroy(orbx_kfdb* d) {
    if (!d || orbx::unloading()) return;
    (void)hipSetDevice(d->device);
    if (d->last) (void)hipStreamSynchronize(d->last);
    if (d->stream) (void)hipStreamSynchronize(d->stream);
    free_db(d);
    delete d;
}

int orbx_kfdb_info(const orbx_kfdb* d, int* max_keyframes, int* cap, int* size) {
    if (!d) return fail(ORBX_ERR_ARG, "null database");
    if (max_keyframes) *max_keyframes = d->max_kf;
    if (cap) *cap = d->cap;
    if (size) *size = d->live;
    return ORBX_OK;
}

void* orbx_kfdb_stream(orbx_kfdb* d) { return d ? (void*)d->stream : nullptr; }

int orbx_kfdb_add_batch_device(orbx_kfdb* d, int n, const int32_t* ids, const int32_t* d_bow_word,
                               const double* d_bow_value, const int32_t* d_nbow, int src_cap, void* stream) {
    if (!d || n < 0 || src_cap < 0) return fail(ORBX_ERR_ARG, "bad argument");
    if (n == 0) return ORBX_OK;
    if (!ids || !d_nbow || (src_cap && (!d_bow_word || !d_bow_value))) return fail(ORBX_ERR_ARG, "null argument");
    if (d->live + n > d->max_kf) return fail(ORBX_ERR_CAPACITY, "database full");
    std::vector<uint8_t> seen((size_t)d->max_kf, 0);
    for (int i = 0; i < n; i++) {
        if (ids[i] < 0 || ids[i] >= d->max_kf) return fail(ORBX_ERR_ARG, "keyframe id outside [0, max_keyframes)");
        if (h_alive(d)[ids[i]] || seen[ids[i]]) return fail(ORBX_ERR_STATE, "keyframe id already in the database");
        seen[ids[i]] = 1;
    }
    hipStream_t s;
    int rc = enter(d, stream, &s);
    if (rc) return rc;
    // the counts decide cap overflow before anything is stored
    std::vector<int32_t> cnt((size_t)n);
    HIP_TRY(hipMemcpyAsync(cnt.data(), d_nbow, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int i = 0; i < n; i++)
        if (cnt[i] < 0 || cnt[i] > d->cap || cnt[i] > src_cap)
            return fail(ORBX_ERR_CAPACITY, "BowVector longer than the database's cap");
    HIP_TRY(d->stage.reserve(up256((size_t)n * 4), s));
    HIP_TRY(hipMemcpyAsync(d->stage.p, ids, (size_t)n * 4, hipMemcpyHostToDevice, s));
    k_kfdb_add<<<n, 256, 0, s>>>(d->words, d->values, d->count, d->reloc, d->max_kf, d->cap, (const int32_t*)d->stage.p,
                                 d_bow_word, d_bow_value, d_nbow, src_cap);
    HIP_TRY(hipGetLastError());
    for (int i = 0; i < n; i++) {
        h_alive(d)[ids[i]] = 1;
        d->seq[ids[i]] = d->next_seq++;
        std::fill(h_covis(d) + (size_t)ids[i] * kKfdbCovis, h_covis(d) + (size_t)(ids[i] + 1) * kKfdbCovis, -1);
    }
    d->live += n;
    d->dirty = true;
    return ORBX_OK;
}

int orbx_kfdb_add(orbx_kfdb* d, int id, const int32_t* word, const double* value, int n) {
    if (!d || n < 0 || (n && (!word || !value))) return fail(ORBX_ERR_ARG, "bad argument");
    if (n > d->cap) return fail(ORBX_ERR_CAPACITY, "BowVector longer than the database's cap");
    hipStream_t s;
    int rc = enter(d, nullptr, &s);
    if (rc) return rc;
    const int cap = n > 0 ? n : 1;
    const size_t b_w = up256((size_t)cap * 4), b_v = up256((size_t)cap * 8);
    HIP_TRY(d->stage_add.reserve(b_w + b_v + 256, s));
    int32_t* d_w = (int32_t*)d->stage_add.p;
    double* d_v = (double*)(d->stage_add.p + b_w);
    int32_t* d_n = (int32_t*)(d->stage_add.p + b_w + b_v);
    if (n) {
        HIP_TRY(hipMemcpyAsync(d_w, word, (size_t)n * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_v, value, (size_t)n * 8, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipMemcpyAsync(d_n, &n, 4, hipMemcpyHostToDevice, s));
    return orbx_kfdb_add_batch_device(d, 1, &id, d_w, d_v, d_n, cap, nullptr);
}

int orbx_kfdb_erase(orbx_kfdb* d, int id) {
    if (!d || id < 0 || id >= d->max_kf) return fail(ORBX_ERR_ARG, "bad argument");
    if (!h_alive(d)[id]) return fail(ORBX_ERR_STATE, "keyframe id not in the database");
    h_alive(d)[id] = 0;
    d->live--;
    d->dirty = true;
    return ORBX_OK;
}

int orbx_kfdb_clear(orbx_kfdb* d) {
    if (!d) return fail(ORBX_ERR_ARG, "null database");
    std::fill(h_alive(d), h_alive(d) + d->max_kf, 0);
    d->live = 0;
    d->dirty = true;
    return ORBX_OK;
}

int orbx_kfdb_set_covisibility(orbx_kfdb* d, int id, const int32_t* best, int n) {
    if (!d || id < 0 || id >= d->max_kf || n < 0 || n > kKfdbCovis || (n && !best))
        return fail(ORBX_ERR_ARG, "bad argument");
    if (!h_alive(d)[id]) return fail(ORBX_ERR_STATE, "keyframe id not in the database");
    int32_t* row = h_covis(d) + (size_t)id * kKfdbCovis;
    for (int j = 0; j < kKfdbCovis; j++) row[j] = j < n ? best[j] : -1;
    d->dirty = true;
    return ORBX_OK;
}

int orbx_kfdb_reloc_scores(orbx_kfdb* d, float* scores) {
    if (!d || !scores) return fail(ORBX_ERR_ARG, "null argument");
    hipStream_t s;
    int rc = enter(d, nullptr, &s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(scores, d->reloc, (size_t)d->max_kf * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int id = 0; id < d->max_kf; id++)
        if (!h_alive(d)[id]) scores[id] = 0.0f;
    return ORBX_OK;
}

int orbx_kfdb_score_device(orbx_kfdb* d, const int32_t* d_qword, const double* d_qvalue, const int32_t* d_qn,
                           int qcap, const int32_t* d_ids, int nids, float* d_score, void* stream) {
    if (!d || qcap < 0 || nids < 0) return fail(ORBX_ERR_ARG, "bad argument");
    if (nids == 0) return ORBX_OK;
    if (!d_qword || !d_qvalue || !d_qn || !d_ids || !d_score) return fail(ORBX_ERR_ARG, "null argument");
    if (qcap > kKfdbMaxCap) return fail(ORBX_ERR_UNSUPPORTED, "more than 8192 words per query");
    hipStream_t s;
    int rc = enter(d, stream, &s);
    if (rc) return rc;
    rc = flush_meta(d, s);
    if (rc) return rc;
    k_kfdb_score_ids<<<(nids + kPairWaves - 1) / kPairWaves, kPairThreads, (size_t)(qcap > 0 ? qcap : 1) * 4, s>>>(
        view(d), d_qword, d_qvalue, d_qn, qcap, d_ids, nids, d_score);
    HIP_TRY(hipGetLastError());
    return ORBX_OK;
}

int orbx_kfdb_detect_relocalization_candidates_device(orbx_kfdb* d, int batch, const int32_t* d_qword,
                                                      const double* d_qvalue, const int32_t* d_qn, int qcap,
                                                      int32_t* d_cand, int max_cand, int32_t* d_ncand,
                                                      int32_t* d_words, float* d_score, void* stream) {
    return detect(d, 0, batch, d_qword, d_qvalue, d_qn, qcap, nullptr, nullptr, nullptr, d_cand, max_cand, d_ncand,
                  d_words, d_score, stream);
}

int orbx_kfdb_detect_loop_candidates_device(orbx_kfdb* d, int batch, const int32_t* d_qword, const double* d_qvalue,
                                            const int32_t* d_qn, int qcap, const int32_t* d_conn_off,
                                            const int32_t* d_conn_ids, const float* d_min_score, int32_t* d_cand,
                                            int max_cand, int32_t* d_ncand, int32_t* d_words, float* d_score,
                                            void* stream) {
    return detect(d, 1, batch, d_qword, d_qvalue, d_qn, qcap, d_conn_off, d_conn_ids, d_min_score, d_cand, max_cand,
                  d_ncand, d_words, d_score, stream);
}

int orbx_kfdb_detect_relocalization_candidates(orbx_kfdb* d, const int32_t* word, const double* value, int n,
                                               int32_t* cand, int max_cand, int* ncand) {
    return detect_host(d, 0, word, value, n, nullptr, 0, 0.0f, cand, max_cand, ncand);
}

int orbx_kfdb_detect_loop_candidates(orbx_kfdb* d, const int32_t* word, const double* value, int n,
                                     const int32_t* connected, int nconnected, float min_score, int32_t* cand,
                                     int max_cand, int* ncand) {
    return detect_host(d, 1, word, value, n, connected, nconnected, min_score, cand, max_cand, ncand);
}

}  // extern "C"
