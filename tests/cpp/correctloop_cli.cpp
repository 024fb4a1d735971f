// Drives orbx::LoopClosing (include/orbx.hpp) on one map read from a binary file and writes every
// result array to another, for tests/test_correct_loop_cpp.py.
//   correctloop_cli <in.bin> <out.bin>
// in.bin: int32 {K, cap, n_mp, max_conn, cur, loop, min_feat, nlevels, n_loop_ids, max_edges, max_lc},
// then kf_mp, kf_mp_fused [K][cap] i32, kf_n [K] i32, kf_bad [K] u8, mp_bad [n_mp] u8, poses [K][12]
// f32, mp_pos [n_mp][3] f32, mnCorrectedByKF, mnCorrectedReference, mpRefKF [n_mp] i32, octave [K][cap]
// i32, scale [nlevels] f32, Scw [8] f64, loop_off [K + 1] i32, loop_ids [n_loop_ids] i32.
// The chain: UpdateConnections of every keyframe, CorrectLoopPropagate, the fused table and a
// refresh, AssembleEssentialGraph.  out.bin: the arrays in the order of the put() calls below.
// The HIP runtime is used for device memory only.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

#include "orbx.hpp"

extern "C" {
int hipMalloc(void** p, size_t bytes);
int hipMemcpy(void* dst, const void* src, size_t bytes, int kind);
int hipMemset(void* p, int v, size_t bytes);
int hipDeviceSynchronize(void);
}

static FILE* g_in = nullptr;
static FILE* g_out = nullptr;

template <class T>
static std::vector<T> get(size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, g_in) != n) throw std::runtime_error("short input");
    return v;
}

template <class T>
static T* dev(const std::vector<T>& v, size_t n = 0, int fill = 0) {
    void* p = nullptr;
    const size_t bytes = (v.empty() ? n : v.size()) * sizeof(T);
    if (hipMalloc(&p, bytes ? bytes : 4)) throw std::runtime_error("hipMalloc");
    if (v.empty() ? hipMemset(p, fill, bytes ? bytes : 4) : hipMemcpy(p, v.data(), bytes, 1)) throw std::runtime_error("hip copy");
    return (T*)p;
}

template <class T>
static void put(const T* d, size_t n) {
    std::vector<T> v(n);
    if (hipDeviceSynchronize() || (n && hipMemcpy(v.data(), d, n * sizeof(T), 2))) throw std::runtime_error("hip copy");
    fwrite(v.data(), sizeof(T), n, g_out);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    try {
        g_in = fopen(argv[1], "rb");
        g_out = fopen(argv[2], "wb");
        if (!g_in || !g_out) return 2;
        const std::vector<int32_t> hd = get<int32_t>(11);
        const int K = hd[0], cap = hd[1], n = hd[2], max_conn = hd[3], cur = hd[4], loop = hd[5], min_feat = hd[6], nlevels = hd[7],
                  n_loop = hd[8], max_edges = hd[9], max_lc = hd[10];
        const size_t slots = (size_t)K * cap, m = (size_t)max_conn + 1;
        const auto kf_mp = get<int32_t>(slots), fused = get<int32_t>(slots), kf_n = get<int32_t>(K);
        const auto kf_bad = get<uint8_t>(K), mp_bad = get<uint8_t>(n);
        const auto poses = get<float>((size_t)K * 12), mp_pos = get<float>((size_t)n * 3);
        const auto by_kf = get<int32_t>(n), corr_ref = get<int32_t>(n), ref_kf = get<int32_t>(n), octave = get<int32_t>(slots);
        const auto scale = get<float>(nlevels);
        const auto Scw = get<double>(8);
        const auto loop_off = get<int32_t>((size_t)K + 1), loop_ids = get<int32_t>(n_loop);
        std::vector<orbx_keypoint> keys(slots);
        memset(keys.data(), 0, slots * sizeof(orbx_keypoint));
        for (size_t i = 0; i < slots; i++) keys[i].octave = octave[i];

        int32_t* d_kf_mp = dev(kf_mp);
        orbx::Covisibility g(K, cap, n, max_conn);
        const int32_t* d_kf_n = dev(kf_n);
        const uint8_t *d_kf_bad = dev(kf_bad), *d_mp_bad = dev(mp_bad);
        g.RefreshObservations(K, d_kf_mp, d_kf_n, d_kf_bad, n, d_mp_bad);
        std::vector<int32_t> all((size_t)K);
        std::iota(all.begin(), all.end(), 0);
        g.UpdateConnections(all);

        orbx::LoopClosing lc(g);
        const std::vector<int32_t> none;
        orbx_correct_loop_propagate p{};
        p.cur_kf = cur;
        p.Scw = dev(Scw);
        p.matched_kf = -1;
        p.kf_Tcw = dev(poses);
        p.mp_pos = dev(mp_pos);
        p.mp_corrected_by_kf = dev(by_kf);
        p.mp_corrected_ref = dev(corr_ref);
        p.mp_ref_kf = dev(ref_kf);
        p.kf_keys_un = dev(keys);
        p.scale_factors = scale.data();
        p.nlevels = nlevels;
        p.normal = dev(std::vector<float>(), (size_t)n * 3);
        p.max_distance = dev(std::vector<float>(), n);
        p.min_distance = dev(std::vector<float>(), n);
        p.conn = dev(none, m, 0xFF);
        p.n_conn = dev(none, 1);
        p.corr_S = dev(std::vector<double>(), m * 8);
        p.kf_corr = dev(none, K, 0xFF);
        p.kf_Tcw_nc = dev(std::vector<float>(), m * 12);
        p.status = dev(none, 1);
        lc.CorrectLoopPropagate(p);
        put(p.n_conn, 1);
        put(p.conn, m);
        put(p.corr_S, m * 8);
        put(p.kf_corr, K);
        put(p.kf_Tcw_nc, m * 12);
        put(p.status, 1);
        put(p.kf_Tcw, (size_t)K * 12);
        put(p.mp_pos, (size_t)n * 3);
        put(p.mp_corrected_by_kf, n);
        put(p.mp_corrected_ref, n);
        put(p.normal, (size_t)n * 3);
        put(p.max_distance, n);
        put(p.min_distance, n);

        if (hipDeviceSynchronize() || hipMemcpy(d_kf_mp, fused.data(), slots * 4, 1)) throw std::runtime_error("hip copy");
        g.RefreshObservations(K, d_kf_mp, d_kf_n, d_kf_bad, n, d_mp_bad);
        orbx_essential_graph_assembly a{};
        a.cur_kf = cur;
        a.loop_kf = loop;
        a.min_feat = min_feat;
        a.conn = p.conn;
        a.n_conn = p.n_conn;
        a.kf_corr = p.kf_corr;
        a.kf_Tcw_nc = p.kf_Tcw_nc;
        a.kf_Tcw = p.kf_Tcw;
        a.loop_off = dev(loop_off);
        a.loop_kf_ids = dev(loop_ids, 1);
        a.mp_corrected_by_kf = p.mp_corrected_by_kf;
        a.mp_corrected_ref = p.mp_corrected_ref;
        a.mp_ref_kf = p.mp_ref_kf;
        a.max_lc = max_lc;
        a.max_edges = max_edges;
        a.lc_off = dev(none, m + 1);
        a.lc_member = dev(none, m, 0xFF);
        a.lc_kf = dev(none, (size_t)max_lc + 1);
        a.lc_w = dev(none, (size_t)max_lc + 1);
        a.kf_ids = dev(none, K);
        a.kf_row = dev(none, K, 0xFF);
        a.n_rows = dev(none, 1);
        a.kf_off = dev(none, 2);
        a.loop_row = dev(none, 1);
        a.kf_corr_rows = dev(none, K);
        a.kf_Tcw_rows = dev(std::vector<float>(), (size_t)K * 12);
        a.edge_v = dev(none, ((size_t)max_edges + 1) * 2);
        a.edge_kind = dev(none, (size_t)max_edges + 1);
        a.n_edges = dev(none, 1);
        a.edge_off = dev(none, 2);
        a.pt_ref = dev(none, n);
        a.pt_off = dev(none, 2);
        a.env_blocks = dev(std::vector<int64_t>(), 1);
        a.status = dev(none, 1);
        lc.AssembleEssentialGraph(a);
        put(a.lc_off, m + 1);
        put(a.lc_member, m);
        put(a.lc_kf, (size_t)max_lc + 1);
        put(a.lc_w, (size_t)max_lc + 1);
        put(a.kf_ids, K);
        put(a.kf_row, K);
        put(a.n_rows, 1);
        put(a.kf_off, 2);
        put(a.loop_row, 1);
        put(a.kf_corr_rows, K);
        put(a.kf_Tcw_rows, (size_t)K * 12);
        put(a.edge_v, ((size_t)max_edges + 1) * 2);
        put(a.edge_kind, (size_t)max_edges + 1);
        put(a.n_edges, 1);
        put(a.edge_off, 2);
        put(a.pt_ref, n);
        put(a.pt_off, 2);
        put(a.env_blocks, 1);
        put(a.status, 1);

        orbx_normal_depth nd{};  // cc:1148 over every point, on the state the propagation left
        nd.kf_Tcw = p.kf_Tcw;
        nd.kf_keys_un = p.kf_keys_un;
        nd.mp_ref_kf = p.mp_ref_kf;
        nd.mp_pos = p.mp_pos;
        nd.scale_factors = scale.data();
        nd.nlevels = nlevels;
        nd.normal = p.normal;
        nd.max_distance = p.max_distance;
        nd.min_distance = p.min_distance;
        lc.UpdateNormalAndDepth(nd, nullptr, 0, p.status);
        put(p.normal, (size_t)n * 3);
        put(p.max_distance, n);
        put(p.min_distance, n);
        put(p.status, 1);
        fclose(g_in);
        fclose(g_out);
    } catch (const std::exception& e) {
        fprintf(stderr, "correctloop_cli: %s\n", e.what());
        return 1;
    }
    return 0;
}
