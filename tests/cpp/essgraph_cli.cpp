// Drives orbx::Optimizer::OptimizeEssentialGraph (include/orbx.hpp) on one map read from a text
// file and prints the results' bytes, for tests/test_essential_graph_cpp.py.
//   essgraph_cli <graph.txt>
// graph.txt: n_kf n_corr n_edges n_pt loop fix_scale / n_kf lines "corr Tcw (12)" / n_corr lines
// "S (8)" / n_edges lines "i j kind" / n_pt lines "ref X Y Z"; floats and doubles as hex bit
// patterns.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbx.hpp"

static float rdf(FILE* f) {
    unsigned u = 0;
    if (fscanf(f, "%x", &u) != 1) throw std::runtime_error("bad input");
    float v;
    std::memcpy(&v, &u, 4);
    return v;
}

static double rdd(FILE* f) {
    unsigned long long u = 0;
    if (fscanf(f, "%llx", &u) != 1) throw std::runtime_error("bad input");
    double v;
    std::memcpy(&v, &u, 8);
    return v;
}

static int rdi(FILE* f) {
    int v = 0;
    if (fscanf(f, "%d", &v) != 1) throw std::runtime_error("bad input");
    return v;
}

static void hex(const char* name, const float* v, size_t n) {
    printf("%s", name);
    for (size_t i = 0; i < n; i++) {
        unsigned u;
        std::memcpy(&u, &v[i], 4);
        printf(" %08x", u);
    }
    printf("\n");
}

static void hex(const char* name, const double* v, size_t n) {
    printf("%s", name);
    for (size_t i = 0; i < n; i++) {
        unsigned long long u;
        std::memcpy(&u, &v[i], 8);
        printf(" %016llx", u);
    }
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    try {
        FILE* f = fopen(argv[1], "r");
        if (!f) return 2;
        const int n_kf = rdi(f), n_corr = rdi(f), n_edges = rdi(f), n_pt = rdi(f), loop = rdi(f), fix = rdi(f);
        std::vector<float> Tcw((size_t)n_kf * 12), pos((size_t)n_pt * 3);
        std::vector<int32_t> corr((size_t)n_kf), ev((size_t)n_edges * 2), kind((size_t)n_edges), ref((size_t)n_pt);
        std::vector<double> cS((size_t)n_corr * 8), Scw;
        for (int k = 0; k < n_kf; k++) {
            corr[k] = rdi(f);
            for (int i = 0; i < 12; i++) Tcw[(size_t)k * 12 + i] = rdf(f);
        }
        for (double& v : cS) v = rdd(f);
        for (int e = 0; e < n_edges; e++) {
            ev[2 * e] = rdi(f);
            ev[2 * e + 1] = rdi(f);
            kind[e] = rdi(f);
        }
        for (int p = 0; p < n_pt; p++) {
            ref[p] = rdi(f);
            for (int i = 0; i < 3; i++) pos[(size_t)p * 3 + i] = rdf(f);
        }
        fclose(f);
        orbx::ORBmatcher matcher(0.75f, true);
        int32_t trace[2];
        double chi2[2];
        const int status =
            orbx::Optimizer::OptimizeEssentialGraph(matcher, Tcw, corr, cS, loop, ev, kind, pos, ref, fix != 0, &Scw, trace, chi2);
        printf("status %d trace %d %d\n", status, trace[0], trace[1]);
        hex("Tcw", Tcw.data(), Tcw.size());
        hex("pos", pos.data(), pos.size());
        hex("Scw", Scw.data(), Scw.size());
        hex("chi2", chi2, 2);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
