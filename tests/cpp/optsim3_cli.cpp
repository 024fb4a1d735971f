// Drives orbx::Optimizer::OptimizeSim3 (include/orbx.hpp) on one loop candidate read from a
// text file and prints the results' bytes, for tests/test_optimize_sim3_cpp.py.
//   optsim3_cli <candidate.txt>
// candidate.txt: n1 n2 n_mp nlevels fix_scale / K1 (4) / K2 (4) / Tcw1 (12) / Tcw2 (12) /
// R12 (9) t12 (3) s12 th2 / invSigma2_1 (nlevels) / invSigma2_2 (nlevels) / n1 lines
// "x y octave mp1 matches12 idx2" / n2 lines "x y octave" / n_mp lines "X Y Z"; floats as hex
// bit patterns.
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

static int rdi(FILE* f) {
    int v = 0;
    if (fscanf(f, "%d", &v) != 1) throw std::runtime_error("bad input");
    return v;
}

static void hex(const char* name, const float* v, int n) {
    printf("%s", name);
    for (int i = 0; i < n; i++) {
        unsigned u;
        std::memcpy(&u, &v[i], 4);
        printf(" %08x", u);
    }
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    try {
        FILE* f = fopen(argv[1], "r");
        if (!f) return 2;
        const int n1 = rdi(f), n2 = rdi(f), n_mp = rdi(f), nlevels = rdi(f), fix = rdi(f);
        float K1[4], K2[4], T1[12], T2[12], R[9], t[3];
        for (float& v : K1) v = rdf(f);
        for (float& v : K2) v = rdf(f);
        for (float& v : T1) v = rdf(f);
        for (float& v : T2) v = rdf(f);
        for (float& v : R) v = rdf(f);
        for (float& v : t) v = rdf(f);
        float s = rdf(f);
        const float th2 = rdf(f);
        std::vector<float> sig1((size_t)nlevels), sig2((size_t)nlevels), pos((size_t)n_mp * 3);
        for (float& v : sig1) v = rdf(f);
        for (float& v : sig2) v = rdf(f);
        std::vector<orbx_keypoint> k1((size_t)n1), k2((size_t)n2);
        std::vector<int32_t> mp1((size_t)n1), m12((size_t)n1), idx2((size_t)n1);
        for (int i = 0; i < n1; i++) {
            std::memset(&k1[i], 0, sizeof(orbx_keypoint));
            k1[i].x = rdf(f);
            k1[i].y = rdf(f);
            k1[i].octave = rdi(f);
            mp1[i] = rdi(f);
            m12[i] = rdi(f);
            idx2[i] = rdi(f);
        }
        for (int i = 0; i < n2; i++) {
            std::memset(&k2[i], 0, sizeof(orbx_keypoint));
            k2[i].x = rdf(f);
            k2[i].y = rdf(f);
            k2[i].octave = rdi(f);
        }
        for (float& p : pos) p = rdf(f);
        fclose(f);
        orbx::ORBmatcher matcher(0.75f, true);
        int32_t trace[4];
        int ncorr = 0, nbad = 0;
        const int inliers = orbx::Optimizer::OptimizeSim3(matcher, k1, mp1, m12, idx2, k2, pos, T1, T2, sig1, sig2, K1,
                                                          K2, R, t, &s, th2, fix != 0, trace, &ncorr, &nbad);
        printf("inliers %d ncorr %d nbad %d\n", inliers, ncorr, nbad);
        hex("R12", R, 9);
        hex("t12", t, 3);
        hex("s12", &s, 1);
        printf("trace");
        for (int v : trace) printf(" %d", v);
        printf("\nmatches12");
        for (int32_t v : m12) printf(" %d", v);
        printf("\n");
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
