// Drives orbx::Sim3Solver (include/orbx.hpp) on one candidate read from a text file and prints
// the results' bytes after every call, for tests/test_sim3_host.py and tests/test_gpu_sim3.py.
//   sim3_cli <candidate.txt> <call> [<call> ...]     call: an iteration count, or "find"
// candidate.txt: n1 n_mp nlevels fix_scale min_inliers max_iterations / probability (hex bits of
// the float) / K1 (4) / K2 (4) / Tcw1 (12) / Tcw2 (12) / level_sigma2 (nlevels) / n1 lines
// "mp1 mp2 oct1 oct2" / n_mp lines "X Y Z" / max_iterations lines "r0 r1 r2"; floats as hex
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

static void hex(const char* tag, const std::vector<float>& a) {
    printf("%s", tag);
    for (float t : a) {
        unsigned u;
        std::memcpy(&u, &t, 4);
        printf(" %08x", u);
    }
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    try {
        FILE* f = fopen(argv[1], "r");
        if (!f) return 2;
        const int n1 = rdi(f), n_mp = rdi(f), nlevels = rdi(f), fix = rdi(f), min_inliers = rdi(f), max_its = rdi(f);
        const float prob = rdf(f);
        float K1[4], K2[4], T1[12], T2[12];
        for (float& k : K1) k = rdf(f);
        for (float& k : K2) k = rdf(f);
        for (float& t : T1) t = rdf(f);
        for (float& t : T2) t = rdf(f);
        std::vector<float> sig((size_t)nlevels), pos((size_t)n_mp * 3);
        for (float& s : sig) s = rdf(f);
        std::vector<int32_t> mp1((size_t)n1), mp2((size_t)n1), o1((size_t)n1), o2((size_t)n1), draws((size_t)max_its * 3);
        for (int i = 0; i < n1; i++) {
            mp1[i] = rdi(f);
            mp2[i] = rdi(f);
            o1[i] = rdi(f);
            o2[i] = rdi(f);
        }
        for (float& p : pos) p = rdf(f);
        for (int32_t& d : draws) d = rdi(f);
        fclose(f);
        orbx::ORBmatcher matcher(0.75f, true);
        orbx::Sim3Solver solver(matcher, mp1, mp2, o1, o2, pos, T1, T2, sig, K1, K2, fix != 0, draws);
        solver.SetRansacParameters((double)prob, min_inliers, max_its);
        for (int c = 2; c < argc; c++) {
            bool no_more = false;
            std::vector<bool> inl;
            int n = 0;
            std::vector<float> T;
            if (!std::strcmp(argv[c], "find")) T = solver.find(inl, n);
            else T = solver.iterate(atoi(argv[c]), no_more, inl, n);
            printf("call %s found %d no_more %d inliers %d best %d at %d iterations %d pairs %d status %d\n", argv[c],
                   T.empty() ? 0 : 1, no_more ? 1 : 0, n, solver.bestInliers, solver.bestIteration, solver.iterations,
                   solver.N, solver.status);
            hex("T12", T);
            hex("R", solver.GetEstimatedRotation());
            hex("t", solver.GetEstimatedTranslation());
            hex("s", {solver.GetEstimatedScale()});
            printf("flags ");
            for (bool b : inl) putchar(b ? '1' : '0');
            printf("\n");
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
