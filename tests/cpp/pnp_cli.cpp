// Drives orbx::PnPsolver (include/orbx.hpp) on one candidate read from a text file and prints
// the results' bytes after every call, for tests/test_pnp_cpp.py.
//   pnp_cli <candidate.txt> <call> [<call> ...]     call: an iteration count, or "find"
// candidate.txt: n n_mp nlevels min_inliers max_iterations min_set n_draws / probability epsilon
// th2 / K (4) / level_sigma2 (nlevels) / n lines "x y octave match" / n_mp lines "X Y Z" / n_draws
// lines "r0 r1 r2 r3"; floats as hex bit patterns.
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

static void hex(const char* tag, const float* a, size_t n) {
    printf("%s", tag);
    for (size_t i = 0; i < n; i++) {
        unsigned u;
        std::memcpy(&u, &a[i], 4);
        printf(" %08x", u);
    }
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    try {
        FILE* f = fopen(argv[1], "r");
        if (!f) return 2;
        const int n = rdi(f), n_mp = rdi(f), nlevels = rdi(f), min_inliers = rdi(f), max_its = rdi(f), min_set = rdi(f),
                  n_draws = rdi(f);
        const float prob = rdf(f), eps = rdf(f), th2 = rdf(f);
        float K[4];
        for (float& k : K) k = rdf(f);
        std::vector<float> sig((size_t)nlevels), pos((size_t)n_mp * 3);
        for (float& s : sig) s = rdf(f);
        std::vector<orbx_keypoint> keys((size_t)n);
        std::vector<int32_t> mp((size_t)n), draws((size_t)n_draws * 4);
        for (int i = 0; i < n; i++) {
            keys[i] = orbx_keypoint{};
            keys[i].x = rdf(f);
            keys[i].y = rdf(f);
            keys[i].octave = rdi(f);
            mp[i] = rdi(f);
        }
        for (float& p : pos) p = rdf(f);
        for (int32_t& d : draws) d = rdi(f);
        fclose(f);
        orbx::ORBmatcher matcher(0.75f, true);
        orbx::PnPsolver solver(matcher, keys, mp, pos, sig, K, draws);
        solver.SetRansacParameters((double)prob, min_inliers, max_its, min_set, eps, th2);
        for (int c = 2; c < argc; c++) {
            bool no_more = false;
            std::vector<bool> inl;
            int ni = 0;
            std::vector<float> T;
            if (!std::strcmp(argv[c], "find")) T = solver.find(inl, ni);
            else T = solver.iterate(atoi(argv[c]), no_more, inl, ni);
            printf("call %s found %d no_more %d inliers %d refined %d best %d at %d iterations %d corr %d min %d its %d status %d\n",
                   argv[c], T.empty() ? 0 : 1, no_more ? 1 : 0, ni, solver.refined, solver.bestInliers,
                   solver.bestIteration, solver.iterations, solver.N, solver.minInliersUsed, solver.maxItsUsed,
                   solver.status);
            hex("Tcw", T.data(), T.size());
            hex("best", solver.bestTcw, 12);
            printf("flags ");
            for (bool b : inl) putchar(b ? '1' : '0');
            printf("\nmp");
            for (int32_t v : solver.frameMP) printf(" %d", v);
            printf("\n");
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
