// Drives orbx::Optimizer::BundleAdjustment (include/orbx.hpp) on one map read from a text file
// and prints the results' bytes, for tests/test_global_ba_cpp.py.
//   globalba_cli <map.txt>
// map.txt: n_kf n_pt n_obs n_slots cap nlevels has_u_right iterations robust / fx fy cx cy bf /
// invSigma2 (nlevels) / n_kf lines "fixed slot Tcw (12)" / n_pt lines "X Y Z" / obs_off
// (n_pt + 1) / n_obs lines "kf kp" / n_slots * cap lines "x y octave u_right"; floats as hex
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

static void hex(const char* name, const float* v, size_t n) {
    printf("%s", name);
    for (size_t i = 0; i < n; i++) {
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
        const int n_kf = rdi(f), n_pt = rdi(f), n_obs = rdi(f), n_slots = rdi(f), cap = rdi(f), nlevels = rdi(f),
                  has_ur = rdi(f), iterations = rdi(f), robust = rdi(f);
        float K[5];
        for (float& v : K) v = rdf(f);
        std::vector<float> sig((size_t)nlevels), Tcw((size_t)n_kf * 12), pos((size_t)n_pt * 3), ur;
        for (float& v : sig) v = rdf(f);
        std::vector<uint8_t> fixed((size_t)n_kf), notIncluded;
        std::vector<int32_t> slot((size_t)n_kf), off((size_t)n_pt + 1), okf((size_t)n_obs), okp((size_t)n_obs);
        for (int k = 0; k < n_kf; k++) {
            fixed[k] = (uint8_t)rdi(f);
            slot[k] = rdi(f);
            for (int i = 0; i < 12; i++) Tcw[(size_t)k * 12 + i] = rdf(f);
        }
        for (float& v : pos) v = rdf(f);
        for (int32_t& v : off) v = rdi(f);
        for (int o = 0; o < n_obs; o++) {
            okf[o] = rdi(f);
            okp[o] = rdi(f);
        }
        std::vector<orbx_keypoint> keys((size_t)n_slots * cap);
        if (has_ur) ur.resize(keys.size());
        for (size_t i = 0; i < keys.size(); i++) {
            std::memset(&keys[i], 0, sizeof(orbx_keypoint));
            keys[i].x = rdf(f);
            keys[i].y = rdf(f);
            keys[i].octave = rdi(f);
            const float r = rdf(f);
            if (has_ur) ur[i] = r;
        }
        fclose(f);
        orbx::ORBmatcher matcher(0.75f, true);
        int32_t trace[2];
        double chi2[2];
        const int status = orbx::Optimizer::BundleAdjustment(matcher, Tcw, fixed, slot, pos, off, okf, okp, keys, ur, cap,
                                                             sig, K[0], K[1], K[2], K[3], K[4], iterations, robust != 0,
                                                             &notIncluded, trace, chi2);
        printf("status %d\n", status);
        hex("Tcw", Tcw.data(), Tcw.size());
        hex("pos", pos.data(), pos.size());
        printf("trace %d %d\n", trace[0], trace[1]);
        unsigned long long c[2];
        std::memcpy(c, chi2, 16);
        printf("chi2 %016llx %016llx\n", c[0], c[1]);
        printf("not_included");
        for (uint8_t v : notIncluded) printf(" %d", (int)v);
        printf("\n");
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
