// Drives orbx::Optimizer::PoseOptimization (include/orbx.hpp) on one frame read from a text
// file and prints the results' bytes, for tests/test_pose_opt_cpp.py.
//   poseopt_cli <frame.txt>
// frame.txt: n n_mp nlevels stereo / fx fy cx cy bf / Tcw (12) / invSigma2 (nlevels) /
// n lines "x y octave u_right mp" / n_mp lines "X Y Z"; floats as hex bit patterns.
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

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    try {
        FILE* f = fopen(argv[1], "r");
        if (!f) return 2;
        const int n = rdi(f), n_mp = rdi(f), nlevels = rdi(f), stereo = rdi(f);
        float cam[5], T[12];
        for (float& c : cam) c = rdf(f);
        for (float& t : T) t = rdf(f);
        std::vector<float> sig((size_t)nlevels), ur, pos((size_t)n_mp * 3);
        for (float& s : sig) s = rdf(f);
        std::vector<orbx_keypoint> keys((size_t)n);
        std::vector<int32_t> mp((size_t)n);
        if (stereo) ur.resize((size_t)n);
        for (int i = 0; i < n; i++) {
            std::memset(&keys[i], 0, sizeof(orbx_keypoint));
            keys[i].x = rdf(f);
            keys[i].y = rdf(f);
            keys[i].octave = rdi(f);
            const float r = rdf(f);
            if (stereo) ur[i] = r;
            mp[i] = rdi(f);
        }
        for (float& p : pos) p = rdf(f);
        fclose(f);
        orbx::ORBmatcher matcher(0.9f, true);
        std::vector<uint8_t> outlier;
        int32_t trace[8];
        int ninit = 0;
        const int inliers = orbx::Optimizer::PoseOptimization(matcher, keys, ur, mp, pos, sig, cam[0], cam[1], cam[2],
                                                              cam[3], cam[4], T, outlier, trace, &ninit);
        printf("inliers %d ninit %d\ntcw", inliers, ninit);
        for (float t : T) {
            unsigned u;
            std::memcpy(&u, &t, 4);
            printf(" %08x", u);
        }
        printf("\ntrace");
        for (int t : trace) printf(" %d", t);
        printf("\noutlier ");
        for (uint8_t o : outlier) putchar(o ? '1' : '0');
        printf("\n");
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
