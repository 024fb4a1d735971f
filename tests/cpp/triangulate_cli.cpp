// Drives orbx::LocalMapping::TriangulatePairs (include/orbx.hpp) on one matched pair read from a
// text file and prints the result's bytes, for tests/test_gpu_triangulate.py.
//   triangulate_cli <pair.txt>
// pair.txt: fx fy cx cy mb mbf / nlevels / mvScaleFactors (nlevels) / mvLevelSigma2 (nlevels) /
// then per keyframe: Tcw (12) / "x y octave" of mvKeysUn / "has x y" of mvKeys / "has u_right" /
// "has depth" (has = 0: the array is not passed); floats as hex bit patterns.
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
    printf(" %s", name);
    for (int i = 0; i < n; i++) {
        unsigned u;
        std::memcpy(&u, &v[i], 4);
        printf(" %08x", u);
    }
}

static orbx::LocalMapping::KeyFrameGeom read_keyframe(FILE* f) {
    orbx::LocalMapping::KeyFrameGeom K;
    for (float& v : K.mTcw) v = rdf(f);
    orbx_keypoint kp{};
    kp.x = rdf(f);
    kp.y = rdf(f);
    kp.octave = rdi(f);
    K.mvKeysUn.push_back(kp);
    const int has_raw = rdi(f);
    kp.x = rdf(f);
    kp.y = rdf(f);
    if (has_raw) K.mvKeys.push_back(kp);
    const int has_ur = rdi(f);
    const float ur = rdf(f);
    if (has_ur) K.mvuRight.push_back(ur);
    const int has_depth = rdi(f);
    const float depth = rdf(f);
    if (has_depth) K.mvDepth.push_back(depth);
    return K;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    try {
        FILE* f = fopen(argv[1], "r");
        if (!f) return 2;
        orbx_frame_view cam{};
        cam.fx = rdf(f);
        cam.fy = rdf(f);
        cam.cx = rdf(f);
        cam.cy = rdf(f);
        const float mb = rdf(f), mbf = rdf(f);
        cam.nlevels = rdi(f);
        if (cam.nlevels < 1 || cam.nlevels > ORBX_MAX_LEVELS) throw std::runtime_error("bad input");
        std::vector<float> scale((size_t)cam.nlevels), sigma2((size_t)cam.nlevels);
        for (float& v : scale) v = rdf(f);
        for (float& v : sigma2) v = rdf(f);
        cam.scale_factors = scale.data();
        cam.level_sigma2 = sigma2.data();
        const orbx::LocalMapping::KeyFrameGeom K1 = read_keyframe(f), K2 = read_keyframe(f);
        fclose(f);
        orbx::ORBmatcher matcher(0.6f, false);  // LocalMapping.cc:243
        orbx::LocalMapping::NewMapPoints out;
        const int nnew = orbx::LocalMapping::TriangulatePairs(matcher, K1, K2, cam, {0, 0}, mb, mbf, out);
        printf("reason %d method %d", (int)out.reason[0], (int)out.method[0]);
        hex("pos", out.pos.data(), 3);
        hex("normal", out.normal.data(), 3);
        hex("max", out.maxDistance.data(), 1);
        hex("min", out.minDistance.data(), 1);
        printf(" nnew %d\n", nnew);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
