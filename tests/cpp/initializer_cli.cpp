// Drives orbx::Initializer (include/orbx.hpp) on one frame pair read from a binary file and
// prints the results' bytes, for tests/test_initializer_host.py and tests/test_gpu_initializer.py.
//   initializer_cli <scene.bin>
// scene.bin: int32 n1 n2 iterations / float32 K (4) / n1 orbx_keypoint / n2 orbx_keypoint /
// int32 matches12 (n1) / int32 sets (iterations x 8).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbx.hpp"

template <class T>
static void rd(FILE* f, T* p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) throw std::runtime_error("bad input");
}

static void hex(const char* tag, const void* p, size_t bytes) {
    printf("%s ", tag);
    for (size_t i = 0; i < bytes; i++) printf("%02x", ((const unsigned char*)p)[i]);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    try {
        FILE* f = fopen(argv[1], "rb");
        if (!f) return 2;
        int32_t head[3];
        float K[4];
        rd(f, head, 3);
        rd(f, K, 4);
        const size_t n1 = (size_t)head[0], n2 = (size_t)head[1], its = (size_t)head[2];
        std::vector<orbx_keypoint> k1(n1), k2(n2);
        std::vector<int32_t> m12(n1), sets(its * 8);
        rd(f, k1.data(), n1);
        rd(f, k2.data(), n2);
        rd(f, m12.data(), n1);
        rd(f, sets.data(), its * 8);
        fclose(f);
        orbx::ORBmatcher matcher(0.9f, true);
        orbx::Initializer init(matcher, k1, K, 1.0f, (int)its);
        std::vector<float> R21, t21, p3d;
        std::vector<bool> tri;
        const bool ok = init.Initialize(k2, m12, R21, t21, p3d, tri, sets);
        printf("ok %d\n", ok ? 1 : 0);
        printf("model %d\n", init.model);
        printf("best %d %d\n", init.bestIterationH, init.bestIterationF);
        hex("R21", R21.data(), R21.size() * 4);
        hex("t21", t21.data(), t21.size() * 4);
        hex("p3d", p3d.data(), p3d.size() * 4);
        std::vector<uint8_t> flags(tri.size());
        for (size_t i = 0; i < tri.size(); i++) flags[i] = tri[i] ? 1 : 0;
        hex("triangulated", flags.data(), flags.size());
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
