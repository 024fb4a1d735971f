// Drives orbx::Covisibility (include/orbx.hpp) on one map read from a text file and prints the
// graph's lists, for tests/test_covisibility_cpp.py.
//   covis_cli <map.txt>
// map.txt: K cap n_mp max_conn / K lines "n bad id (cap)" / n_mp bad flags / then commands, one
// per line: "u Q id (Q)" UpdateConnections, "e id" EraseKeyFrame, "r" RefreshObservations,
// "b id" set keyframe id bad, "p" print.  Print: per keyframe "k: kf:w ..." (the ordered list),
// then "best10 k: ...", "w15 k: ..." and the parents and first-connection flags from the view.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbx.hpp"

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
        const int K = rdi(f), cap = rdi(f), n_mp = rdi(f), max_conn = rdi(f);
        std::vector<int32_t> kf_mp((size_t)K * cap), kf_n((size_t)K);
        std::vector<uint8_t> kf_bad((size_t)K), mp_bad((size_t)n_mp);
        for (int k = 0; k < K; k++) {
            kf_n[k] = rdi(f);
            kf_bad[k] = (uint8_t)rdi(f);
            for (int i = 0; i < cap; i++) kf_mp[(size_t)k * cap + i] = rdi(f);
        }
        for (uint8_t& b : mp_bad) b = (uint8_t)rdi(f);
        orbx::Covisibility g(K, cap, n_mp, max_conn);
        g.RefreshObservations(kf_mp, kf_n, kf_bad, n_mp, mp_bad);
        char cmd[8];
        while (fscanf(f, "%7s", cmd) == 1) {
            if (cmd[0] == 'u') {
                std::vector<int32_t> ids((size_t)rdi(f));
                for (int32_t& v : ids) v = rdi(f);
                g.UpdateConnections(ids);
            } else if (cmd[0] == 'e') {
                g.EraseKeyFrame(rdi(f));
            } else if (cmd[0] == 'b') {
                kf_bad[(size_t)rdi(f)] = 1;
            } else if (cmd[0] == 'r') {
                g.RefreshObservations(kf_mp, kf_n, kf_bad, n_mp, mp_bad);
            } else if (cmd[0] == 'p') {
                for (int k = 0; k < K; k++) {
                    std::vector<int32_t> w, kf = g.GetVectorCovisibleKeyFrames(k, &w);
                    printf("%d:", k);
                    for (size_t i = 0; i < kf.size(); i++) printf(" %d:%d", kf[i], w[i]);
                    printf("\nbest10 %d:", k);
                    for (int32_t v : g.GetBestCovisibilityKeyFrames(k, 10)) printf(" %d", v);
                    printf("\nw15 %d:", k);
                    for (int32_t v : g.GetCovisiblesByWeight(k, 15)) printf(" %d", v);
                    printf("\n");
                }
                const orbx_covis_view v = g.View();
                std::vector<int32_t> parent((size_t)K);
                std::vector<uint8_t> first((size_t)K);
                orbx::check(orbx_covis_read(g.handle(), v.parent, parent.data(), parent.size() * 4));
                orbx::check(orbx_covis_read(g.handle(), v.first, first.data(), first.size()));
                printf("parent");
                for (int32_t p : parent) printf(" %d", p);
                printf("\nfirst");
                for (uint8_t b : first) printf(" %d", (int)b);
                printf("\n");
            }
        }
        fclose(f);
    } catch (const std::exception& e) {
        fprintf(stderr, "covis_cli: %s\n", e.what());
        return 1;
    }
    return 0;
}
