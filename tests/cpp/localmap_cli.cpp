// Drives orbx::Tracking::UpdateLocalMap (include/orbx.hpp) on one map and a batch of frames read
// from a text file and prints the local maps, for tests/test_local_map_model.py.
//   localmap_cli <frames.txt>
// frames.txt: K cap n_mp max_conn / K lines "n id (cap)" / n_mp bad flags / "m id (m)" the keyframes
// that go bad after every keyframe was connected / B max_local_kf max_local_points max_total /
// B lines "n id (cap)".  Print, per frame: "b: status s ref r kf ...", "points ...", "frame ...".
#include <cstdint>
#include <cstdio>
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
        std::vector<int32_t> kf_mp((size_t)K * cap), kf_n((size_t)K), ids((size_t)K);
        std::vector<uint8_t> kf_bad((size_t)K, 0), mp_bad((size_t)n_mp);
        for (int k = 0; k < K; k++) {
            kf_n[k] = rdi(f);
            ids[k] = k;
            for (int i = 0; i < cap; i++) kf_mp[(size_t)k * cap + i] = rdi(f);
        }
        for (uint8_t& b : mp_bad) b = (uint8_t)rdi(f);
        orbx::Covisibility g(K, cap, n_mp, max_conn);
        g.RefreshObservations(kf_mp, kf_n, kf_bad, n_mp, mp_bad);
        g.UpdateConnections(ids);
        for (int m = rdi(f); m > 0; m--) kf_bad[(size_t)rdi(f)] = 1;
        g.RefreshObservations(kf_mp, kf_n, kf_bad, n_mp, mp_bad);
        const int B = rdi(f), max_kf = rdi(f), max_points = rdi(f), max_total = rdi(f);
        std::vector<int32_t> frame_mp((size_t)B * cap), n((size_t)B);
        for (int b = 0; b < B; b++) {
            n[b] = rdi(f);
            for (int i = 0; i < cap; i++) frame_mp[(size_t)b * cap + i] = rdi(f);
        }
        fclose(f);
        orbx::Tracking tracking(g);
        orbx::Tracking::LocalMaps lm;
        tracking.UpdateLocalMap(frame_mp, n, cap, lm, max_kf, max_points, max_total);
        for (int b = 0; b < B; b++) {
            printf("%d: status %d ref %d kf", b, lm.status[b], lm.referenceKF[b]);
            for (int j = 0; j < lm.nLocalKeyFrames[b]; j++) printf(" %d", lm.localKeyFrames[(size_t)b * max_kf + j]);
            printf("\npoints");
            for (int j = lm.localOff[b]; j < lm.localOff[b + 1]; j++) printf(" %d", lm.localMapPoints[j]);
            printf("\nframe");
            for (int i = 0; i < cap; i++) printf(" %d", frame_mp[(size_t)b * cap + i]);
            printf("\n");
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "localmap_cli: %s\n", e.what());
        return 1;
    }
    return 0;
}
