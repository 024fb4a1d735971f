// Dumps make_plan's k_pyramid tiling (orbx_geometry.h) with what the plan precomputes for
// the kernel beyond the rectangles, for one configuration:
//   pyramid_plan_fields W H nfeatures nlevels
// prints what tests/cpp/pyramid_plan.cpp prints ("L nseg", per segment "l0 nl nx ny lds_a
// lds_b", one line per level "w h" plus its resize tables, then per segment, tile and
// segment level "x0 y0 x1 y1 ox0 oy0 ox1 oy1"), then "pz_win", per segment, tile and segment
// level the 8 constants of the parallel table and the 17 tap entries of the rectangle's
// first quad, then per level >= 1 "nquads" and per quad its 17 tap entries.
// tests/test_pyramid_plan_fields.py checks them.
#include <cstdio>
#include <cstdlib>

#include "orbx_geometry.h"

using namespace orbx;

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const int W = std::atoi(argv[1]), H = std::atoi(argv[2]), nf = std::atoi(argv[3]), L = std::atoi(argv[4]);
    OrbParams p;
    if (!init_params(p, nf, 1.2f, L, 20, 7)) return 3;
    Plan pl;
    if (!make_plan(pl, p, W, H)) {
        std::printf("FAIL %s\n", pl.why ? pl.why : "");
        return 4;
    }
    std::printf("%d %d\n", pl.L, pl.pz_nseg);
    for (int s = 0; s < pl.pz_nseg; s++)
        std::printf("%d %d %d %d %d %d\n", pl.pz[s].l0, pl.pz[s].nl, pl.pz[s].nx, pl.pz[s].ny, pl.pz[s].lds_a,
                    pl.pz[s].lds_b);
    for (int l = 0; l < pl.L; l++) {
        const LevelGeom& g = pl.lv[l];
        std::printf("%d %d\n", g.w, g.h);
        if (l > 0) {
            const int16_t* xt = pl.rtab.data() + g.xtab_off;
            const int16_t* yt = pl.rtab.data() + g.ytab_off;
            for (int x = 0; x < g.w; x++) std::printf("%d %d ", xt[4 * x], xt[4 * x + 1]);
            std::printf("\n");
            for (int y = 0; y < g.h; y++) std::printf("%d %d ", yt[4 * y], yt[4 * y + 1]);
            std::printf("\n");
        }
    }
    for (int s = 0; s < pl.pz_nseg; s++)
        for (int t = 0; t < pl.pz[s].tiles * pl.pz[s].nl; t++) {
            const int16_t* R = pl.rtab.data() + pl.pz[s].off + (size_t)t * 8;
            std::printf("%d %d %d %d %d %d %d %d\n", R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7]);
        }
    std::printf("%d\n", pl.pz_win ? 1 : 0);
    for (int s = 0; s < pl.pz_nseg; s++)
        for (int t = 0; t < pl.pz[s].tiles * pl.pz[s].nl; t++) {
            const int16_t* c = pl.rtab.data() + pl.pz[s].coff + (size_t)t * kPzRec;
            std::printf("%d %d %d %d %d %d %d %d", c[0], c[1], c[2], c[3], c[4], c[5], (uint16_t)c[6], c[7]);
            for (int k = 0; k < 17; k++) std::printf(" %d", c[8 + k]);
            std::printf("\n");
        }
    for (int l = 1; l < pl.L; l++) {
        const int nqd = (pl.lv[l].w + 3) / 4;
        const int16_t* q = pl.rtab.data() + pl.lv[l].qtab_off;
        std::printf("%d\n", nqd);
        for (int i = 0; i < nqd; i++, q += kPzQuadRec) {
            for (int k = 0; k < 17; k++) std::printf("%d ", q[k]);
            std::printf("\n");
        }
    }
    return 0;
}
