// Dumps what make_plan precomputes for k_fast_cells (orbx_geometry.h), for one configuration:
//   fast_cells_plan W H nfeatures nlevels
// prints "FAIL why" for a refused frame, else "L ncells fc_wr fc_wc pyr_frame_bytes", one
// line per level "w h pitch off", then one line per cell "level x0 y0 cols rows src_off
// pitch src_al first_mask last_q last_mask", then for a few divisors d (the plan's workgroups
// per frame among them) "d fc_div_mul(d) exact", exact being fc_div_exact at the largest id
// with id * d < 2^31.  tests/test_fast_cells_plan.py checks them.
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
        return 0;
    }
    std::printf("%d %d %d %d %lld\n", pl.L, (int)pl.cells.size(), pl.fc_wr, pl.fc_wc, pl.pyr_frame_bytes);
    for (int l = 0; l < pl.L; l++)
        std::printf("%d %d %d %lld\n", pl.lv[l].w, pl.lv[l].h, pl.lv[l].pitch, pl.lv[l].off);
    for (const CellGeom& c : pl.cells)
        std::printf("%d %d %d %d %d %d %d %d %u %d %u\n", c.level, c.x0, c.y0, c.cols, c.rows, c.src_off, c.pitch,
                    c.src_al, c.first_mask, c.last_q, c.last_mask);
    const int per_frame = ((int)pl.cells.size() + 3) / 4;
    const int divs[] = {1, 2, 3, 7, 204, 1000, per_frame > 0 ? per_frame : 1};
    for (int d : divs) std::printf("%d %u %d\n", d, fc_div_mul(d), fc_div_exact((1ll << 31) / d - 1, d) ? 1 : 0);
    return 0;
}
