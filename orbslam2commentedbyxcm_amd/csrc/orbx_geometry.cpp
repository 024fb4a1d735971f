// orbx_geometry.cpp -- host-side extraction plan (see orbx_geometry.h).
// Compiled with -ffp-contract=off: every float expression below restates a
// reference expression operation by operation.
#include <algorithm>
#include "orbx_geometry.h"
#include "orbx_error.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace orbx {

static int cv_round(double v) { return (int)std::lrint(v); }   // cvRound: round half to even
static int cv_roundf(float v) { return (int)std::lrintf(v); }

// ORBextractor::ORBextractor, ORBextractor.cc:438-550
bool init_params(OrbParams& p, int nfeatures, float scale_factor, int nlevels, int ini, int min) {
    if (nlevels < 1 || nlevels > kMaxLevels || nfeatures < 0 || !(scale_factor > 1.0f)) return false;
    p.nfeatures = nfeatures;
    p.scale_factor = (double)scale_factor;
    p.nlevels = nlevels;
    p.ini_th = ini;
    p.min_th = min;
    p.scale[0] = 1.0f;
    p.sigma2[0] = 1.0f;
    for (int i = 1; i < nlevels; i++) {
        p.scale[i] = (float)((double)p.scale[i - 1] * p.scale_factor);   // cc:458
        p.sigma2[i] = p.scale[i] * p.scale[i];                            // cc:460
    }
    for (int i = 0; i < nlevels; i++) {
        p.inv_scale[i] = 1.0f / p.scale[i];                               // cc:468
        p.inv_sigma2[i] = 1.0f / p.sigma2[i];                             // cc:469
    }
    const float factor = (float)(1.0f / p.scale_factor);                   // cc:480
    float desired = (float)nfeatures * (1 - factor) /
                    (1 - (float)std::pow((double)factor, (double)nlevels));  // cc:485
    int sum = 0;
    for (int level = 0; level < nlevels - 1; level++) {                    // cc:490-498
        p.features[level] = cv_roundf(desired);
        sum += p.features[level];
        desired *= factor;
    }
    p.features[nlevels - 1] = nfeatures - sum > 0 ? nfeatures - sum : 0;  // cc:500
    // umax, cc:519-549
    const int vmax = (int)std::floor(15 * std::sqrt(2.f) / 2 + 1);
    const int vmin = (int)std::ceil(15 * std::sqrt(2.f) / 2);
    const double hp2 = 15 * 15;
    int v, v0;
    for (v = 0; v <= vmax; ++v) p.umax[v] = cv_round(std::sqrt(hp2 - v * v));
    for (v = 15, v0 = 0; v >= vmin; --v) {
        while (p.umax[v0] == p.umax[v0 + 1]) ++v0;
        p.umax[v] = v0;
        ++v0;
    }
    return true;
}

// OpenCV 3.3.1 resize(INTER_LINEAR) coefficient tables for CV_8U (11-bit fixed point).
static void resize_tables(int sw, int sh, int dw, int dh, int16_t* xtab, int16_t* ytab) {
    const double inv_scale_x = (double)dw / sw, inv_scale_y = (double)dh / sh;
    const double scale_x = 1. / inv_scale_x, scale_y = 1. / inv_scale_y;
    int xmax = dw;
    std::vector<int> sxs(dw);
    std::vector<float> fxs(dw);
    for (int dx = 0; dx < dw; dx++) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = (int)std::floor(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx + 1 >= sw) {
            if (dx < xmax) xmax = dx;
            if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
        }
        sxs[dx] = sx;
        fxs[dx] = fx;
    }
    for (int dx = 0; dx < dw; dx++) {
        int16_t* t = xtab + 4 * dx;
        if (dx < xmax) {
            t[0] = (int16_t)sxs[dx];
            t[1] = (int16_t)(sxs[dx] + 1);
            t[2] = (int16_t)cv_roundf((1.f - fxs[dx]) * 2048);
            t[3] = (int16_t)cv_roundf(fxs[dx] * 2048);
        } else {  // HResizeLinear tail: D = S[sx] * INTER_RESIZE_COEF_SCALE
            t[0] = (int16_t)sxs[dx];
            t[1] = (int16_t)sxs[dx];
            t[2] = 2048;
            t[3] = 0;
        }
    }
    for (int dy = 0; dy < dh; dy++) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = (int)std::floor(fy);
        fy -= sy;
        int16_t* t = ytab + 4 * dy;
        auto clip = [&](int y) { return y < 0 ? 0 : (y >= sh ? sh - 1 : y); };
        t[0] = (int16_t)clip(sy);
        t[1] = (int16_t)clip(sy + 1);
        t[2] = (int16_t)cv_roundf((1.f - fy) * 2048);
        t[3] = (int16_t)cv_roundf(fy * 2048);
    }
}

// Tap record of k_pyramid<true> for the column quad x .. x + 3 of a resized level, columns
// clamped to [lo, hi]: kPzQuadRec int16 (three 16-byte pieces) -- the four v_perm_b32
// selectors that pair source bytes sx0, sx1 of each column (relative to the first
// column's sx0) as u16 halves, the four (a0, a1) weight pairs, and the first column's sx0
// (the start of the row's source window).  A clamped column borrows its neighbour's taps
// (the quad's source span stays monotone): its byte is computed but never read by the
// next level and never owned.
static void quad_taps(const int16_t* xt, int x, int lo, int hi, int16_t* qt) {
    const int c00 = xt[4 * std::min(std::max(x, lo), hi)];
    for (int k = 0; k < 4; k++) {
        const int16_t* t = xt + 4 * std::min(std::max(x + k, lo), hi);
        // byte selectors hold only while pz_win's span check does (masked otherwise)
        qt[2 * k] = (int16_t)(((t[0] - c00) & 7) | 0x0c00);
        qt[2 * k + 1] = (int16_t)(((t[1] - c00) & 7) | 0x0c00);
        qt[8 + 2 * k] = t[2];
        qt[8 + 2 * k + 1] = t[3];
    }
    qt[16] = (int16_t)c00;
    for (int k = 17; k < kPzQuadRec; k++) qt[k] = 0;
}

// k_pyramid tile rectangles (orbx_geometry.h).  Ownership: level 0 is split into an
// nx x ny grid; a boundary b at level l - 1 moves to the first level-l column (row)
// whose resize source starts at or after b, so a tile's owned pixels at level l read
// only its own pixels at level l - 1 apart from the one-pixel right / bottom reach of
// the interpolation.  Needed rectangles are then grown from the top level down by the
// resize tables' source footprints (the tables are monotone, so a range of columns
// maps to [t(first).s0, t(last).s1]): the halo is 0 on the left / top and about
// 1 + 1.2 * (halo of the level above) on the right / bottom.
// Per (tile, level) one table holds the rectangles (8 int16) and a parallel one kPzRec
// int16 (orbx_geometry.h): what every thread of the workgroup would otherwise derive
// from the rectangles, and the tap record of the rectangle's first column quad.
// One segment: levels s.l0 .. s.l0 + s.nl - 1, tiled over level s.l0 (owned by the
// segment only when s.l0 == 0: a later segment's input level is already in HBM).
static bool pyramid_segment(Plan& plan, PzSeg& s, int tw, int th) {
    const int l0 = s.l0, n = s.nl;
    const LevelGeom& g0 = plan.lv[l0];
    const int nx = (g0.w + tw - 1) / tw, ny = (g0.h + th - 1) / th;
    s.nx = nx;
    s.ny = ny;
    s.tiles = nx * ny;
    plan.rtab.resize((plan.rtab.size() + 7) & ~(size_t)7);  // records are read as 16-byte pieces
    s.off = (int)plan.rtab.size();
    plan.rtab.resize(plan.rtab.size() + (size_t)nx * ny * n * 8);
    s.coff = (int)plan.rtab.size();
    plan.rtab.resize(plan.rtab.size() + (size_t)nx * ny * n * kPzRec);
    // owned boundaries per segment level: bx[k][0..nx], by[k][0..ny] (level l0 + k)
    std::vector<std::vector<int>> bx(n, std::vector<int>(nx + 1)), by(n, std::vector<int>(ny + 1));
    for (int j = 0; j <= nx; j++) bx[0][j] = (int)(((long long)j * g0.w) / nx);
    for (int i = 0; i <= ny; i++) by[0][i] = (int)(((long long)i * g0.h) / ny);
    for (int k = 1; k < n; k++) {
        const LevelGeom& g = plan.lv[l0 + k];
        const int16_t* xt = plan.rtab.data() + g.xtab_off;
        const int16_t* yt = plan.rtab.data() + g.ytab_off;
        for (int j = 0; j <= nx; j++) {
            int c = j == 0 ? 0 : bx[k][j - 1];
            while (c < g.w && (j == nx || xt[4 * c] < bx[k - 1][j])) c++;
            bx[k][j] = c;
        }
        for (int i = 0; i <= ny; i++) {
            int r = i == 0 ? 0 : by[k][i - 1];
            while (r < g.h && (i == ny || yt[4 * r] < by[k - 1][i])) r++;
            by[k][i] = r;
        }
    }
    for (int ty = 0; ty < ny; ty++)
        for (int tx = 0; tx < nx; tx++) {
            int16_t* R = plan.rtab.data() + s.off + (size_t)(ty * nx + tx) * n * 8;
            int16_t* Cn = plan.rtab.data() + s.coff + (size_t)(ty * nx + tx) * n * kPzRec;
            int nx0 = 0, ny0 = 0, nx1 = 0, ny1 = 0;  // needed rectangle of level l + 1
            for (int k = n - 1; k >= 0; k--) {
                const int l = l0 + k;
                int ox0 = bx[k][tx], ox1 = bx[k][tx + 1], oy0 = by[k][ty], oy1 = by[k][ty + 1];
                if (k == 0 && l0 > 0) ox0 = ox1 = oy0 = oy1 = 0;  // the input level: not owned here
                int x0 = ox0, x1 = ox1, y0 = oy0, y1 = oy1;
                bool any = ox1 > ox0 && oy1 > oy0;
                if (k + 1 < n && nx1 > nx0 && ny1 > ny0) {
                    const LevelGeom& u = plan.lv[l + 1];
                    const int16_t* xt = plan.rtab.data() + u.xtab_off;
                    const int16_t* yt = plan.rtab.data() + u.ytab_off;
                    const int sx0 = xt[4 * nx0], sx1 = xt[4 * (nx1 - 1) + 1] + 1;
                    const int sy0 = yt[4 * ny0], sy1 = yt[4 * (ny1 - 1) + 1] + 1;
                    if (any) {
                        x0 = std::min(x0, sx0); x1 = std::max(x1, sx1);
                        y0 = std::min(y0, sy0); y1 = std::max(y1, sy1);
                    } else {
                        x0 = sx0; x1 = sx1; y0 = sy0; y1 = sy1;
                    }
                    any = true;
                }
                if (!any) x0 = x1 = y0 = y1 = 0;
                // thread -> (column quad, row group) split of the rectangle (k_pyramid): G
                // groups of min(nq, 256) lanes, rc rows each; tid / nqp = (tid * mul) >> 16
                // for tid < 256 (mul = 65536 / nqp + 1 errs by under 256 / 65536 <= 1 / nqp)
                const int nq = any ? (x1 - (x0 & ~3) + 3) >> 2 : 0, nqp = std::min(nq, 256);
                const int G = any ? 256 / nqp : 0, rc = any ? (y1 - y0 + G - 1) / G : 0;
                const int mul = any ? 65536 / nqp + 1 : 0;
                const int16_t r[8] = {(int16_t)x0, (int16_t)y0, (int16_t)x1, (int16_t)y1,
                                      (int16_t)ox0, (int16_t)oy0, (int16_t)ox1, (int16_t)oy1};
                std::memcpy(R + 8 * k, r, sizeof(r));
                int16_t c[kPzRec] = {(int16_t)nq, (int16_t)G, (int16_t)rc, 0, 0, 0,
                                     (int16_t)(mul & 0xffff), (int16_t)(mul >> 16)};
                // the first quad starts at x0 & ~3, left of the rectangle when x0 is not on a
                // quad: those columns borrow x0's taps, so the quad's source window starts
                // inside the staged source rectangle (the level-wide records start theirs at
                // the quad's own first column)
                if (k >= 1 && any) quad_taps(plan.rtab.data() + plan.lv[l].xtab_off, x0 & ~3, x0, x1 - 1, c + 8);
                std::memcpy(Cn + kPzRec * k, c, sizeof(c));
                if (k + 1 < n) {  // this level's staged rectangle is the source of level k + 1
                    int16_t* U = Cn + kPzRec * (k + 1);
                    const int sxa = x0 & ~3;
                    U[3] = (int16_t)(4 * nq);  // LDS row stride of the source
                    U[4] = (int16_t)sxa;
                    U[5] = (int16_t)y0;
                }
                // LDS holds the needed columns widened to whole 4-byte quads
                // (+ 16: k_pyramid<true> reads a row's source window as three dwords, which
                // can reach 8 bytes past the last row's last quad)
                const int bytes = any ? 4 * ((x1 - (x0 & ~3) + 3) / 4) * (y1 - y0) : 0;
                int& buf = (k & 1) ? s.lds_b : s.lds_a;
                buf = std::max(buf, ((bytes + 15) & ~15) + 16);
                nx0 = x0; nx1 = x1; ny0 = y0; ny1 = y1;
            }
        }
    if (s.lds_a + s.lds_b > kPzMaxLds) { plan.why = "pyramid tile exceeds LDS (scale factor too large)"; return false; }
    return true;
}

static bool pyramid_tiles(Plan& plan) {
    const int L = plan.L;
    // debug builds: ORBX_PZ_TILE=WxH / ORBX_PZ_TILE2=WxH override the first / later
    // segments' tile size; switch pz_seg = n the levels per segment (0: one segment);
    // tuning, the output is the same
    int tw = kPzTW, th = kPzTH, tw2 = kPzTW2, th2 = kPzTH2, seg = kPzSegLevels;
    auto tile_env = [](const char* name, int& w, int& h) {
        int a = 0, b = 0;
        if (const char* e = debug_env(name))
            if (std::sscanf(e, "%dx%d", &a, &b) == 2 && a >= 16 && b >= 16) { w = a; h = b; }
    };
    tile_env("ORBX_PZ_TILE", tw, th);
    tile_env("ORBX_PZ_TILE2", tw2, th2);
    seg = tuning(Tune::PzSeg, seg);
    if (seg < 2 || seg > L) seg = L;
    plan.pz_nseg = 0;
    for (int l0 = 0;;) {
        PzSeg& s = plan.pz[plan.pz_nseg++];
        s = PzSeg{};
        s.l0 = l0;
        s.nl = std::min(seg, L - l0);
        if (!pyramid_segment(plan, s, l0 == 0 ? tw : tw2, l0 == 0 ? th : th2)) return false;
        if (l0 + s.nl >= L) break;
        l0 += s.nl - 1;
    }
    // k_pyramid<true> needs the source bytes of any 4 consecutive output columns (sx0 of the
    // first .. sx1 of the last) within 8 bytes: scale factors up to about 2
    // (switch pz_byte = 1 forces the byte-read form: tuning, the output is the same)
    plan.pz_win = tuning(Tune::PzByte, 0) <= 0;
    for (int l = 1; l < L && plan.pz_win; l++) {
        const LevelGeom& g = plan.lv[l];
        const int16_t* xt = plan.rtab.data() + g.xtab_off;
        for (int x = 0; x < g.w; x++)
            if (xt[4 * std::min(x + 3, g.w - 1) + 1] - xt[4 * x] > 7) { plan.pz_win = false; break; }
    }
    // Level-wide quad tap records (quad_taps), one per aligned column quad x = 4 q of every
    // resized level; columns past the level's width borrow the last column's taps.
    for (int l = 1; l < L; l++) {
        LevelGeom& g = plan.lv[l];
        const int nqd = (g.w + 3) / 4;
        plan.rtab.resize((plan.rtab.size() + 7) & ~(size_t)7);
        g.qtab_off = (int)plan.rtab.size();
        plan.rtab.resize(plan.rtab.size() + (size_t)nqd * kPzQuadRec, 0);
        for (int q = 0; q < nqd; q++)
            quad_taps(plan.rtab.data() + g.xtab_off, 4 * q, 0, g.w - 1, plan.rtab.data() + g.qtab_off + (size_t)q * kPzQuadRec);
    }
    // A rectangle's first quad takes the tile's own record, the others the level-wide ones
    // (their first column lies inside the rectangle).  The window form also needs every
    // quad's three-dword source window inside the staged source rectangle's rows plus
    // their 8 bytes of slack.
    for (int s = 0; s < plan.pz_nseg && plan.pz_win; s++) {
        const PzSeg& sg = plan.pz[s];
        for (int t = 0; t < sg.tiles * sg.nl && plan.pz_win; t++) {
            const int16_t* R = plan.rtab.data() + sg.off + (size_t)t * 8;
            const int16_t* Cn = plan.rtab.data() + sg.coff + (size_t)t * kPzRec;
            if (t % sg.nl == 0 || Cn[0] == 0) continue;
            const int16_t* qt = plan.rtab.data() + plan.lv[sg.l0 + t % sg.nl].qtab_off;
            for (int q = 0; q < Cn[0]; q++) {
                const int c00 = q == 0 ? Cn[8 + 16] : qt[(size_t)((R[0] >> 2) + q) * kPzQuadRec + 16];
                const int wb = (c00 & ~3) - Cn[4];
                if (wb < 0 || wb + 12 > Cn[3] + 8) { plan.pz_win = false; break; }
            }
        }
    }
    return true;
}

bool make_plan(Plan& plan, const OrbParams& prm, int W, int H) {
    plan = Plan();
    plan.prm = prm;
    plan.W = W;
    plan.H = H;
    plan.L = prm.nlevels;
    if (W <= 0 || H <= 0) { plan.why = "empty image"; return false; }
    long long off = 0;
    int cell_first = 0, key_off = 0, out_off = 0, tile_first = 0, slot_off = 0;
    int prev_w = W, prev_h = H;
    for (int l = 0; l < prm.nlevels; l++) {
        LevelGeom& g = plan.lv[l];
        std::memset(&g, 0, sizeof(g));
        const float s = prm.inv_scale[l];
        g.w = cv_roundf((float)W * s);                 // cc:1643
        g.h = cv_roundf((float)H * s);
        // below 33 px the reference's DistributeOctTree divides by a zero or negative
        // border-trimmed size (ORBextractor.cc:674-676: nIni = round(width / height),
        // vpIniNodes.resize(nIni)), so such frames are refused rather than given a meaning
        if (g.w < kMinLevelSide || g.h < kMinLevelSide) { plan.why = "pyramid level under 33 px"; return false; }
        if (g.w - 2 * kMinBorder >= 4096 || g.h - 2 * kMinBorder >= 4096) { plan.why = "frame too large"; return false; }
        g.pitch = (g.w + 63) & ~63;
        g.off = off;
        off += (long long)g.pitch * g.h;
        off = (off + 255) & ~255LL;
        g.scale = prm.scale[l];
        g.kp_size = (float)(int)(31 * prm.scale[l]);  // cc:1140
        g.N = prm.features[l];

        // FAST cell grid, cc:1025-1085
        const int minBorderX = kMinBorder, minBorderY = kMinBorder;
        const int maxBorderX = g.w - kEdge + 3, maxBorderY = g.h - kEdge + 3;
        const float width = (float)(maxBorderX - minBorderX);
        const float height = (float)(maxBorderY - minBorderY);
        const int nCols = (int)(width / 30.f);
        const int nRows = (int)(height / 30.f);
        // a level narrower or shorter than one 30-px FAST cell (under 62 px) has no cells:
        // the reference's cell loops run zero times and the level keeps no keypoints
        const bool no_cells = nCols <= 0 || nRows <= 0;
        const int wCell = no_cells ? 0 : (int)std::ceil(width / nCols);
        const int hCell = no_cells ? 0 : (int)std::ceil(height / nRows);
        g.cell_first = cell_first;
        g.key_off = key_off;
        int level_cap = 0;
        for (int i = 0; i < (no_cells ? 0 : nRows); i++) {
            const float iniY = (float)(minBorderY + i * hCell);
            float maxY = iniY + hCell + 6;
            if (iniY >= maxBorderY - 3) continue;
            if (maxY > maxBorderY) maxY = (float)maxBorderY;
            for (int j = 0; j < nCols; j++) {
                const float iniX = (float)(minBorderX + j * wCell);
                float maxX = iniX + wCell + 6;
                if (iniX >= maxBorderX - 6) continue;
                if (maxX > maxBorderX) maxX = (float)maxBorderX;
                CellGeom c{};
                c.level = l;
                c.x0 = (int)iniX;
                c.y0 = (int)iniY;
                c.cols = (int)maxX - c.x0;
                c.rows = (int)maxY - c.y0;
                const int wc = c.cols > 6 ? c.cols - 6 : 0, wr = c.rows > 6 ? c.rows - 6 : 0;
                if (wc > kCellMax || wr > kCellMax) { plan.why = "FAST cell wider than 64 px"; return false; }
                c.slot_off = slot_off;
                c.slot_cap = ((wc + 1) / 2) * ((wr + 1) / 2);
                c.pitch = g.pitch;
                plan.fc_wr = std::max(plan.fc_wr, wr);
                plan.fc_wc = std::max(plan.fc_wc, wc);
                c.src_off = (int)(g.off + (long long)(c.y0 + 3) * g.pitch + c.x0 + 3);
                if (wc > 0 && wr > 0) {
                    // k_fast_cells' dword staging: g.off and g.pitch are multiples of 4, so the
                    // window's rows all start a = src_off & 3 bytes into an aligned dword
                    const int a = c.src_off & 3, last = a + wc - 1;
                    if (a + wc > kFcSpan) { plan.why = "FAST cell window spans more than 16 aligned dwords"; return false; }
                    c.src_al = c.src_off - a;
                    c.first_mask = 0xffffffffu << (8 * a);
                    c.last_q = last >> 2;
                    c.last_mask = 0xffffffffu >> (8 * (3 - (last & 3)));
                    // the last load reads up to 3 rows past the window, every row 64 bytes
                    // from its aligned start (into the next row of the level when the window
                    // lies at its right end): all of it inside this level's block
                    const int nl = (wr + kFcRows - 1) / kFcRows;
                    if ((long long)c.src_al + (long long)(kFcRows * nl - 1) * g.pitch + kFcSpan > g.off + (long long)g.pitch * g.h) {
                        plan.why = "FAST cell loads reach past the level";
                        return false;
                    }
                }
                slot_off += c.slot_cap;
                level_cap += c.slot_cap;
                plan.cells.push_back(c);
            }
        }
        g.ncells = (int)plan.cells.size() - cell_first;
        cell_first = (int)plan.cells.size();
        g.key_cap = level_cap;
        key_off += level_cap;
        if (level_cap > plan.max_key_cap) plan.max_key_cap = level_cap;

        // octree roots, cc:674-699
        const int minX = minBorderX, maxX = maxBorderX, minY = minBorderY, maxY = maxBorderY;
        g.nIni = (int)std::round((float)(maxX - minX) / (maxY - minY));
        // a level without keypoints never reads its root nodes (DistributeOctTree of no keys)
        if (level_cap == 0) g.nIni = std::min(std::max(g.nIni, 1), kMaxIni);
        if (g.nIni < 1 || g.nIni > kMaxIni) { plan.why = "aspect ratio outside octree support"; return false; }
        g.hX = (float)(maxX - minX) / g.nIni;
        for (int i = 0; i <= g.nIni; i++) g.ini_x0[i] = (int)(g.hX * (float)i);
        g.height_rel = maxY - minY;
        int ncap = g.N + 4;
        if (4 * g.nIni + 4 > ncap) ncap = 4 * g.nIni + 4;
        if (prm.node_cap_limit > 0 && prm.node_cap_limit < ncap) ncap = prm.node_cap_limit;
        g.ncap = ncap;
        g.out_off = out_off;
        out_off += ncap;
        if (ncap > plan.max_ncap) plan.max_ncap = ncap;

        // score/blur tiles (kLtTW x kLtTH outputs)
        g.tiles_x = (g.w + kLtTW - 1) / kLtTW;
        g.tiles_y = (g.h + kLtTH - 1) / kLtTH;
        g.tile_first = tile_first;
        tile_first += g.tiles_x * g.tiles_y;

        // resize tables
        if (l > 0) {
            g.xtab_off = (int)plan.rtab.size();
            plan.rtab.resize(plan.rtab.size() + 4 * (size_t)g.w);
            g.ytab_off = (int)plan.rtab.size();
            plan.rtab.resize(plan.rtab.size() + 4 * (size_t)g.h);
            resize_tables(prev_w, prev_h, g.w, g.h, plan.rtab.data() + g.xtab_off, plan.rtab.data() + g.ytab_off);
            // k_pyramid's row walk: a level is never taller than its source, so an output
            // row's first source row is at or past the row before's second
            const int16_t* yt = plan.rtab.data() + g.ytab_off;
            for (int y = 1; y < g.h; y++)
                if (yt[4 * y] < yt[4 * (y - 1) + 1]) { plan.why = "resize rows do not advance"; return false; }
        }
        prev_w = g.w;
        prev_h = g.h;
    }
    if (!pyramid_tiles(plan)) return false;
    plan.pyr_frame_bytes = off;
    plan.slots_per_frame = slot_off;
    plan.keys_per_frame = key_off;
    plan.kept_per_frame = out_off;
    plan.tiles_total = tile_first;
    {
        // k_describe_tiles (switch desc_tiles = 1; measured slower than k_describe, DESIGN.md
        // section 4 item 5): k_octree bins each level's kept slots into its tiles with
        // NC-entry LDS counters and 16-bit list offsets
        const int NC = (plan.max_ncap + 63) & ~63;
        bool fits = true;
        for (int l = 0; l < plan.L; l++)
            fits = fits && plan.lv[l].tiles_x * plan.lv[l].tiles_y <= NC && plan.lv[l].ncap < 65536;
        plan.desc_tiles = fits && tuning(Tune::DescTiles, 0) == 1;
    }
    plan.rtab.resize(plan.rtab.size() + 64, 0);  // k_pyramid reads row taps in batches of 8 rows
    plan.ok = true;
    return true;
}

}  // namespace orbx
