// epnp_host -- csrc/orbx_epnp.h compiled for the host, driven over stdin / stdout in binary, so
// that tests/test_pnp_model.py can compare it bit for bit with the float64 model.
//
//   epnp_host pose    < i32 n, f64 fu fv uc vc, f64 pws[3n], f64 us[2n]   > f64 R[9] t[3] err
//   epnp_host inlier  < f64 R[9] t[3], f64 fu fv uc vc, i32 m, f32 (X Y Z u v max)[m]  > u8 [m]
//   epnp_host jacobi  < i32 rows, i32 n, f64 a[rows * n]   > f64 b[rows * n] v[n * n]
//   epnp_host qr      < f64 a[24] b[6] x[4]   > f64 x[4]
//
// Build with -ffp-contract=off.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbx_epnp.h"

using namespace orbx::epnp;

static bool rd(void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, stdin) == bytes; }
static void wr(const void* p, size_t bytes) { fwrite(p, 1, bytes, stdout); }

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    if (!strcmp(argv[1], "pose")) {
        int32_t n;
        Camera K;
        if (!rd(&n, 4) || n < 1 || !rd(&K, 32)) return 1;
        std::vector<double> pws(3 * (size_t)n), us(2 * (size_t)n), alphas(4 * (size_t)n), pcs(3 * (size_t)n), W(kWork);
        if (!rd(pws.data(), pws.size() * 8) || !rd(us.data(), us.size() * 8)) return 1;
        double out[13];
        out[12] = compute_pose(n, Mem{pws.data(), 1}, Mem{us.data(), 1}, Mem{alphas.data(), 1}, Mem{pcs.data(), 1},
                               Mem{W.data(), 1}, K, out, out + 9);
        wr(out, sizeof(out));
        return 0;
    }
    if (!strcmp(argv[1], "inlier")) {
        double P[12];
        Camera K;
        int32_t m;
        if (!rd(P, 96) || !rd(&K, 32) || !rd(&m, 4) || m < 0) return 1;
        std::vector<float> pts(6 * (size_t)m);
        if (!rd(pts.data(), pts.size() * 4)) return 1;
        std::vector<uint8_t> f((size_t)m);
        for (int i = 0; i < m; i++) {
            const float* p = &pts[6 * (size_t)i];
            f[i] = check_inlier(P, P + 9, K, p[0], p[1], p[2], p[3], p[4], p[5]) ? 1 : 0;
        }
        wr(f.data(), f.size());
        return 0;
    }
    if (!strcmp(argv[1], "jacobi")) {
        int32_t rows, n;
        if (!rd(&rows, 4) || !rd(&n, 4) || rows < 1 || n < 1 || n > 12 || rows > 12) return 1;
        std::vector<double> a((size_t)rows * n), v((size_t)n * n);
        if (!rd(a.data(), a.size() * 8)) return 1;
        hestenes(Mem{a.data(), 1}, Mem{v.data(), 1}, rows, n);
        wr(a.data(), a.size() * 8);
        wr(v.data(), v.size() * 8);
        return 0;
    }
    if (!strcmp(argv[1], "qr")) {
        double a[24], b[6], x[4];
        if (!rd(a, sizeof(a)) || !rd(b, sizeof(b)) || !rd(x, sizeof(x))) return 1;
        qr_solve_6x4(a, b, x);
        wr(x, sizeof(x));
        return 0;
    }
    return 2;
}
