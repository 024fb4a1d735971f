// orbx_triangulate.hip -- LocalMapping::CreateNewMapPoints' second half (LocalMapping.cc:
// 307-501) over the vMatchedPairs that SearchForTriangulation left in HBM.
//
// k_triangulate_pairs: one 256-thread workgroup per keyframe pair p, one thread per matched
// pair (p, k), k < npairs[p], in chunks of 256.  A thread chooses the linear triangulation or a
// stereo back-projection by the parallax test (cc:341-393), applies the depth-sign, reprojection
// and scale-consistency tests (cc:395-476) and gives an accepted point its position, normal and
// distance range (MapPoint::UpdateNormalAndDepth with the two observations, MapPoint.cc:386-439).
//
// Arithmetic (the rule of 4.16): float inputs are widened to double, everything
// after is double, outputs are rounded to float once.  The only float operation is the
// reference's own float division mvDepth = mbf / (u - u_right) where the caller passes no depth
// array.  No floating-point value crosses lanes: a pair's bytes do not depend on the batch
// around it.  The counting (ballot, popcount, a four-entry LDS prefix) is integer only.
//
// The 4x4 SVD of the linear branch (orbx_jacobi4.h) is a one-sided (Hestenes) Jacobi on the columns
// of A with V accumulated from the identity, fully unrolled over 32 named doubles (no runtime-indexed
// array, so nothing goes to scratch): a sweep visits the six column pairs in the order (0,1)
// (0,2) (0,3) (1,2) (1,3) (2,3), a pair is rotated unless |a_i . a_j| <= 8 eps |a_i| |a_j|, the
// sweeps end with the first one that rotates nothing or after kSweepCap.  x3D is the column of
// V that belongs to the smallest column norm (ties: the higher index), divided by its 4th entry.
#include <hip/hip_runtime.h>

#include "orbx_jacobi4.h"
#include "orbx_kernels.h"

namespace orbx {

namespace {

constexpr int kTgThreads = 256;
constexpr int kTgWaves = kTgThreads / 64;

struct TgPoint {
    int reason, method;
    double X, Y, Z, nx, ny, nz, dmax, dmin;
};

// mvDepth of keypoint i: the caller's array, or mbf / (mvKeys[i].pt.x - mvuRight[i]) in float,
// as ComputeStereoMatches derived it (Frame.cc:852-856)
__device__ __forceinline__ double depth_of(const TriGeomKF& K, const orbx_keypoint* keys, int i, float ur, float mbf) {
    if (K.depth) return (double)K.depth[i];
    return (double)(mbf / (keys[i].x - ur));
}

__device__ __forceinline__ int clamp_octave(int o, int nlevels) { return o < 0 ? 0 : (o >= nlevels ? nlevels - 1 : o); }

__device__ TgPoint triangulate_one(const TriGeomArgs& A, const TriGeomKF& K1, const TriGeomKF& K2, int idx1, int idx2) {
    TgPoint r{};
    r.reason = 9;
    int n1 = *K1.n, n2 = *K2.n;
    n1 = n1 < 0 ? 0 : (n1 > A.kcap ? A.kcap : n1);
    n2 = n2 < 0 ? 0 : (n2 > A.kcap ? A.kcap : n2);
    if (idx1 < 0 || idx1 >= n1 || idx2 < 0 || idx2 >= n2) return r;
    const orbx_keypoint* raw1 = K1.keys ? K1.keys : K1.keys_un;
    const orbx_keypoint* raw2 = K2.keys ? K2.keys : K2.keys_un;
    const orbx_keypoint kp1 = K1.keys_un[idx1], kp2 = K2.keys_un[idx2];
    const float ur1f = K1.u_right ? K1.u_right[idx1] : -1.0f, ur2f = K2.u_right ? K2.u_right[idx2] : -1.0f;
    const bool st1 = ur1f >= 0.0f, st2 = ur2f >= 0.0f;  // cc:331-338
    const double fx = A.fx, fy = A.fy, cx = A.cx, cy = A.cy;
    const double invfx = 1.0 / fx, invfy = 1.0 / fy;
    const double u1 = kp1.x, v1 = kp1.y, u2 = kp2.x, v2 = kp2.y;
    const double R100 = K1.Tcw[0], R101 = K1.Tcw[1], R102 = K1.Tcw[2], t10 = K1.Tcw[3];
    const double R110 = K1.Tcw[4], R111 = K1.Tcw[5], R112 = K1.Tcw[6], t11 = K1.Tcw[7];
    const double R120 = K1.Tcw[8], R121 = K1.Tcw[9], R122 = K1.Tcw[10], t12 = K1.Tcw[11];
    const double R200 = K2.Tcw[0], R201 = K2.Tcw[1], R202 = K2.Tcw[2], t20 = K2.Tcw[3];
    const double R210 = K2.Tcw[4], R211 = K2.Tcw[5], R212 = K2.Tcw[6], t21 = K2.Tcw[7];
    const double R220 = K2.Tcw[8], R221 = K2.Tcw[9], R222 = K2.Tcw[10], t22 = K2.Tcw[11];
    // cc:341-348
    const double xa = (u1 - cx) * invfx, ya = (v1 - cy) * invfy;
    const double xb = (u2 - cx) * invfx, yb = (v2 - cy) * invfy;
    const double ra0 = (R100 * xa + R110 * ya) + R120, ra1 = (R101 * xa + R111 * ya) + R121,
                 ra2 = (R102 * xa + R112 * ya) + R122;
    const double rb0 = (R200 * xb + R210 * yb) + R220, rb1 = (R201 * xb + R211 * yb) + R221,
                 rb2 = (R202 * xb + R212 * yb) + R222;
    const double cos_rays = ((ra0 * rb0 + ra1 * rb1) + ra2 * rb2) /
                            (sqrt((ra0 * ra0 + ra1 * ra1) + ra2 * ra2) * sqrt((rb0 * rb0 + rb1 * rb1) + rb2 * rb2));
    // cc:351-363: cos(2 atan2(mb / 2, depth)) = (d^2 - a^2) / (d^2 + a^2); the `else if` is the reference's
    double cs1 = cos_rays + 1.0, cs2 = cos_rays + 1.0;
    const double a = (double)A.mb / 2.0;
    double d1 = 0.0, d2 = 0.0;
    if (st1) d1 = depth_of(K1, raw1, idx1, ur1f, A.mbf);
    if (st2) d2 = depth_of(K2, raw2, idx2, ur2f, A.mbf);
    if (st1) cs1 = (d1 * d1 - a * a) / (d1 * d1 + a * a);
    else if (st2) cs2 = (d2 * d2 - a * a) / (d2 * d2 + a * a);
    const double cs = cs2 < cs1 ? cs2 : cs1;  // std::min(cs1, cs2)
    double X, Y, Z;
    if (cos_rays < cs && cos_rays > 0.0 && (st1 || st2 || cos_rays < 0.9998)) {
        r.method = 1;
        double h0, h1, h2, h3;
        smallest_right_singular_vector(  // cc:374-377
            xa * R120 - R100, xa * R121 - R101, xa * R122 - R102, xa * t12 - t10,
            ya * R120 - R110, ya * R121 - R111, ya * R122 - R112, ya * t12 - t11,
            xb * R220 - R200, xb * R221 - R201, xb * R222 - R202, xb * t22 - t20,
            yb * R220 - R210, yb * R221 - R211, yb * R222 - R212, yb * t22 - t21, h0, h1, h2, h3);
        if (h3 == 0.0) {
            r.reason = 2;
            return r;
        }
        X = h0 / h3;
        Y = h1 / h3;
        Z = h2 / h3;
    } else if (st1 && cs1 < cs2 && d1 > 0.0) {  // KeyFrame::UnprojectStereo(idx1): mvKeys, mvDepth, Twc
        r.method = 2;
        const double uu = raw1[idx1].x, vv = raw1[idx1].y;
        const double xc = (uu - cx) * d1 * invfx, yc = (vv - cy) * d1 * invfy;
        X = ((R100 * xc + R110 * yc) + R120 * d1) + K1.Ow[0];
        Y = ((R101 * xc + R111 * yc) + R121 * d1) + K1.Ow[1];
        Z = ((R102 * xc + R112 * yc) + R122 * d1) + K1.Ow[2];
    } else if (!(st1 && cs1 < cs2) && st2 && cs2 < cs1 && d2 > 0.0) {
        r.method = 3;
        const double uu = raw2[idx2].x, vv = raw2[idx2].y;
        const double xc = (uu - cx) * d2 * invfx, yc = (vv - cy) * d2 * invfy;
        X = ((R200 * xc + R210 * yc) + R220 * d2) + K2.Ow[0];
        Y = ((R201 * xc + R211 * yc) + R221 * d2) + K2.Ow[1];
        Z = ((R202 * xc + R212 * yc) + R222 * d2) + K2.Ow[2];
    } else {
        r.reason = 1;  // no stereo and very low parallax (or a stereo point whose mvDepth is not positive)
        return r;
    }
    const double z1 = ((R120 * X + R121 * Y) + R122 * Z) + t12;
    if (z1 <= 0.0) {
        r.reason = 3;
        return r;
    }
    const double z2 = ((R220 * X + R221 * Y) + R222 * Z) + t22;
    if (z2 <= 0.0) {
        r.reason = 4;
        return r;
    }
    const int o1 = clamp_octave(kp1.octave, A.nlevels), o2 = clamp_octave(kp2.octave, A.nlevels);
    const double mbf = A.mbf;
    {  // cc:407-430
        const double sig = A.sigma2[o1];
        const double x1 = ((R100 * X + R101 * Y) + R102 * Z) + t10, y1 = ((R110 * X + R111 * Y) + R112 * Z) + t11;
        const double invz = 1.0 / z1;
        const double pu = fx * x1 * invz + cx, pv = fy * y1 * invz + cy;
        const double ex = pu - u1, ey = pv - v1;
        if (!st1) {
            if (ex * ex + ey * ey > 5.991 * sig) r.reason = 5;
        } else {
            const double er = (pu - mbf * invz) - (double)ur1f;
            if ((ex * ex + ey * ey) + er * er > 7.8 * sig) r.reason = 5;
        }
        if (r.reason == 5) return r;
    }
    {  // cc:433-454; KF2's stereo test uses KF1's mbf (cc:446): the call has one mbf
        const double sig = A.sigma2[o2];
        const double x2 = ((R200 * X + R201 * Y) + R202 * Z) + t20, y2 = ((R210 * X + R211 * Y) + R212 * Z) + t21;
        const double invz = 1.0 / z2;
        const double pu = fx * x2 * invz + cx, pv = fy * y2 * invz + cy;
        const double ex = pu - u2, ey = pv - v2;
        if (!st2) {
            if (ex * ex + ey * ey > 5.991 * sig) r.reason = 6;
        } else {
            const double er = (pu - mbf * invz) - (double)ur2f;
            if ((ex * ex + ey * ey) + er * er > 7.8 * sig) r.reason = 6;
        }
        if (r.reason == 6) return r;
    }
    // cc:458-476
    const double na0 = X - K1.Ow[0], na1 = Y - K1.Ow[1], na2 = Z - K1.Ow[2];
    const double nb0 = X - K2.Ow[0], nb1 = Y - K2.Ow[1], nb2 = Z - K2.Ow[2];
    const double dist1 = sqrt((na0 * na0 + na1 * na1) + na2 * na2), dist2 = sqrt((nb0 * nb0 + nb1 * nb1) + nb2 * nb2);
    if (dist1 == 0.0 || dist2 == 0.0) {
        r.reason = 7;
        return r;
    }
    const double ratio_dist = dist2 / dist1;
    const double ratio_octave = (double)A.scale[o1] / (double)A.scale[o2];
    const double ratio_factor = 1.5 * (double)A.scale_factor;
    if (ratio_dist * ratio_factor < ratio_octave || ratio_dist > ratio_octave * ratio_factor) {
        r.reason = 8;
        return r;
    }
    // MapPoint::UpdateNormalAndDepth, observations {KF1, KF2}, reference KF1 (MapPoint.cc:404-437)
    r.reason = 0;
    r.X = X;
    r.Y = Y;
    r.Z = Z;
    r.nx = (na0 / dist1 + nb0 / dist2) / 2.0;
    r.ny = (na1 / dist1 + nb1 / dist2) / 2.0;
    r.nz = (na2 / dist1 + nb2 / dist2) / 2.0;
    r.dmax = dist1 * (double)A.scale[o1];
    r.dmin = r.dmax / (double)A.scale[A.nlevels - 1];
    return r;
}

__global__ __launch_bounds__(kTgThreads) void k_triangulate_pairs(TriGeomArgs A) {
    __shared__ int s_cnt[kTgWaves];
    const int p = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int np = A.npairs[p];
    np = np < 0 ? 0 : (np > A.cap ? A.cap : np);
    const TriGeomKF& K1 = A.kfs[A.pair_kf[2 * p]];
    const TriGeomKF& K2 = A.kfs[A.pair_kf[2 * p + 1]];
    const size_t row = (size_t)p * A.cap;
    int base_new = 0;
    for (int k0 = 0; k0 < np; k0 += kTgThreads) {  // uniform over the workgroup
        const int k = k0 + tid;
        bool ok = false;
        if (k < np) {
            const size_t s = row + k;
            const TgPoint r = triangulate_one(A, K1, K2, A.pairs[2 * s], A.pairs[2 * s + 1]);
            ok = r.reason == 0;
            if (A.reason) A.reason[s] = (uint8_t)r.reason;
            if (A.method) A.method[s] = (uint8_t)r.method;
            if (A.pos) {
                A.pos[3 * s] = (float)r.X;
                A.pos[3 * s + 1] = (float)r.Y;
                A.pos[3 * s + 2] = (float)r.Z;
            }
            if (A.normal) {
                A.normal[3 * s] = (float)r.nx;
                A.normal[3 * s + 1] = (float)r.ny;
                A.normal[3 * s + 2] = (float)r.nz;
            }
            if (A.max_distance) A.max_distance[s] = (float)r.dmax;
            if (A.min_distance) A.min_distance[s] = (float)r.dmin;
        }
        // accepted slots in pair order: ballot within the wave, a prefix over the four waves
        const unsigned long long b = __ballot(ok);
        if (lane == 0) s_cnt[wave] = __popcll(b);
        __syncthreads();
        int before = base_new, total = 0;
        for (int w = 0; w < kTgWaves; w++) {
            const int c = s_cnt[w];
            if (w < wave) before += c;
            total += c;
        }
        if (ok && A.new_idx) A.new_idx[row + before + __popcll(b & ((1ull << lane) - 1ull))] = k;
        base_new += total;
        __syncthreads();
    }
    if (tid == 0 && A.nnew) A.nnew[p] = base_new;
}

}  // namespace

hipError_t launch_triangulate_pairs(const TriGeomArgs& A, int npairs, hipStream_t stream) {
    if (npairs <= 0) return hipSuccess;
    k_triangulate_pairs<<<npairs, kTgThreads, 0, stream>>>(A);
    return hipGetLastError();
}

}  // namespace orbx
