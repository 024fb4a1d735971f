// The matchers' orientation check (mbCheckOrientation): the rotation bin of a match and
// ComputeThreeMaxima.  Device code; one home for every kernel that runs the check.
#pragma once

#include <hip/hip_runtime.h>

#include "orbx_match_types.h"

namespace orbx {

// rotHist bin of a match (ORBmatcher.cc:363-371): a1 / a2 the two keypoints' angles
__device__ __forceinline__ int rot_bin(float a1, float a2) {
    const float factor = kHistoLength / 360.0f;
    float rot = a1 - a2;
    if (rot < 0.0f) rot += 360.0f;
    int bin = (int)roundf(rot * factor);
    if (bin == kHistoLength) bin = 0;
    return bin;
}

// The bins a match may lie in to survive the check; -1: no such bin.
struct RotMaxima {
    int ind1, ind2, ind3;
    __device__ __forceinline__ bool keeps(int bin) const { return bin == ind1 || bin == ind2 || bin == ind3; }
};

// ComputeThreeMaxima, ORBmatcher.cc:1935-1977, on the kHistoLength bin counts h.  The
// result comes back in registers, so a caller whose threads each compute it (same counts,
// same result) needs neither LDS for it nor a barrier after it.
__device__ __forceinline__ RotMaxima three_maxima(const int* h) {
    int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
    for (int i = 0; i < kHistoLength; i++) {
        const int s = h[i];
        if (s > max1) {
            max3 = max2; max2 = max1; max1 = s;
            ind3 = ind2; ind2 = ind1; ind1 = i;
        } else if (s > max2) {
            max3 = max2; max2 = s;
            ind3 = ind2; ind2 = i;
        } else if (s > max3) {
            max3 = s;
            ind3 = i;
        }
    }
    if (max2 < 0.1f * (float)max1) {
        ind2 = -1;
        ind3 = -1;
    } else if (max3 < 0.1f * (float)max1) {
        ind3 = -1;
    }
    return RotMaxima{ind1, ind2, ind3};
}

}  // namespace orbx
