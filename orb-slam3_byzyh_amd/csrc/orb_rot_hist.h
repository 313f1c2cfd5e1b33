// The matchers' rotation-consistency check (reference src/ORBmatcher.cc): the histogram bin of a
// match's angle difference and ComputeThreeMaxima (src:2336-2378), shared by SearchByProjection,
// SearchForTriangulation and SearchByBoW.
#pragma once
#include <hip/hip_runtime.h>

constexpr int kOrbHistoLength = 30;  // HISTO_LENGTH, src/ORBmatcher.cc:38

// rot = a1 - a2 (+360 when negative), bin = round(rot * factor) with the reference's
// factor = 1.0f / HISTO_LENGTH (kept as upstream has it), bin HISTO_LENGTH -> 0.
__device__ __forceinline__ int orb_rot_bin(float a1, float a2) {
    float rot = a1 - a2;
    if ((double)rot < 0.0) rot += 360.0f;
    int bin = (int)roundf(rot * (1.0f / kOrbHistoLength));
    if (bin == kOrbHistoLength) bin = 0;
    return bin;
}

// ComputeThreeMaxima on the bin counts: keep[0..2] = ind1, ind2, ind3 (-1: not kept).
__device__ __forceinline__ void orb_three_maxima(const int* hist, int* keep) {
    int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
    for (int i = 0; i < kOrbHistoLength; ++i) {
        const int s = hist[i];
        if (s > max1) {
            max3 = max2; max2 = max1; max1 = s;
            ind3 = ind2; ind2 = ind1; ind1 = i;
        } else if (s > max2) {
            max3 = max2; max2 = s;
            ind3 = ind2; ind2 = i;
        } else if (s > max3) {
            max3 = s; ind3 = i;
        }
    }
    if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if (max3 < 0.1f * (float)max1) ind3 = -1;
    keep[0] = ind1; keep[1] = ind2; keep[2] = ind3;
}
