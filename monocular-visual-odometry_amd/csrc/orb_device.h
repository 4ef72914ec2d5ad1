// csrc/orb_device.h -- device helpers shared by the two detectors (orb_kernels.hip: k_fast_harris; orb_distribute_kernels.hip:
// k_fast_cells, k_ic_angle): the FAST-9/16 quick test and score, cv::fastAtan2 and the integer wave sum.  One statement of each, so
// that both detectors score and orient a pixel with the same instructions.
#ifndef MVO_ORB_DEVICE_H
#define MVO_ORB_DEVICE_H
#include <cfloat>
#include <cmath>

#include "mvo_internal.h"

// cornerScore<16> in two halves.  d[k] = centre - circle[k].
// fast_quick_test: can the pixel be a FAST-9 corner at threshold thr at all?  (bit masks of the circle pixels darker / brighter
// than the centre by more than thr; nine consecutive set bits in either)
__device__ __forceinline__ bool fast_quick_test(const int (&d)[16], int thr) {
    uint32_t dark = 0, bright = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        dark |= (uint32_t)(d[k] > thr) << k;
        bright |= (uint32_t)(d[k] < -thr) << k;
    }
    auto has9 = [](uint32_t m) {
        uint32_t x = m | (m << 16);
        uint32_t a = x & (x >> 1);
        uint32_t b = a & (a >> 2);
        uint32_t c = b & (b >> 4);
        return (c & (x >> 8) & 0xffffu) != 0;
    };
    return has9(dark) || has9(bright);
}
// fast_score_full: the largest threshold for which the pixel is still a FAST-9 corner (for a pixel that passed the quick test):
// max over the 16 arcs of 9 consecutive circle pixels of min(d) and of min(-d), by a sliding minimum / maximum with doubling.
__device__ __forceinline__ int fast_score_full(const int (&d)[16], int thr) {
    int mn2[16], mx2[16], mn4[16], mx4[16], mn8[16], mx8[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        mn2[k] = min(d[k], d[(k + 1) & 15]);
        mx2[k] = max(d[k], d[(k + 1) & 15]);
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        mn4[k] = min(mn2[k], mn2[(k + 2) & 15]);
        mx4[k] = max(mx2[k], mx2[(k + 2) & 15]);
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        mn8[k] = min(mn4[k], mn4[(k + 4) & 15]);
        mx8[k] = max(mx4[k], mx4[(k + 4) & 15]);
    }
    int A = -256, B = -256;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        A = max(A, min(mn8[k], d[(k + 8) & 15]));
        B = max(B, -max(mx8[k], d[(k + 8) & 15]));
    }
    int best = max(A, B);
    return best > thr ? best - 1 : 0;
}

// cv::fastAtan2 (degrees)
__device__ __forceinline__ float fast_atan2_deg(float y, float x) {
    const float p1 = 0.9997878412794807f * (float)(180 / M_PI);
    const float p3 = -0.3258083974640975f * (float)(180 / M_PI);
    const float p5 = 0.1555786518463281f * (float)(180 / M_PI);
    const float p7 = -0.04432655554792128f * (float)(180 / M_PI);
    float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        c = ay / (ax + (float)DBL_EPSILON);
        c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        c = ax / (ay + (float)DBL_EPSILON);
        c2 = c * c;
        a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

__device__ __forceinline__ int wave_sum(int v) {
#ifndef MVO_KERNEL_SIM
    // Inclusive scan inside each row of 16 lanes by DPP row shifts (a lane outside the row contributes 0), then the row totals
    // are carried over by the two row broadcasts: lane 63 holds the sum of the wave and is read back as a scalar.  Six VALU
    // instructions instead of six ds_bpermute round trips (each ~60 cycles of dependent latency: five sums per survivor were the
    // longest chain of the survivor phase).  Integer adds: the order does not matter.
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);  // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);  // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);  // row_shr:8   -> lane 15 of every row: the row's total
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2 and 3 -> lane 63: the total
    return __builtin_amdgcn_readlane(v, 63);
#else
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
#endif
}

#endif
