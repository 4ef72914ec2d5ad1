// csrc/undistort_kernels.hip -- cv::undistort with newCameraMatrix = K (include/mvo_hip.h: mvo_undistort*), the step
// the reference runs over a dataset before run_vo sees it (python_tools/undistort_all_images.py:11-37).  Two kernels,
// the arithmetic of both declared in DESIGN.md section 13:
//   k_undistort_map    once per configuration: the distortion model in f64 per output pixel, rounded to the 1/32 px
//                      grid of initUndistortRectifyMap's fixed-point maps.  The only floating-point code of the feature.
//   k_undistort_remap  per frame: remap(INTER_LINEAR, BORDER_CONSTANT, 0) in integers from that map.
#include "mvo_internal.h"

#ifdef MVO_KERNEL_SIM
// v_cvt_i32_f64 under the default rounding mode: nearest even, saturating, NaN -> 0
static inline int __double2int_rn(double v) {
    if (!(v == v)) return 0;
    if (v >= 2147483647.0) return 2147483647;
    if (v <= -2147483648.0) return (-2147483647 - 1);
    return (int)lrint(v);
}
#endif

// One lane per output pixel p = i * w + j.  Every operation below is one IEEE f64 operation in the written order (the
// build has -ffp-contract=off; the quotient is hipcc's correctly rounded f64 division).
__global__ __launch_bounds__(256) void k_undistort_map(UndistortArgs a, int w, unsigned n, UndistortRec* __restrict__ map) {
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const int i = (int)(p / (unsigned)w), j = (int)(p - (unsigned)i * (unsigned)w);
    const double x = ((double)j - a.cx) * a.ifx, y = ((double)i - a.cy) * a.ify;
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, _2xy = 2 * x * y;
    const double kr = (1 + ((a.k3 * r2 + a.k2) * r2 + a.k1) * r2) / (1 + ((a.k6 * r2 + a.k5) * r2 + a.k4) * r2);
    const double u = a.fx * (x * kr + a.p1 * _2xy + a.p2 * (r2 + 2 * x2)) + a.cx;
    const double v = a.fy * (y * kr + a.p1 * (r2 + 2 * y2) + a.p2 * _2xy) + a.cy;
    UndistortRec rec;
    rec.iu = __double2int_rn(u * 32);
    rec.iv = __double2int_rn(v * 32);
    map[p] = rec;
}

// One lane per output pixel, all CH channels: the record is one coalesced 8-byte load, the four taps are plain byte
// loads (the distortion field is smooth: neighbouring lanes read neighbouring addresses).  A tap outside the source
// counts as 0 on its own; the weights are exact integers that sum to 32768.
template <int CH>
__global__ __launch_bounds__(256) void k_undistort_remap(const UndistortRec* __restrict__ map, const uint8_t* __restrict__ src,
                                                         int w, int h, int stride, unsigned n, uint8_t* __restrict__ out,
                                                         int out_stride) {
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const int i = (int)(p / (unsigned)w), j = (int)(p - (unsigned)i * (unsigned)w);
    const UndistortRec rec = map[p];
    const int ix = rec.iu >> 5, iy = rec.iv >> 5, ax = rec.iu & 31, ay = rec.iv & 31;
    const int w00 = 32 * (32 - ay) * (32 - ax), w01 = 32 * (32 - ay) * ax, w10 = 32 * ay * (32 - ax), w11 = 32 * ay * ax;
    // (ix + 1, iy + 1 cannot overflow: |iu >> 5| < 2^26)
    const bool x0 = ix >= 0 && ix < w, x1 = ix + 1 >= 0 && ix + 1 < w, y0 = iy >= 0 && iy < h, y1 = iy + 1 >= 0 && iy + 1 < h;
    uint8_t* o = out + (size_t)i * out_stride + (size_t)j * CH;
    if (x0 && x1 && y0 && y1) {
        const uint8_t* s0 = src + (size_t)iy * stride + (size_t)ix * CH;
        const uint8_t* s1 = s0 + stride;
#pragma unroll
        for (int c = 0; c < CH; ++c)
            o[c] = (uint8_t)((w00 * s0[c] + w01 * s0[CH + c] + w10 * s1[c] + w11 * s1[CH + c] + 16384) >> 15);
        return;
    }
    // the border: offsets are formed only for taps that are inside
    const size_t r0 = y0 ? (size_t)iy * stride : 0, r1 = y1 ? (size_t)(iy + 1) * stride : 0;
    const size_t c0 = x0 ? (size_t)ix * CH : 0, c1 = x1 ? (size_t)(ix + 1) * CH : 0;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const int p00 = y0 && x0 ? src[r0 + c0 + c] : 0, p01 = y0 && x1 ? src[r0 + c1 + c] : 0;
        const int p10 = y1 && x0 ? src[r1 + c0 + c] : 0, p11 = y1 && x1 ? src[r1 + c1 + c] : 0;
        o[c] = (uint8_t)((w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + 16384) >> 15);
    }
}

int undistort_launch_map(mvo_ctx* ctx, const UndistortArgs& a, int w, int h, UndistortRec* d_map) {
    const unsigned n = (unsigned)w * (unsigned)h;
    ProfScope ps(ctx, "k_undistort_map");
    hipLaunchKernelGGL(k_undistort_map, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, a, w, n, d_map);
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}

int undistort_launch_remap(mvo_ctx* ctx, const UndistortRec* d_map, const uint8_t* d_src, int w, int h, int stride,
                           int channels, uint8_t* d_out, int out_stride) {
    const unsigned n = (unsigned)w * (unsigned)h;
    const dim3 grid((n + 255u) / 256u), block(256);
    ProfScope ps(ctx, "k_undistort_remap");
    if (channels == 1)
        hipLaunchKernelGGL((k_undistort_remap<1>), grid, block, 0, ctx->stream, d_map, d_src, w, h, stride, n, d_out, out_stride);
    else if (channels == 3)
        hipLaunchKernelGGL((k_undistort_remap<3>), grid, block, 0, ctx->stream, d_map, d_src, w, h, stride, n, d_out, out_stride);
    else
        hipLaunchKernelGGL((k_undistort_remap<4>), grid, block, 0, ctx->stream, d_map, d_src, w, h, stride, n, d_out, out_stride);
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}
