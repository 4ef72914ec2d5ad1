// csrc/undistort_host.cpp -- host side of the undistortion (include/mvo_hip.h: mvo_undistort_configure, mvo_undistort,
// mvo_undistort_dev, mvo_debug_get_undistort_map): argument checks, the cached map of a configuration, the staging of
// the host-pointer form.  The kernels are in undistort_kernels.hip, the arithmetic in DESIGN.md section 13.  No other
// translation unit refers to this one.
#include <cmath>
#include <cstring>
#include <vector>

#include "mvo_internal.h"

namespace {

const int kMaxWidth = 8192;            // as the extraction (FT_ROW_TILES)
const long long kMaxPixels = 1 << 30;  // pixel indices are 32-bit in the kernels, the debug getter counts in int

// the parameters as they are compared and used: coefficients beyond n_coeffs are 0.  false: not a supported model
bool normalise(const mvo_undistort_params& in, mvo_undistort_params* out) {
    if (in.n_coeffs != 4 && in.n_coeffs != 5 && in.n_coeffs != 8) return false;
    std::memset(out, 0, sizeof *out);  // (padding bytes too: configurations are compared with memcmp)
    out->fx = in.fx, out->fy = in.fy, out->cx = in.cx, out->cy = in.cy;
    out->n_coeffs = in.n_coeffs;
    for (int k = 0; k < in.n_coeffs; ++k) out->coeffs[k] = in.coeffs[k];
    const double all[4] = {in.fx, in.fy, in.cx, in.cy};
    for (double v : all)
        if (!std::isfinite(v)) return false;
    for (double v : out->coeffs)
        if (!std::isfinite(v)) return false;
    return in.fx != 0 && in.fy != 0;
}

int check_call(mvo_ctx* ctx, const void* img, int w, int h, int stride, int ch, const void* out, int out_stride) {
    if (!ctx) return MVO_ERR_INVALID;
    if (!img || !out || w < 1 || h < 1 || w > kMaxWidth || (ch != 1 && ch != 3 && ch != 4) || stride < w * ch || out_stride < w * ch)
        return mvo_set_err(ctx, MVO_ERR_INVALID, "mvo_undistort: bad image arguments", hipSuccess);
    const mvo_undistort_state* u = ctx->undist.get();
    if (!u || !u->configured)
        return mvo_set_err(ctx, MVO_ERR_STATE, "mvo_undistort before mvo_undistort_configure", hipSuccess);
    if (u->w != w || u->h != h)
        return mvo_set_err(ctx, MVO_ERR_STATE, "mvo_undistort: image size differs from the configured one", hipSuccess);
    return MVO_OK;
}

// bytes of an h-row image from its first to its last pixel
size_t extent(int w, int h, int stride, int ch) { return (size_t)(h - 1) * stride + (size_t)w * ch; }

}  // namespace

extern "C" {

int mvo_undistort_configure(mvo_ctx* ctx, const mvo_undistort_params* params, int width, int height) {
    if (!ctx) return MVO_ERR_INVALID;
    mvo_undistort_params p;
    if (!params || !normalise(*params, &p))
        return mvo_set_err(ctx, MVO_ERR_INVALID, "mvo_undistort_configure: 4, 5 or 8 finite coefficients, fx and fy non-zero", hipSuccess);
    if (width < 1 || height < 1 || width > kMaxWidth || (long long)width * height > kMaxPixels)
        return mvo_set_err(ctx, MVO_ERR_INVALID, "mvo_undistort_configure: image size out of range", hipSuccess);
    MVO_HIP(hipSetDevice(ctx->device));
    mvo_undistort_state* u = mvo_state(ctx->undist);
    if (u->configured && u->w == width && u->h == height && !std::memcmp(&u->params, &p, sizeof p)) return MVO_OK;
    u->configured = false;
    int r = u->d_map.ensure_exact(ctx, (size_t)width * height, 64);
    if (r) return r;
    const double* k = p.coeffs;
    const UndistortArgs a{p.fx, p.fy, p.cx, p.cy, 1.0 / p.fx, 1.0 / p.fy, k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7]};
    if ((r = undistort_launch_map(ctx, a, width, height, u->d_map))) return r;
    if (ctx->prof) mvo_prof_collect(ctx);
    u->params = p;
    u->w = width, u->h = height;
    u->configured = true;
    return MVO_OK;
}

int mvo_undistort_dev(mvo_ctx* ctx, const void* d_image, int w, int h, int stride, int ch, void* d_out, int out_stride) {
    int r = check_call(ctx, d_image, w, h, stride, ch, d_out, out_stride);
    if (r) return r;
    const uintptr_t s = (uintptr_t)d_image, o = (uintptr_t)d_out;
    if (s < o + extent(w, h, out_stride, ch) && o < s + extent(w, h, stride, ch))
        return mvo_set_err(ctx, MVO_ERR_INVALID, "mvo_undistort_dev: d_out overlaps d_image", hipSuccess);
    MVO_HIP(hipSetDevice(ctx->device));
    if ((r = undistort_launch_remap(ctx, ctx->undist->d_map, (const uint8_t*)d_image, w, h, stride, ch, (uint8_t*)d_out, out_stride))) return r;
    if (ctx->prof) mvo_prof_collect(ctx);
    return MVO_OK;
}

int mvo_undistort(mvo_ctx* ctx, const uint8_t* image, int w, int h, int stride, int ch, uint8_t* out, int out_stride) {
    int r = check_call(ctx, image, w, h, stride, ch, out, out_stride);
    if (r) return r;
    MVO_HIP(hipSetDevice(ctx->device));
    mvo_undistort_state* u = ctx->undist.get();
    const size_t in_bytes = extent(w, h, stride, ch), row = (size_t)w * ch;
    if ((r = u->d_src.ensure_exact(ctx, in_bytes, 64))) return r;
    if ((r = u->d_dst.ensure_exact(ctx, row * h, 64))) return r;
    MVO_HIP(hipMemcpyAsync(u->d_src, image, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    if ((r = undistort_launch_remap(ctx, u->d_map, u->d_src, w, h, stride, ch, u->d_dst, (int)row))) return r;
    // the device image is packed; the caller's padding between rows is never written
    if ((size_t)out_stride == row) {
        MVO_HIP(hipMemcpyAsync(out, u->d_dst, row * h, hipMemcpyDeviceToHost, ctx->stream));
        MVO_HIP(hipStreamSynchronize(ctx->stream));
    } else {
        std::vector<uint8_t> packed(row * h);
        MVO_HIP(hipMemcpyAsync(packed.data(), u->d_dst, row * h, hipMemcpyDeviceToHost, ctx->stream));
        MVO_HIP(hipStreamSynchronize(ctx->stream));
        for (int i = 0; i < h; ++i) std::memcpy(out + (size_t)i * out_stride, packed.data() + (size_t)i * row, row);
    }
    if (ctx->prof) mvo_prof_collect(ctx);
    return MVO_OK;
}

int mvo_debug_get_undistort_map(mvo_ctx* ctx, int32_t* ix, int32_t* iy, uint8_t* ax, uint8_t* ay, int cap) {
    if (!ctx) return MVO_ERR_INVALID;
    const mvo_undistort_state* u = ctx->undist.get();
    if (!u || !u->configured) return mvo_set_err(ctx, MVO_ERR_STATE, "no undistortion map: call mvo_undistort_configure first", hipSuccess);
    const size_t n = (size_t)u->w * u->h;
    if (cap < 0 || (size_t)cap < n) return mvo_set_err(ctx, MVO_ERR_CAPACITY, "undistortion map buffer too small", hipSuccess);
    MVO_HIP(hipSetDevice(ctx->device));
    std::vector<UndistortRec> rec(n);
    MVO_HIP(hipMemcpyAsync(rec.data(), u->d_map, n * sizeof(UndistortRec), hipMemcpyDeviceToHost, ctx->stream));
    MVO_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t p = 0; p < n; ++p) {
        if (ix) ix[p] = rec[p].iu >> 5;
        if (iy) iy[p] = rec[p].iv >> 5;
        if (ax) ax[p] = (uint8_t)(rec[p].iu & 31);
        if (ay) ay[p] = (uint8_t)(rec[p].iv & 31);
    }
    return MVO_OK;
}

}  // extern "C"
