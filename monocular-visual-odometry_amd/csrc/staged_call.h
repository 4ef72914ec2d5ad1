// csrc/staged_call.h -- the one-upload, one-launch, one-wait call through the ctx's pinned staging buffer, as the host sides of
// the map-maintenance and tracking calls make it (map_refresh, map_refine, map_fuse, window_triangulate, pose_optimize): the
// kernel writes its results straight into the first out_bytes of ctx->h_pin, the part behind them carries the inputs up in one
// copy into the call's own device buffer.  Inline, no translation unit of its own.
#ifndef MVO_STAGED_CALL_H
#define MVO_STAGED_CALL_H
#include "mvo_internal.h"

inline size_t align64(size_t b) { return (b + 63) / 64 * 64; }

// The byte offsets of consecutive blocks: a layout is written once, in order, and read by the names the offsets are given.
// Every block starts on a multiple of 64; the last one of an upload is taken with last() and adds no padding behind it.
struct BlockCursor {
    size_t bytes = 0;  // of the blocks handed out so far
    size_t block(size_t b) { return last(align64(b)); }
    size_t last(size_t b) {
        const size_t off = bytes;
        bytes += b;
        return off;
    }
};

struct StagedCall {
    mvo_ctx* ctx;
    uint8_t *h_out = nullptr, *h_in = nullptr;  // the two parts of ctx->h_pin
    size_t in_bytes = 0;

    // room in the pinned buffer alone: for a second phase on a stream the first has left idle
    int stage(size_t out_bytes, size_t in_bytes_) {
        if (int r = mvo_ensure_pinned(ctx, out_bytes + in_bytes_)) return r;
        h_out = ctx->h_pin, h_in = ctx->h_pin + out_bytes, in_bytes = in_bytes_;
        return MVO_OK;
    }
    // the device made current, d_in grown to in_bytes (max(floor, 1.5 in_bytes) when it grows), also(): the call's further
    // device buffers, the pinned buffer grown, the stream idle: h_in may be filled
    template <class Also>
    int begin(DevBuf<uint8_t>& d_in, size_t in_bytes_, size_t floor, size_t out_bytes, Also also) {
        MVO_HIP(hipSetDevice(ctx->device));
        int r;
        if ((r = d_in.ensure(ctx, in_bytes_, floor)) || (r = also()) || (r = stage(out_bytes, in_bytes_))) return r;
        MVO_HIP(hipStreamSynchronize(ctx->stream));  // (nothing of an earlier call may still be reading the staging buffer)
        return MVO_OK;
    }
    int begin(DevBuf<uint8_t>& d_in, size_t in_bytes_, size_t floor, size_t out_bytes) {
        return begin(d_in, in_bytes_, floor, out_bytes, [] { return (int)MVO_OK; });
    }
    int upload(void* d_in) {  // the one copy
        MVO_HIP(hipMemcpyAsync(d_in, h_in, in_bytes, hipMemcpyHostToDevice, ctx->stream));
        return MVO_OK;
    }
    // behind the launch: the wait, the admission gate given back, the profile.  The results lie in h_out.
    int finish(ExtractGate& gate) {
        MVO_HIP(hipStreamSynchronize(ctx->stream));
        gate.release();
        if (ctx->prof) mvo_prof_collect(ctx);
        return MVO_OK;
    }
};

#endif
