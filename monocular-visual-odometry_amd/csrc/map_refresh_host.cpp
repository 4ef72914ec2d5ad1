// csrc/map_refresh_host.cpp -- host side of the map-point refresh (include/mvo_hip.h: mvo_map_refresh, mvo_debug_get_map):
// argument checks, one upload of the observation arrays, the launch, the results.  The kernel is in map_refresh_kernels.hip,
// the arithmetic in DESIGN.md section 17.  No other translation unit refers to this one: mvo_destroy reaches refresh_release
// through mvo_ctx::refresh_release.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "mvo_internal.h"

namespace {

void refresh_release(mvo_ctx* ctx) {
    delete ctx->refresh;
    ctx->refresh = nullptr;
}

int ensure_bufs(mvo_ctx* ctx, size_t bytes) {
    if (!ctx->refresh) {
        ctx->refresh = new mvo_refresh_state();
        ctx->refresh_release = refresh_release;
    }
    return ctx->refresh->d_in.ensure(ctx, bytes, (size_t)1 << 20);
}

inline size_t align64(size_t b) { return (b + 63) / 64 * 64; }

}  // namespace

extern "C" {

// ORB-SLAM's MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth on the resident map; the reference
// fills descriptor_ and norm_ once, in pushCurrPointsToMap_ (vo.cpp:528-576), and reads norm_ in getViewAngle_ (vo.cpp:578-584)
int mvo_map_refresh(mvo_ctx* ctx, mvo_map* map, const uint8_t* obs_desc, const double* obs_cam, const int32_t* obs_start, int n_obs,
                    int32_t* choice, uint8_t* desc_out, double* norm_out) {
    if (!ctx) return MVO_ERR_INVALID;
    auto invalid = [&](const char* what, int code = MVO_ERR_INVALID) {
        return mvo_set_err(ctx, code, (std::string("mvo_map_refresh: ") + what).c_str(), hipSuccess);
    };
    if (!map || n_obs < 0 || (n_obs && (!obs_desc || !obs_cam))) return invalid("bad arguments");
    const int n = map->n;
    if (n && (!obs_start || !choice || !norm_out)) return invalid("bad arguments");
    if (n == 0) return n_obs == 0 ? MVO_OK : invalid("observations of an empty map");
    if (obs_start[0] != 0 || obs_start[n] != n_obs) return invalid("obs_start does not span the observations");
    for (int i = 0; i < n; ++i)
        if (obs_start[i + 1] < obs_start[i]) return invalid("obs_start decreases");
    for (int i = 0; i < n; ++i)
        if (obs_start[i + 1] - obs_start[i] > MR_MAX_OBS) return invalid("more than 64 observations of a map point", MVO_ERR_CAPACITY);
    for (size_t k = 0; k < 3 * (size_t)n_obs; ++k)
        if (!std::isfinite(obs_cam[k])) return invalid("obs_cam is not finite");
    MVO_HIP(hipSetDevice(ctx->device));
    // pinned staging: the kernel writes normals, descriptors and choices straight into the first part; the second carries
    // the observation arrays up (one copy)
    const size_t norm_b = align64((size_t)n * 24), desc_b = align64((size_t)n * 32), out_bytes = norm_b + desc_b + align64((size_t)n * 4);
    const size_t cam_b = align64((size_t)n_obs * 24), odesc_b = align64((size_t)n_obs * 32), in_bytes = cam_b + odesc_b + ((size_t)n + 1) * 4;
    int r = ensure_bufs(ctx, in_bytes);
    if (r) return r;
    mvo_refresh_state* e = ctx->refresh;
    if ((r = mvo_ensure_pinned(ctx, out_bytes + in_bytes))) return r;
    MVO_HIP(hipStreamSynchronize(ctx->stream));  // (nothing of an earlier call may still be reading the staging buffer)
    uint8_t* h_in = ctx->h_pin + out_bytes;
    if (n_obs) {
        std::memcpy(h_in, obs_cam, (size_t)n_obs * 24);
        std::memcpy(h_in + cam_b, obs_desc, (size_t)n_obs * 32);
    }
    std::memcpy(h_in + cam_b + odesc_b, obs_start, ((size_t)n + 1) * 4);
    MVO_HIP(hipMemcpyAsync(e->d_in, h_in, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    double* h_norm = reinterpret_cast<double*>(ctx->h_pin);
    uint8_t* h_desc = ctx->h_pin + norm_b;
    int32_t* h_choice = reinterpret_cast<int32_t*>(ctx->h_pin + norm_b + desc_b);
    ExtractGate gate(ctx);
    if ((r = map_refresh_launch(ctx, map->d_pos, map->d_desc, n, e->d_in + cam_b, reinterpret_cast<const double*>(e->d_in.p),
                                reinterpret_cast<const int32_t*>(e->d_in + cam_b + odesc_b), h_choice, h_desc, h_norm)))
        return r;
    MVO_HIP(hipStreamSynchronize(ctx->stream));
    gate.release();
    if (ctx->prof) mvo_prof_collect(ctx);
    std::memcpy(choice, h_choice, (size_t)n * 4);
    std::memcpy(norm_out, h_norm, (size_t)n * 24);
    if (desc_out) std::memcpy(desc_out, h_desc, (size_t)n * 32);
    return MVO_OK;
}

// map.h:19 (Map::map_points_ of the resident copy): MapPoint::pos_ and descriptor_ as they lie in HBM, for tests
int mvo_debug_get_map(mvo_ctx* ctx, mvo_map* map, float* pos, uint8_t* desc, int cap, int* n) {
    if (!ctx) return MVO_ERR_INVALID;
    if (!map || !n || cap < 0) return mvo_set_err(ctx, MVO_ERR_INVALID, "mvo_debug_get_map: bad arguments", hipSuccess);
    *n = map->n;
    if (map->n > cap) return mvo_set_err(ctx, MVO_ERR_CAPACITY, "mvo_debug_get_map: buffer too small", hipSuccess);
    if (map->n == 0) return MVO_OK;
    MVO_HIP(hipSetDevice(ctx->device));
    MVO_HIP(hipStreamSynchronize(ctx->stream));
    if (pos) MVO_HIP(hipMemcpy(pos, map->d_pos, (size_t)map->n * 12, hipMemcpyDeviceToHost));
    if (desc) MVO_HIP(hipMemcpy(desc, map->d_desc, (size_t)map->n * 32, hipMemcpyDeviceToHost));
    return MVO_OK;
}

}  // extern "C"
