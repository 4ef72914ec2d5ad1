// csrc/map_refresh_host.cpp -- host side of the map-point refresh (include/mvo_hip.h: mvo_map_refresh, mvo_debug_get_map):
// argument checks, one upload of the observation arrays, the launch, the results.  The kernel is in map_refresh_kernels.hip,
// the arithmetic in DESIGN.md section 17.  No other translation unit refers to this one.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "staged_call.h"

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
    // pinned staging: the kernel writes normals, descriptors and choices straight into the first part; the second carries
    // the observation arrays up (one copy)
    BlockCursor out, in;
    const size_t o_norm = out.block((size_t)n * 24), o_desc = out.block((size_t)n * 32), o_choice = out.block((size_t)n * 4);
    const size_t i_cam = in.block((size_t)n_obs * 24), i_desc = in.block((size_t)n_obs * 32), i_start = in.last(((size_t)n + 1) * 4);
    mvo_refresh_state* e = mvo_state(ctx->refresh);
    StagedCall call{ctx};
    int r = call.begin(e->d_in, in.bytes, (size_t)1 << 20, out.bytes);
    if (r) return r;
    if (n_obs) {
        std::memcpy(call.h_in + i_cam, obs_cam, (size_t)n_obs * 24);
        std::memcpy(call.h_in + i_desc, obs_desc, (size_t)n_obs * 32);
    }
    std::memcpy(call.h_in + i_start, obs_start, ((size_t)n + 1) * 4);
    if ((r = call.upload(e->d_in))) return r;
    double* h_norm = reinterpret_cast<double*>(call.h_out + o_norm);
    uint8_t* h_desc = call.h_out + o_desc;
    int32_t* h_choice = reinterpret_cast<int32_t*>(call.h_out + o_choice);
    ExtractGate gate(ctx);
    if ((r = map_refresh_launch(ctx, map->d_pos, map->d_desc, n, e->d_in + i_desc, reinterpret_cast<const double*>(e->d_in + i_cam),
                                reinterpret_cast<const int32_t*>(e->d_in + i_start), h_choice, h_desc, h_norm)) ||
        (r = call.finish(gate)))
        return r;
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
