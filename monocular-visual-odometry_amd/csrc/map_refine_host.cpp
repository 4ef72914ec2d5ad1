// csrc/map_refine_host.cpp -- host side of the map-point position refinement (include/mvo_hip.h: mvo_map_refine_positions):
// argument checks, the pose inverses, one upload, the launch, the results.  The kernel is in map_refine_kernels.hip, the
// arithmetic in DESIGN.md section 18.  No other translation unit refers to this one.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "staged_call.h"

extern "C" {

// ORB-SLAM's structure-only refinement of every map point over all its observations; the reference triangulates a position once
// from two views and stores it (pushCurrPointsToMap_, vo.cpp:528-576) and its bundle adjustment keeps the points fixed
// (config.yaml:123)
int mvo_map_refine_positions(mvo_ctx* ctx, mvo_map* map, const double* T_w_c, int n_frames, double fx, double fy, double cx, double cy,
                             const int32_t* obs_frame, const float* obs_uv, const int32_t* obs_start, int n_obs,
                             const mvo_map_refine_params* params, float* pos_out, double* chi2, int32_t* info, uint8_t* obs_outlier) {
    if (!ctx) return MVO_ERR_INVALID;
    auto invalid = [&](const char* what, int code = MVO_ERR_INVALID) {
        return mvo_set_err(ctx, code, (std::string("mvo_map_refine_positions: ") + what).c_str(), hipSuccess);
    };
    if (!map || n_obs < 0 || n_frames < 0 || (n_obs && (!obs_frame || !obs_uv)) || (n_frames && !T_w_c)) return invalid("bad arguments");
    const int n = map->n;
    if (n && (!obs_start || !pos_out || !chi2 || !info)) return invalid("bad arguments");
    mvo_map_refine_params P{20, 2, std::sqrt(5.991), 1e-6};
    if (params) P = *params;
    if (P.max_trials < 1 || P.max_trials > 64 || P.min_observations < 2 || P.min_observations > MR_MAX_OBS || !(P.huber_delta > 0) ||
        !std::isfinite(P.huber_delta) || !(P.rel_tolerance >= 0) || !std::isfinite(P.rel_tolerance))
        return invalid("params out of range");
    if (fx == 0 || fy == 0 || !std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy))
        return invalid("fx or fy 0, or intrinsics not finite");
    if (n_frames > MF_MAX_FRAMES) return invalid("more than 64 frames", MVO_ERR_CAPACITY);
    std::vector<double> Tcw(12 * (size_t)n_frames);
    for (int f = 0; f < n_frames; ++f) {
        for (int k = 0; k < 16; ++k)
            if (!std::isfinite(T_w_c[16 * (size_t)f + k])) return invalid("T_w_c is not finite");
        double Ti[16];
        if (mvo_invert_pose(T_w_c + 16 * (size_t)f, Ti) != MVO_OK) return invalid("T_w_c is singular");
        std::memcpy(&Tcw[12 * (size_t)f], Ti, 12 * sizeof(double));
    }
    if (n == 0) return n_obs == 0 ? MVO_OK : invalid("observations of an empty map");
    if (obs_start[0] != 0 || obs_start[n] != n_obs) return invalid("obs_start does not span the observations");
    for (int i = 0; i < n; ++i)
        if (obs_start[i + 1] < obs_start[i]) return invalid("obs_start decreases");
    for (int i = 0; i < n; ++i)
        if (obs_start[i + 1] - obs_start[i] > MR_MAX_OBS) return invalid("more than 64 observations of a map point", MVO_ERR_CAPACITY);
    for (int k = 0; k < n_obs; ++k)
        if (obs_frame[k] < 0 || obs_frame[k] >= n_frames) return invalid("obs_frame outside [0, n_frames)");
    for (size_t k = 0; k < 2 * (size_t)n_obs; ++k)
        if (!std::isfinite(obs_uv[k])) return invalid("obs_uv is not finite");
    MapRefineArgs a;
    a.fx = fx, a.fy = fy, a.cx = cx, a.cy = cy;
    a.delta = P.huber_delta, a.rel_tol = P.rel_tolerance;
    a.max_trials = P.max_trials, a.min_obs = P.min_observations, a.n_frames = n_frames;
    // pinned staging: the kernel writes chi2, positions, info and flags straight into the first part; the second carries the
    // inverted poses and the observation arrays up (one copy)
    BlockCursor out, in;
    const size_t o_chi2 = out.block((size_t)n * 16), o_pos = out.block((size_t)n * 12), o_info = out.block((size_t)n * 12);
    const size_t o_flag = out.block((size_t)n_obs);
    const size_t i_T = in.block((size_t)n_frames * 96), i_uv = in.block((size_t)n_obs * 8), i_frame = in.block((size_t)n_obs * 4);
    const size_t i_start = in.last(((size_t)n + 1) * 4);
    mvo_refine_state* e = mvo_state(ctx->refine);
    StagedCall call{ctx};
    int r = call.begin(e->d_in, in.bytes, (size_t)1 << 20, out.bytes);
    if (r) return r;
    if (n_frames) std::memcpy(call.h_in + i_T, Tcw.data(), (size_t)n_frames * 96);
    if (n_obs) {
        std::memcpy(call.h_in + i_uv, obs_uv, (size_t)n_obs * 8);
        std::memcpy(call.h_in + i_frame, obs_frame, (size_t)n_obs * 4);
    }
    std::memcpy(call.h_in + i_start, obs_start, ((size_t)n + 1) * 4);
    if ((r = call.upload(e->d_in))) return r;
    double* h_chi2 = reinterpret_cast<double*>(call.h_out + o_chi2);
    float* h_pos = reinterpret_cast<float*>(call.h_out + o_pos);
    int32_t* h_info = reinterpret_cast<int32_t*>(call.h_out + o_info);
    uint8_t* h_flag = call.h_out + o_flag;
    ExtractGate gate(ctx);
    if ((r = map_refine_launch(ctx, map->d_pos, n, a, reinterpret_cast<const double*>(e->d_in + i_T),
                               reinterpret_cast<const float*>(e->d_in + i_uv), reinterpret_cast<const int32_t*>(e->d_in + i_frame),
                               reinterpret_cast<const int32_t*>(e->d_in + i_start), h_pos, h_chi2, h_info, h_flag)) ||
        (r = call.finish(gate)))
        return r;
    std::memcpy(pos_out, h_pos, (size_t)n * 12);
    std::memcpy(chi2, h_chi2, (size_t)n * 16);
    std::memcpy(info, h_info, (size_t)n * 12);
    if (obs_outlier && n_obs) std::memcpy(obs_outlier, h_flag, (size_t)n_obs);
    return MVO_OK;
}

}  // extern "C"
