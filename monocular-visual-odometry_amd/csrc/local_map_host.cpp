// csrc/local_map_host.cpp -- host side of tracking the local map (include/mvo_hip.h: mvo_map_upload_view,
// mvo_map_match_knn2_local, mvo_map_match_knn2_local_dev, mvo_map_match_features_local): the view data of the resident map,
// argument checks, the one upload (parked keypoints, skip mask, descriptors), ORB-SLAM's acceptance rule and the
// one-point-per-keypoint rule.  The kernel is in local_map_kernels.hip, the arithmetic in DESIGN.md section 22.  No other
// translation unit refers to this one.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "guided_match_host.h"

namespace {

const mvo_local_map_params kDefaults = {0.5, 2.5, 4.0, 0.998, 1.0, 0.8, 100, 0};

// Every form: the checks, the upload, the launch, the results.  t is a host pointer (t_on_device false) or a device pointer.
int run(mvo_ctx* ctx, mvo_map* map, const double* T_w_c, double fx, double fy, double cx, double cy, int cols, int rows,
        const void* t, bool t_on_device, const float* txy, const int32_t* t_level, int nt, const uint8_t* skip,
        const double* level_scale, int n_levels, const mvo_local_map_params* params, float* px, int32_t* idx, int32_t* dist,
        int32_t* n_candidates, int32_t* level, double* view_cos, const char* who) {
    if (!ctx) return MVO_ERR_INVALID;
    auto invalid = [&](const char* what) {  // the message names the entry point the caller used
        return mvo_set_err(ctx, MVO_ERR_INVALID, (std::string(who) + ": " + what).c_str(), hipSuccess);
    };
    if (!map || !T_w_c || !level_scale || nt < 0 || (nt && (!t || !txy || !t_level)) || (map->n && (!idx || !dist)))
        return invalid("bad arguments");
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(T_w_c[k])) return invalid("T_w_c is not finite");
    double Ti[16];
    if (mvo_invert_pose(T_w_c, Ti) != MVO_OK) return invalid("T_w_c is singular");
    if (fx == 0 || fy == 0 || !std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy))
        return invalid("fx or fy 0, or intrinsics not finite");
    if (cols <= 0 || rows <= 0) return invalid("cols or rows <= 0");
    if (n_levels < 1 || n_levels > LM_MAX_LEVELS) return invalid("n_levels outside 1..16");
    for (int l = 0; l < n_levels; ++l)
        if (!std::isfinite(level_scale[l]) || !(level_scale[l] > 0) || (l && !(level_scale[l] > level_scale[l - 1])))
            return invalid("level_scale not positive, finite and strictly increasing");
    const mvo_local_map_params P = params ? *params : kDefaults;
    if (!std::isfinite(P.min_view_cos) || !std::isfinite(P.near_cos)) return invalid("min_view_cos or near_cos not finite");
    for (double r : {P.radius_near, P.radius_far, P.radius_scale})
        if (!std::isfinite(r) || r < 0) return invalid("a radius or radius_scale negative or not finite");
    if (nt > 65535)
        return mvo_set_err(ctx, MVO_ERR_CAPACITY, (std::string(who) + ": more than 65535 train descriptors").c_str(), hipSuccess);
    for (int j = 0; j < nt; ++j)
        if (t_level[j] != -2 && (t_level[j] < 0 || t_level[j] >= n_levels)) return invalid("a t_level entry neither a level nor -2");
    const int n_map = map->n;
    if (n_map == 0) return MVO_OK;
    if (!map->has_view) return invalid("no view data since the last upload");
    LocalMapArgs a{};
    std::memcpy(a.view.T, Ti, sizeof a.view.T);
    a.view.fx = fx, a.view.fy = fy, a.view.cx = cx, a.view.cy = cy;
    a.view.cols = cols, a.view.rows = rows;
    for (int r = 0; r < 3; ++r) a.O[r] = T_w_c[4 * r + 3];
    for (int l = 0; l < LM_MAX_LEVELS; ++l) a.level_scale[l] = level_scale[std::min(l, n_levels - 1)];
    a.min_view_cos = P.min_view_cos, a.radius_near = P.radius_near, a.radius_far = P.radius_far;
    a.near_cos = P.near_cos, a.radius_scale = P.radius_scale;
    a.n_levels = n_levels;
    mvo_local_map_state* e = mvo_state(ctx->local_map);
    // the upload: the gate's view of the frame keypoints, the skip mask, the descriptors of the host-pointer form
    BlockCursor in;
    const size_t o_tg = in.block((size_t)nt * 24), o_skip = in.block((size_t)n_map);
    const size_t o_desc = in.last(t_on_device ? 0 : (size_t)nt * 32);
    const size_t out_bytes = align64((size_t)n_map * 40);
    StagedCall call{ctx};
    int r = call.begin(e->d_in, in.bytes, (size_t)1 << 18, out_bytes, [&] { return e->scratch.ensure(ctx, n_map); });
    if (r) return r;
    double* h_tg = reinterpret_cast<double*>(call.h_in + o_tg);
    for (int j = 0; j < nt; ++j) {
        h_tg[3 * j] = (double)txy[2 * j];
        h_tg[3 * j + 1] = (double)txy[2 * j + 1];
        h_tg[3 * j + 2] = (double)t_level[j];
    }
    for (int i = 0; i < n_map; ++i) call.h_in[o_skip + i] = skip && skip[i] ? 1 : 0;
    if (!t_on_device && nt) std::memcpy(call.h_in + o_desc, t, (size_t)nt * 32);
    if ((r = call.upload(e->d_in))) return r;
    const uint8_t* d_t = t_on_device ? static_cast<const uint8_t*>(t) : e->d_in + o_desc;
    ExtractGate gate(ctx);
    if ((r = local_map_launch(ctx, map->d_pos, map->d_desc, map->d_normal, map->d_max_dist, n_map, a, d_t,
                              reinterpret_cast<const double*>(e->d_in + o_tg), e->d_in + o_skip, nt, e->scratch.partials(),
                              reinterpret_cast<int32_t*>(call.h_out))) ||
        (r = call.finish(gate)))
        return r;
    const uint8_t* h = call.h_out;
    std::memcpy(idx, h, (size_t)n_map * 8);
    std::memcpy(dist, h + (size_t)n_map * 8, (size_t)n_map * 8);
    if (px) std::memcpy(px, h + (size_t)n_map * 16, (size_t)n_map * 8);
    if (n_candidates) std::memcpy(n_candidates, h + (size_t)n_map * 24, (size_t)n_map * 4);
    if (level) std::memcpy(level, h + (size_t)n_map * 28, (size_t)n_map * 4);
    if (view_cos) std::memcpy(view_cos, h + (size_t)n_map * 32, (size_t)n_map * 8);
    return MVO_OK;
}

}  // namespace

extern "C" {

// ORB-SLAM MapPoint::GetNormal, MapPoint::GetMaxDistanceInvariance: what Frame::isInFrustum reads of a map point
int mvo_map_upload_view(mvo_ctx* ctx, mvo_map* map, const float* normal, const float* max_dist) {
    if (!ctx) return MVO_ERR_INVALID;
    if (!map || (map->n && (!normal || !max_dist)))
        return mvo_set_err(ctx, MVO_ERR_INVALID, "mvo_map_upload_view: bad arguments", hipSuccess);
    MVO_HIP(hipSetDevice(ctx->device));
    const size_t n = (size_t)map->n;
    int r;
    if (n * 3 > map->d_normal.cap || n > map->d_max_dist.cap) MVO_HIP(hipStreamSynchronize(ctx->stream));
    if ((r = map->d_normal.ensure(ctx, n * 3, 4096 * 3)) || (r = map->d_max_dist.ensure(ctx, n, 4096))) return r;
    if (n) {
        // staged through pinned memory so that the caller's arrays may be reused as soon as we return
        if ((r = mvo_ensure_pinned(ctx, n * 16))) return r;
        MVO_HIP(hipStreamSynchronize(ctx->stream));
        std::memcpy(ctx->h_pin, normal, n * 12);
        std::memcpy(ctx->h_pin + n * 12, max_dist, n * 4);
        MVO_HIP(hipMemcpyAsync(map->d_normal, ctx->h_pin, n * 12, hipMemcpyHostToDevice, ctx->stream));
        MVO_HIP(hipMemcpyAsync(map->d_max_dist, ctx->h_pin + n * 12, n * 4, hipMemcpyHostToDevice, ctx->stream));
        MVO_HIP(hipStreamSynchronize(ctx->stream));
    }
    map->has_view = true;
    return MVO_OK;
}

// ORB-SLAM Tracking::SearchLocalPoints: Frame::isInFrustum + ORBmatcher::SearchByProjection(F, vpMapPoints, th)
int mvo_map_match_knn2_local(mvo_ctx* ctx, mvo_map* map, const double* T_w_c, double fx, double fy, double cx, double cy, int cols,
                             int rows, const uint8_t* t, const float* txy, const int32_t* t_level, int nt, const uint8_t* skip,
                             const double* level_scale, int n_levels, const mvo_local_map_params* params, float* px, int32_t* idx,
                             int32_t* dist, int32_t* n_candidates, int32_t* level, double* view_cos) {
    return run(ctx, map, T_w_c, fx, fy, cx, cy, cols, rows, t, false, txy, t_level, nt, skip, level_scale, n_levels, params, px, idx,
               dist, n_candidates, level, view_cos, "mvo_map_match_knn2_local");
}

// Tracking::SearchLocalPoints: the same with the frame's descriptors already in HBM
int mvo_map_match_knn2_local_dev(mvo_ctx* ctx, mvo_map* map, const double* T_w_c, double fx, double fy, double cx, double cy, int cols,
                                 int rows, const void* d_t, const float* txy, const int32_t* t_level, int nt, const uint8_t* skip,
                                 const double* level_scale, int n_levels, const mvo_local_map_params* params, float* px,
                                 int32_t* idx, int32_t* dist, int32_t* n_candidates, int32_t* level, double* view_cos) {
    return run(ctx, map, T_w_c, fx, fy, cx, cy, cols, rows, d_t, true, txy, t_level, nt, skip, level_scale, n_levels, params, px, idx,
               dist, n_candidates, level, view_cos, "mvo_map_match_knn2_local_dev");
}

// ORBmatcher::SearchByProjection(F, vpMapPoints, th): the raw call, its acceptance rule, one point per keypoint
int mvo_map_match_features_local(mvo_ctx* ctx, mvo_map* map, const double* T_w_c, double fx, double fy, double cx, double cy, int cols,
                                 int rows, const uint8_t* t, const float* txy, const int32_t* t_level, int nt, const uint8_t* skip,
                                 const double* level_scale, int n_levels, const mvo_local_map_params* params, float* px,
                                 int32_t* level, mvo_dmatch* out, int cap, int* n) {
    if (!ctx) return MVO_ERR_INVALID;
    if (!n || !map || cap < 0) return mvo_set_err(ctx, MVO_ERR_INVALID, "mvo_map_match_features_local: bad arguments", hipSuccess);
    *n = 0;
    const int n1 = map->n;
    std::vector<int32_t> idx(2 * (size_t)n1 + 2), dist(2 * (size_t)n1 + 2);
    int r = run(ctx, map, T_w_c, fx, fy, cx, cy, cols, rows, t, false, txy, t_level, nt, skip, level_scale, n_levels, params, px,
                idx.data(), dist.data(), nullptr, level, nullptr, "mvo_map_match_features_local");
    if (r) return r;
    const mvo_local_map_params P = params ? *params : kDefaults;
    // the rule of SearchByProjection: the ratio counts only between two neighbours of one level, and it is inclusive.  The
    // rejected rows lose their neighbours; what is left goes through the ceiling and the one-query-per-train rule of
    // guided_filter_matches, whose ratio test a row without a second neighbour does not meet.
    for (int i = 0; i < n1; ++i) {
        const int j0 = idx[2 * i], j1 = idx[2 * i + 1];
        if (j0 < 0) continue;
        const bool kept = j1 < 0 || t_level[j0] != t_level[j1] || (double)dist[2 * i] <= P.lowe_ratio * (double)dist[2 * i + 1];
        if (!kept) idx[2 * i] = -1;
        idx[2 * i + 1] = -1;
    }
    return guided_filter_matches(ctx, idx.data(), dist.data(), n1, nt, 0.0, P.max_hamming, out, cap, n);
}

}  // extern "C"
