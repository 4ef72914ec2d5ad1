// csrc/projection_host.cpp -- host side of tracking by projection (include/mvo_hip.h: mvo_map_match_knn2_projection,
// mvo_map_match_knn2_projection_dev, mvo_map_match_features_projection, mvo_map_size, mvo_predict_pose): argument checks, the per-keypoint
// radius, staging, the filter and the one-query-per-train rule.  The kernel is in projection_kernels.hip, the arithmetic in
// DESIGN.md section 15.  No other translation unit refers to this one.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "guided_match_host.h"

namespace {

int ensure_bufs(mvo_ctx* ctx, int n_map, int nt) {
    mvo_projection_state* e = mvo_state(ctx->proj);
    int r;
    if ((r = e->scratch.ensure(ctx, n_map)) || (r = e->d_t.ensure(ctx, (size_t)nt * 32, 4096 * 32)) ||
        (r = e->d_tg.ensure(ctx, (size_t)nt * 3, 4096 * 3)))
        return r;
    return MVO_OK;
}

// Every form: the checks, the upload, the launch, the results.  t is a host pointer (t_on_device false) or a device pointer.
int run(mvo_ctx* ctx, mvo_map* map, const double* T_w_c, double fx, double fy, double cx, double cy, int cols, int rows,
        const void* t, bool t_on_device, const float* txy, const float* t_scale, int nt, double max_px, float* px, int32_t* idx,
        int32_t* dist, int32_t* n_candidates, const char* who) {
    if (!ctx) return MVO_ERR_INVALID;
    auto invalid = [&](const char* what) {  // the message names the entry point the caller used
        return mvo_set_err(ctx, MVO_ERR_INVALID, (std::string(who) + ": " + what).c_str(), hipSuccess);
    };
    if (!map || !T_w_c || nt < 0 || (nt && (!t || !txy)) || (map->n && (!idx || !dist)))
        return invalid("bad arguments");
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(T_w_c[k])) return invalid("T_w_c is not finite");
    double Ti[16];
    if (mvo_invert_pose(T_w_c, Ti) != MVO_OK)
        return invalid("T_w_c is singular");
    if (fx == 0 || fy == 0 || !std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy))
        return invalid("fx or fy 0, or intrinsics not finite");
    if (cols <= 0 || rows <= 0) return invalid("cols or rows <= 0");
    if (!(max_px >= 0)) return invalid("max_px negative or NaN");
    if (int r = guided_check_trains(ctx, who, t_scale, nt)) return r;
    const int n_map = map->n;
    if (n_map == 0) return MVO_OK;
    TrackViewArgs a;
    std::memcpy(a.T, Ti, sizeof a.T);
    a.fx = fx, a.fy = fy, a.cx = cx, a.cy = cy;
    a.cols = cols, a.rows = rows;
    MVO_HIP(hipSetDevice(ctx->device));
    int r = ensure_bufs(ctx, n_map, nt);
    if (r) return r;
    mvo_projection_state* e = ctx->proj.get();
    // pinned staging: the kernel writes its n_map x 28 bytes of results straight into the first part; the second carries the
    // gate's view of the frame keypoints up (one copy)
    const size_t out_bytes = align64((size_t)n_map * 28);
    if ((r = mvo_ensure_pinned(ctx, out_bytes + (size_t)nt * 24))) return r;
    MVO_HIP(hipStreamSynchronize(ctx->stream));  // (nothing of an earlier call may still be reading the staging buffer)
    int32_t* h_out = reinterpret_cast<int32_t*>(ctx->h_pin);
    double* h_tg = reinterpret_cast<double*>(ctx->h_pin + out_bytes);
    for (int j = 0; j < nt; ++j) {
        h_tg[3 * j] = (double)txy[2 * j];
        h_tg[3 * j + 1] = (double)txy[2 * j + 1];
        h_tg[3 * j + 2] = guided_tol2(max_px, t_scale, j);
    }
    const uint8_t* d_t = static_cast<const uint8_t*>(t);
    if (nt) {
        MVO_HIP(hipMemcpyAsync(e->d_tg, h_tg, (size_t)nt * 24, hipMemcpyHostToDevice, ctx->stream));
        if (!t_on_device) {
            MVO_HIP(hipMemcpyAsync(e->d_t, t, (size_t)nt * 32, hipMemcpyHostToDevice, ctx->stream));
            d_t = e->d_t;
        }
    }
    ExtractGate gate(ctx);
    if ((r = projection_launch(ctx, map->d_pos, map->d_desc, n_map, a, d_t, e->d_tg, nt, e->scratch.partials(), h_out)) ||
        (r = StagedCall{ctx}.finish(gate)))
        return r;
    std::memcpy(idx, ctx->h_pin, (size_t)n_map * 8);
    std::memcpy(dist, ctx->h_pin + (size_t)n_map * 8, (size_t)n_map * 8);
    if (px) std::memcpy(px, ctx->h_pin + (size_t)n_map * 16, (size_t)n_map * 8);
    if (n_candidates) std::memcpy(n_candidates, ctx->h_pin + (size_t)n_map * 24, (size_t)n_map * 4);
    return MVO_OK;
}

// D = A * B, row-major 4 x 4, summed k = 0..3 in order
void mul4(const double* A, const double* B, double* D) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0;
            for (int k = 0; k < 4; ++k) s += A[4 * i + k] * B[4 * k + j];
            D[4 * i + j] = s;
        }
}

}  // namespace

extern "C" {

// README.md:212 ("doing guided matching based on the estimated camera motion"), vo.cpp:267-289 (the step it replaces:
// getMappointsInCurrentView_ + matchFeatures in poseEstimationPnP_)
int mvo_map_match_knn2_projection(mvo_ctx* ctx, mvo_map* map, const double* T_w_c, double fx, double fy, double cx, double cy,
                                  int cols, int rows, const uint8_t* t, const float* txy, const float* t_scale, int nt, double max_px,
                                  float* px, int32_t* idx, int32_t* dist, int32_t* n_candidates) {
    return run(ctx, map, T_w_c, fx, fy, cx, cy, cols, rows, t, false, txy, t_scale, nt, max_px, px, idx, dist, n_candidates,
               "mvo_map_match_knn2_projection");
}

// README.md:212, vo.cpp:267-289: the same with the frame's descriptors already in HBM
int mvo_map_match_knn2_projection_dev(mvo_ctx* ctx, mvo_map* map, const double* T_w_c, double fx, double fy, double cx, double cy,
                                      int cols, int rows, const void* d_t, const float* txy, const float* t_scale, int nt,
                                      double max_px, float* px, int32_t* idx, int32_t* dist, int32_t* n_candidates) {
    return run(ctx, map, T_w_c, fx, fy, cx, cy, cols, rows, d_t, true, txy, t_scale, nt, max_px, px, idx, dist, n_candidates,
               "mvo_map_match_knn2_projection_dev");
}

// README.md:212, vo.cpp:267-289: the raw call, the filter, one query per train
int mvo_map_match_features_projection(mvo_ctx* ctx, mvo_map* map, const double* T_w_c, double fx, double fy, double cx, double cy,
                                      int cols, int rows, const uint8_t* t, const float* txy, const float* t_scale, int nt,
                                      double max_px, double lowe_ratio, int max_hamming, float* px, uint8_t* in_view, mvo_dmatch* out,
                                      int cap, int* n) {
    if (!ctx) return MVO_ERR_INVALID;
    if (!n || !map || cap < 0) return mvo_set_err(ctx, MVO_ERR_INVALID, "mvo_map_match_features_projection: bad arguments", hipSuccess);
    *n = 0;
    const int n1 = map->n;
    std::vector<int32_t> idx(2 * (size_t)n1 + 2), dist(2 * (size_t)n1 + 2), cand((size_t)n1 + 1);
    int r = run(ctx, map, T_w_c, fx, fy, cx, cy, cols, rows, t, false, txy, t_scale, nt, max_px, px, idx.data(), dist.data(), cand.data(),
                "mvo_map_match_features_projection");
    if (r) return r;
    if (in_view)
        for (int i = 0; i < n1; ++i) in_view[i] = cand[i] >= 0 ? 1 : 0;
    return guided_filter_matches(ctx, idx.data(), dist.data(), n1, nt, lowe_ratio, max_hamming, out, cap, n);
}

// map.h:19 (Map::map_points_.size() of the resident copy): the number of rows the calls above write
int mvo_map_size(mvo_ctx* ctx, mvo_map* map, int* n) {
    if (!ctx) return MVO_ERR_INVALID;
    if (!map || !n) return mvo_set_err(ctx, MVO_ERR_INVALID, "mvo_map_size: bad arguments", hipSuccess);
    *n = map->n;
    return MVO_OK;
}

// README.md:212 ("based on the estimated camera motion"), vo.cpp:267-289: the constant-velocity prediction of the pose the
// map is projected with, T_pred = T_prev * (inv(T_prev2) * T_prev)
int mvo_predict_pose(const double* T_w_c_prev2, const double* T_w_c_prev, double* T_w_c_pred) {
    if (!T_w_c_prev || !T_w_c_pred) return MVO_ERR_INVALID;
    double out[16];
    if (!T_w_c_prev2) {
        std::memcpy(out, T_w_c_prev, sizeof out);
    } else {
        double Ti[16], D[16];
        if (mvo_invert_pose(T_w_c_prev2, Ti) != MVO_OK) return MVO_ERR_INVALID;
        mul4(Ti, T_w_c_prev, D);
        mul4(T_w_c_prev, D, out);
    }
    std::memcpy(T_w_c_pred, out, sizeof out);
    return MVO_OK;
}

}  // extern "C"
