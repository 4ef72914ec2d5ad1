// csrc/pose_optimize_host.cpp -- host side of the robust motion-only pose optimisation (include/mvo_hip.h: mvo_optimize_pose,
// mvo_debug_get_pose_optimize): argument checks, the inverse of the initial pose, one upload, the launch, the results and the
// inverse of the final state.  The kernel is in pose_optimize_kernels.hip, the arithmetic in DESIGN.md section 21.  No other
// translation unit refers to this one.
#include <cmath>
#include <cstring>

#include "staged_call.h"

extern "C" {

// ORB-SLAM's Optimizer::PoseOptimization (called by TrackWithMotionModel) in place of cv::solvePnPRansac in the reference's
// poseEstimationPnP_ (vo.cpp:291-347); the reference's own single-pose optimiser is optimizeSingleFrame (g2o_ba.cpp:34-170)
int mvo_optimize_pose(mvo_ctx* ctx, const float* pts3d, const float* pts2d, const float* inv_sigma2, int n, const double* T_w_c_init,
                      double fx, double fy, double cx, double cy, const mvo_pose_optimize_params* params, double* T_w_c, double* T_c_w,
                      uint8_t* outlier, double* chi2, int32_t* info) {
    if (!ctx) return MVO_ERR_INVALID;
    auto invalid = [&](const char* what, int code = MVO_ERR_INVALID) {
        return mvo_set_err(ctx, code, (std::string("mvo_optimize_pose: ") + what).c_str(), hipSuccess);
    };
    if (n < 0 || !T_w_c_init || !T_w_c || !chi2 || !info || (n && (!pts3d || !pts2d || !outlier))) return invalid("bad arguments");
    mvo_pose_optimize_params P{4, 10, 10, 5.991, std::sqrt(5.991), 1e-6};
    if (params) P = *params;
    if (P.rounds < 1 || P.rounds > PO_MAX_ROUNDS || P.iterations < 1 || P.iterations > 64 || P.min_inliers < 6 || P.min_inliers > PO_MAX_OBS ||
        !(P.chi2_threshold > 0) || !std::isfinite(P.chi2_threshold) || !(P.huber_delta > 0) || !std::isfinite(P.huber_delta) ||
        !(P.rel_tolerance >= 0) || !std::isfinite(P.rel_tolerance))
        return invalid("params out of range");
    if (fx == 0 || fy == 0 || !std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy))
        return invalid("fx or fy 0, or intrinsics not finite");
    for (int k = 0; k < 16; ++k)
        if (!std::isfinite(T_w_c_init[k])) return invalid("T_w_c_init is not finite");
    double T0[16];
    if (mvo_invert_pose(T_w_c_init, T0) != MVO_OK) return invalid("T_w_c_init is singular");
    if (n > PO_MAX_OBS) return invalid("more than 4096 observations", MVO_ERR_CAPACITY);
    for (size_t k = 0; k < 3 * (size_t)n; ++k)
        if (!std::isfinite(pts3d[k])) return invalid("pts3d is not finite");
    for (size_t k = 0; k < 2 * (size_t)n; ++k)
        if (!std::isfinite(pts2d[k])) return invalid("pts2d is not finite");
    if (inv_sigma2)
        for (int k = 0; k < n; ++k)
            if (!(inv_sigma2[k] >= 0) || !std::isfinite(inv_sigma2[k])) return invalid("inv_sigma2 is negative or not finite");
    const double last_row[4] = {0.0, 0.0, 0.0, 1.0};
    std::memcpy(T0 + 12, last_row, sizeof last_row);
    if (n == 0) {  // status 2 without a launch
        std::memcpy(T_w_c, T_w_c_init, 16 * sizeof(double));
        if (T_c_w) std::memcpy(T_c_w, T0, sizeof T0);
        chi2[0] = chi2[1] = 0.0;
        const int32_t none[6] = {2, 0, 0, 0, 0, 0};
        std::memcpy(info, none, sizeof none);
        return MVO_OK;
    }
    PoseOptArgs a;
    std::memcpy(a.T0, T0, sizeof a.T0);
    a.fx = fx, a.fy = fy, a.cx = cx, a.cy = cy;
    a.delta = P.huber_delta, a.chi2_thr = P.chi2_threshold, a.rel_tol = P.rel_tolerance;
    a.rounds = P.rounds, a.iterations = P.iterations, a.min_inliers = P.min_inliers, a.has_sigma = inv_sigma2 ? 1 : 0;
    // pinned staging: the kernel writes the pose, chi2, the rows, info and the flags straight into the first part; the second
    // carries the observations up (one copy)
    BlockCursor out, in;
    const size_t o_out = out.block(sizeof(PoseOptOut)), o_flag = out.block((size_t)n);
    const size_t i_p3 = in.block((size_t)n * 12), i_p2 = in.block((size_t)n * 8), i_sigma = in.last(inv_sigma2 ? (size_t)n * 4 : 0);
    mvo_pose_opt_state* e = mvo_state(ctx->pose_opt);
    StagedCall call{ctx};
    int r = call.begin(e->d_in, in.bytes, (size_t)1 << 16, out.bytes);
    if (r) return r;
    std::memcpy(call.h_in + i_p3, pts3d, (size_t)n * 12);
    std::memcpy(call.h_in + i_p2, pts2d, (size_t)n * 8);
    if (inv_sigma2) std::memcpy(call.h_in + i_sigma, inv_sigma2, (size_t)n * 4);
    if ((r = call.upload(e->d_in))) return r;
    PoseOptOut* h_out = reinterpret_cast<PoseOptOut*>(call.h_out + o_out);
    uint8_t* h_flag = call.h_out + o_flag;
    ExtractGate gate(ctx);
    if ((r = pose_optimize_launch(ctx, reinterpret_cast<const float*>(e->d_in + i_p3), reinterpret_cast<const float*>(e->d_in + i_p2),
                                  inv_sigma2 ? reinterpret_cast<const float*>(e->d_in + i_sigma) : nullptr, n, a, h_out, h_flag)) ||
        (r = call.finish(gate)))
        return r;
    const int status = h_out->info[0];
    double Tcw[16], Twc[16];
    std::memcpy(Tcw, h_out->Tcw, sizeof h_out->Tcw);
    std::memcpy(Tcw + 12, last_row, sizeof last_row);
    if (status == 2 || status == 3) {  // the initial pose, bit for bit
        std::memcpy(Twc, T_w_c_init, sizeof Twc);
    } else if (mvo_invert_pose(Tcw, Twc) != MVO_OK) {
        return mvo_set_err(ctx, MVO_ERR_STATE, "mvo_optimize_pose: the optimised pose is singular", hipSuccess);
    }
    e->n_rounds = h_out->info[1];
    std::memcpy(e->rows, h_out->rows, (size_t)e->n_rounds * 6 * sizeof(double));
    std::memcpy(T_w_c, Twc, sizeof Twc);
    if (T_c_w) std::memcpy(T_c_w, Tcw, sizeof Tcw);
    std::memcpy(outlier, h_flag, (size_t)n);
    chi2[0] = h_out->chi2[0], chi2[1] = h_out->chi2[1];
    std::memcpy(info, h_out->info, 6 * sizeof(int32_t));
    return MVO_OK;
}

int mvo_debug_get_pose_optimize(mvo_ctx* ctx, double* rows, int cap, int* n_rounds) {
    if (!ctx) return MVO_ERR_INVALID;
    if (!ctx->pose_opt) return mvo_set_err(ctx, MVO_ERR_STATE, "no mvo_optimize_pose launch on this ctx yet", hipSuccess);
    if (!n_rounds || cap < 0 || (cap && !rows)) return mvo_set_err(ctx, MVO_ERR_INVALID, "mvo_debug_get_pose_optimize: bad arguments", hipSuccess);
    const mvo_pose_opt_state* e = ctx->pose_opt.get();
    *n_rounds = e->n_rounds;
    if (cap < e->n_rounds) return mvo_set_err(ctx, MVO_ERR_CAPACITY, "mvo_debug_get_pose_optimize: buffer too small", hipSuccess);
    if (e->n_rounds) std::memcpy(rows, e->rows, (size_t)e->n_rounds * 6 * sizeof(double));
    return MVO_OK;
}

}  // extern "C"
