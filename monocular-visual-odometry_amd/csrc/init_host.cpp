// csrc/init_host.cpp -- the finish of the monocular initialisation (include/mvo_hip.h: mvo_init_two_view): what
// VisualOdometry::estimateMotionAnd3DPoints_ does with the result of
// helperEstimatePossibleRelativePosesByEpipolarGeometry (src/vo/vo.cpp:77-110) and VisualOdometry::isVoGoodToInit_
// (vo.cpp:112-170).  k_init_finish (track_kernels.hip, init_wave.h) computes the per-point part on what the composed
// call left on the device; the tail below is order-sensitive and works on a few thousand items at most, so it stays
// on the host like retainGoodTriangulationResult_ itself and follows the reference's loops
// sequentially.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "mvo_internal.h"

namespace {

// T = T_ref * [R t; 0 1]^-1 (vo.cpp:89,109): the inverse by the LU of mvo_invert_pose (zeros for a singular matrix,
// as cv::Mat::inv leaves them), every entry of the product summed k = 0..3 in order
void compose_pose(const double* T_ref, const double* R, const double* t, double* T) {
    const double M[16] = {R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2], 0, 0, 0, 1};
    double Mi[16];
    if (mvo_invert_pose(M, Mi) != MVO_OK)
        for (double& v : Mi) v = 0;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double v = T_ref[4 * i] * Mi[j];
            v = v + T_ref[4 * i + 1] * Mi[4 + j];
            v = v + T_ref[4 * i + 2] * Mi[8 + j];
            T[4 * i + j] = v + T_ref[4 * i + 3] * Mi[12 + j];
        }
}

}  // namespace

extern "C" {

int mvo_init_two_view(mvo_ctx* ctx, const float* pts1, const float* pts2, int n, double fx, double fy, double cx,
                      double cy, double prob, double threshold, double h_threshold, double h_confidence, double sigma,
                      const double* T_w_c_ref, const mvo_init_params* params, mvo_init_poses* poses,
                      mvo_init_result* out) {
    if (!ctx || !T_w_c_ref || !params || !poses || !out || out->cap < 0 ||
        (out->cap && (!out->matches_for_3d || !out->pts3d_in_curr || !out->angles)))
        return mvo_set_err(ctx, MVO_ERR_INVALID, "bad arguments", hipSuccess);
    out->slot = -1;
    out->n_slot_inliers = out->n_kept = out->scaled = 0;
    for (double& v : out->R) v = 0;
    for (double& v : out->t) v = 0;
    std::memcpy(out->T_w_c, T_w_c_ref, sizeof(out->T_w_c));
    out->mean_depth = out->scale = 0;
    out->mean_pixel_dist = out->mean_angle = out->median_angle = out->min_angle = out->max_angle = 0;
    out->criteria[0] = out->criteria[1] = out->criteria[2] = out->good = 0;
    ctx->init_called = true;
    std::vector<float>& p_curr = ctx->init_p_curr;
    std::vector<double>& cosang = ctx->init_cosang;
    std::vector<double>& pixdist = ctx->init_pixdist;
    p_curr.clear();
    cosang.clear();
    pixdist.clear();
    int r = mvo_estimate_possible_relative_poses(ctx, pts1, pts2, n, fx, fy, cx, cy, prob, threshold, h_threshold,
                                                 h_confidence, sigma, /*motion_cam2_to_cam1=*/1, poses);
    if (r) return r;
    const int slot = poses->best;
    if (slot < 0) return MVO_OK;  // DESIGN.md section 2, deviation 12
    const int32_t* list = slot == 0 ? poses->inliers_e : poses->inliers_h;
    const int m = poses->pts_count[slot];
    if (m > out->cap) return mvo_set_err(ctx, MVO_ERR_CAPACITY, "mvo_init_two_view: result buffers too small", hipSuccess);
    out->slot = slot;
    out->n_slot_inliers = m;
    std::memcpy(out->R, poses->R[slot], sizeof(out->R));
    std::memcpy(out->t, poses->t[slot], sizeof(out->t));
    compose_pose(T_w_c_ref, out->R, out->t, out->T_w_c);
    if (m) {
        // the per-point part on the device, in stream order after k_init_triangulate: nothing is uploaded again
        const size_t bytes = (size_t)m * 28;  // cosang (m doubles), pixdist (m doubles), p_curr (3 m floats)
        TrackInitView v;
        if ((r = track_init_view(ctx, n, m, &v)) || (r = mvo_ensure_pinned(ctx, bytes))) return r;
        const int c = poses->h_candidate[slot];
        const int n_e_list = poses->found_e ? poses->n_inliers_e : 0;
        double* d_cos = reinterpret_cast<double*>(v.out);
        double* d_pix = d_cos + m;
        float* d_pc = reinterpret_cast<float*>(d_pix + m);
        if ((r = track_launch_init_finish(ctx, v.pts + 3 * (size_t)(slot == 0 ? 0 : 1 + c) * n,
                                          v.lists + (slot == 0 ? 0 : n_e_list), m,
                                          slot == 0 ? v.e_out + 9 : v.h_out + kHdR + 9 * c,
                                          slot == 0 ? v.e_out + 18 : v.h_out + kHdTn + 3 * c, v.kp1, v.kp2, out->T_w_c,
                                          T_w_c_ref, d_pc, d_cos, d_pix)))
            return r;
        MVO_HIP(hipMemcpyAsync(ctx->h_pin, v.out, bytes, hipMemcpyDeviceToHost, ctx->stream));
        MVO_HIP(hipStreamSynchronize(ctx->stream));
        if (ctx->prof) mvo_prof_collect(ctx);
        const double* h = reinterpret_cast<const double*>(ctx->h_pin);
        cosang.assign(h, h + m);
        pixdist.assign(h + m, h + 2 * (size_t)m);
        const float* hp = reinterpret_cast<const float*>(h + 2 * (size_t)m);
        p_curr.assign(hp, hp + 3 * (size_t)m);
    }
    // retainGoodTriangulationResult_ (vo.cpp:199-243; N == 0 returns before the median)
    int n_kept = 0;
    double sum_pix = 0;
    if (m) {
        std::vector<double> ang(m);
        for (int i = 0; i < m; ++i) ang[i] = std::acos(cosang[i]) / 3.1415926 * 180.0;  // vo.cpp:210
        std::vector<double> sorted(ang);
        std::sort(sorted.begin(), sorted.end());
        const double median = sorted[m / 2];
        for (int i = 0; i < m; ++i) {
            if (ang[i] < params->min_triang_angle || ang[i] / median > params->max_ratio_to_median) continue;  // vo.cpp:235-237
            out->matches_for_3d[n_kept] = list[i];
            std::memcpy(out->pts3d_in_curr + 3 * (size_t)n_kept, p_curr.data() + 3 * (size_t)i, 12);
            out->angles[n_kept] = ang[i];
            sum_pix += pixdist[i];
            ++n_kept;
        }
    }
    out->n_kept = n_kept;
    if (n_kept >= 20) {  // vo.cpp:94-109
        double mean_depth = 0;
        for (int i = 0; i < n_kept; ++i) mean_depth += (double)out->pts3d_in_curr[3 * (size_t)i + 2];
        mean_depth /= n_kept;
        const double scale = params->assumed_mean_depth / mean_depth;
        for (int k = 0; k < 3; ++k) out->t[k] *= scale;
        for (size_t k = 0; k < 3 * (size_t)n_kept; ++k) out->pts3d_in_curr[k] = (float)((double)out->pts3d_in_curr[k] * scale);
        compose_pose(T_w_c_ref, out->R, out->t, out->T_w_c);
        out->mean_depth = mean_depth;
        out->scale = scale;
        out->scaled = 1;
    }
    // isVoGoodToInit_ (vo.cpp:126-169)
    out->criteria[0] = !(n_kept < params->min_inlier_matches);
    out->mean_pixel_dist = sum_pix / n_kept;
    out->criteria[1] = out->mean_pixel_dist > params->min_pixel_dist;
    if (n_kept > 0) {
        std::vector<double> sort_a(out->angles, out->angles + n_kept);
        std::sort(sort_a.begin(), sort_a.end());
        double acc = 0.0;
        for (double a : sort_a) acc += a;
        out->mean_angle = acc / n_kept;
        out->median_angle = sort_a[n_kept / 2];
        out->min_angle = sort_a[0];
        out->max_angle = sort_a[n_kept - 1];
        out->criteria[2] = out->median_angle > params->min_median_triangulation_angle;
    }
    out->good = out->criteria[0] && out->criteria[1] && out->criteria[2];
    return MVO_OK;
}

int mvo_debug_get_init_finish(mvo_ctx* ctx, float* p_curr, double* cosang, double* pixdist, int cap, int* n) {
    if (!ctx || !ctx->init_called) return mvo_set_err(ctx, MVO_ERR_STATE, "no mvo_init_two_view on this ctx yet", hipSuccess);
    const int m = (int)ctx->init_cosang.size();
    if (n) *n = m;
    if ((p_curr || cosang || pixdist) && m > cap)
        return mvo_set_err(ctx, MVO_ERR_CAPACITY, "mvo_debug_get_init_finish: buffers too small", hipSuccess);
    if (p_curr && m) std::memcpy(p_curr, ctx->init_p_curr.data(), (size_t)m * 12);
    if (cosang && m) std::memcpy(cosang, ctx->init_cosang.data(), (size_t)m * 8);
    if (pixdist && m) std::memcpy(pixdist, ctx->init_pixdist.data(), (size_t)m * 8);
    return MVO_OK;
}
}
