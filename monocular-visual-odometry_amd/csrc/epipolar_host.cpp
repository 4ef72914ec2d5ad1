// csrc/epipolar_host.cpp -- host side of the pose-guided matcher (include/mvo_hip.h: mvo_match_knn2_epipolar,
// mvo_match_knn2_epipolar_dev, mvo_match_features_epipolar, mvo_fundamental_from_poses): argument checks, the per-train
// tolerance, staging, the filter and the one-query-per-train rule.  The kernel is in epipolar_kernels.hip, the arithmetic in
// DESIGN.md section 14.  No other translation unit refers to this one.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "guided_match_host.h"

namespace {

int ensure_bufs(mvo_ctx* ctx, int nq, int nt) {
    mvo_epipolar_state* e = mvo_state(ctx->epi);
    int r;
    if ((r = e->d_q.ensure(ctx, (size_t)nq * 32, 4096 * 32)) || (r = e->d_qxy.ensure(ctx, (size_t)nq * 2, 4096 * 2)) ||
        (r = e->scratch.ensure(ctx, nq)) || (r = e->d_t.ensure(ctx, (size_t)nt * 32, 4096 * 32)) ||
        (r = e->d_txy.ensure(ctx, (size_t)nt * 2, 4096 * 2)) || (r = e->d_tol2.ensure(ctx, nt, 4096)))
        return r;
    return MVO_OK;
}

// the checks every form shares; MVO_OK with *done set: nothing to launch, the outputs are filled
int check_and_trivial(mvo_ctx* ctx, const void* q, const float* qxy, int nq, const void* t, const float* txy, const float* t_scale,
                      int nt, const double* F, double max_line_px, int32_t* idx, int32_t* dist, int32_t* n_candidates, bool* done) {
    *done = false;
    if (!ctx) return MVO_ERR_INVALID;
    if (nq < 0 || nt < 0 || !F || (nq && (!q || !qxy || !idx || !dist)) || (nt && (!t || !txy)))
        return mvo_set_err(ctx, MVO_ERR_INVALID, "mvo_match_knn2_epipolar: bad arguments", hipSuccess);
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(F[k])) return mvo_set_err(ctx, MVO_ERR_INVALID, "mvo_match_knn2_epipolar: F is not finite", hipSuccess);
    if (!(max_line_px >= 0)) return mvo_set_err(ctx, MVO_ERR_INVALID, "mvo_match_knn2_epipolar: max_line_px negative or NaN", hipSuccess);
    if (int r = guided_check_trains(ctx, "mvo_match_knn2_epipolar", t_scale, nt)) return r;
    if (nq == 0 || nt == 0) {
        for (int i = 0; i < nq; ++i) {
            idx[2 * i] = idx[2 * i + 1] = -1;
            dist[2 * i] = dist[2 * i + 1] = INT_MAX;
            if (n_candidates) n_candidates[i] = 0;
        }
        *done = true;
    }
    return MVO_OK;
}

// d_q / d_t: device descriptors; qxy, txy, t_scale: host.  nq, nt >= 1, arguments checked.
int run(mvo_ctx* ctx, const uint8_t* d_q, const float* qxy, int nq, const uint8_t* d_t, const float* txy, const float* t_scale,
        int nt, const double* F, double max_line_px, int32_t* idx, int32_t* dist, int32_t* n_candidates) {
    mvo_epipolar_state* e = ctx->epi.get();
    std::vector<double> tol2(nt);
    for (int j = 0; j < nt; ++j) tol2[j] = guided_tol2(max_line_px, t_scale, j);
    EpipolarArgs a;
    std::memcpy(a.f, F, sizeof a.f);
    // the kernel writes the nq x (idx[2], dist[2]) block and the counts straight into the pinned staging buffer
    int r = mvo_ensure_pinned(ctx, (size_t)nq * 20);
    if (r) return r;
    MVO_HIP(hipMemcpyAsync(e->d_qxy, qxy, (size_t)nq * 8, hipMemcpyHostToDevice, ctx->stream));
    MVO_HIP(hipMemcpyAsync(e->d_txy, txy, (size_t)nt * 8, hipMemcpyHostToDevice, ctx->stream));
    MVO_HIP(hipMemcpyAsync(e->d_tol2, tol2.data(), (size_t)nt * 8, hipMemcpyHostToDevice, ctx->stream));
    ExtractGate gate(ctx);
    if ((r = epipolar_launch_knn2(ctx, d_q, e->d_qxy, nq, d_t, e->d_txy, e->d_tol2, nt, a, e->scratch.partials(),
                                  reinterpret_cast<int32_t*>(ctx->h_pin))) ||
        (r = StagedCall{ctx}.finish(gate)))  // (tol2 is pageable: its copy has left the vector by now either way)
        return r;
    std::memcpy(idx, ctx->h_pin, (size_t)nq * 8);
    std::memcpy(dist, ctx->h_pin + (size_t)nq * 8, (size_t)nq * 8);
    if (n_candidates) std::memcpy(n_candidates, ctx->h_pin + (size_t)nq * 16, (size_t)nq * 4);
    return MVO_OK;
}

}  // namespace

extern "C" {

// README.md:212 ("doing guided matching based on the estimated camera motion"), README.md:272 ("Utilize epipolar constraint
// to do feature matching"): the reference names the method and has no function for it
int mvo_match_knn2_epipolar(mvo_ctx* ctx, const uint8_t* q, const float* qxy, int nq, const uint8_t* t, const float* txy,
                            const float* t_scale, int nt, const double* F, double max_line_px, int32_t* idx, int32_t* dist,
                            int32_t* n_candidates) {
    bool done;
    int r = check_and_trivial(ctx, q, qxy, nq, t, txy, t_scale, nt, F, max_line_px, idx, dist, n_candidates, &done);
    if (r || done) return r;
    MVO_HIP(hipSetDevice(ctx->device));
    if ((r = ensure_bufs(ctx, nq, nt))) return r;
    mvo_epipolar_state* e = ctx->epi.get();
    MVO_HIP(hipMemcpyAsync(e->d_q, q, (size_t)nq * 32, hipMemcpyHostToDevice, ctx->stream));
    MVO_HIP(hipMemcpyAsync(e->d_t, t, (size_t)nt * 32, hipMemcpyHostToDevice, ctx->stream));
    return run(ctx, e->d_q, qxy, nq, e->d_t, txy, t_scale, nt, F, max_line_px, idx, dist, n_candidates);
}

// README.md:212, README.md:272: the same with both descriptor sets already in HBM
int mvo_match_knn2_epipolar_dev(mvo_ctx* ctx, const void* d_q, const float* qxy, int nq, const void* d_t, const float* txy,
                                const float* t_scale, int nt, const double* F, double max_line_px, int32_t* idx, int32_t* dist,
                                int32_t* n_candidates) {
    bool done;
    int r = check_and_trivial(ctx, d_q, qxy, nq, d_t, txy, t_scale, nt, F, max_line_px, idx, dist, n_candidates, &done);
    if (r || done) return r;
    MVO_HIP(hipSetDevice(ctx->device));
    if ((r = ensure_bufs(ctx, nq, nt))) return r;
    return run(ctx, (const uint8_t*)d_q, qxy, nq, (const uint8_t*)d_t, txy, t_scale, nt, F, max_line_px, idx, dist, n_candidates);
}

// README.md:212, README.md:272: the raw call, the filter, one query per train
int mvo_match_features_epipolar(mvo_ctx* ctx, const uint8_t* d1, const float* xy1, int n1, const uint8_t* d2, const float* xy2,
                                const float* scale2, int n2, const double* F, double max_line_px, double lowe_ratio, int max_hamming,
                                mvo_dmatch* out, int cap, int* n) {
    if (!ctx) return MVO_ERR_INVALID;
    if (!n || n1 < 0 || n2 < 0) return mvo_set_err(ctx, MVO_ERR_INVALID, "mvo_match_features_epipolar: bad arguments", hipSuccess);
    *n = 0;
    std::vector<int32_t> idx(2 * (size_t)n1 + 2), dist(2 * (size_t)n1 + 2);
    int r = mvo_match_knn2_epipolar(ctx, d1, xy1, n1, d2, xy2, scale2, n2, F, max_line_px, idx.data(), dist.data(), nullptr);
    if (r) return r;
    return guided_filter_matches(ctx, idx.data(), dist.data(), n1, n2, lowe_ratio, max_hamming, out, cap, n);
}

// README.md:212 ("based on the estimated camera motion"): the fundamental matrix of the two estimated poses
int mvo_fundamental_from_poses(const double* T_w_c_1, const double* T_w_c_2, double fx, double fy, double cx, double cy, double* F) {
    if (!T_w_c_1 || !T_w_c_2 || !F || fx == 0 || fy == 0 || !std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) ||
        !std::isfinite(cy))
        return MVO_ERR_INVALID;
    double Ti1[16], Ti2[16], T[16];
    if (mvo_invert_pose(T_w_c_1, Ti1) != MVO_OK || mvo_invert_pose(T_w_c_2, Ti2) != MVO_OK) return MVO_ERR_INVALID;
    for (int i = 0; i < 4; ++i)  // T_2_1 = inv(T_w_c_2) * T_w_c_1, summed k = 0..3 in order
        for (int j = 0; j < 4; ++j) {
            double s = 0;
            for (int k = 0; k < 4; ++k) s += Ti2[4 * i + k] * T_w_c_1[4 * k + j];
            T[4 * i + j] = s;
        }
    const double tx = T[3], ty = T[7], tz = T[11];
    const double S[9] = {0, -tz, ty, tz, 0, -tx, -ty, tx, 0};  // [t]x
    const double Ki[9] = {1 / fx, 0, -cx / fx, 0, 1 / fy, -cy / fy, 0, 0, 1};
    double E[9], M[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += S[3 * i + k] * T[4 * k + j];
            E[3 * i + j] = s;
        }
    for (int i = 0; i < 3; ++i)  // M = E K^-1
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += E[3 * i + k] * Ki[3 * k + j];
            M[3 * i + j] = s;
        }
    for (int i = 0; i < 3; ++i)  // F = K^-T M
        for (int j = 0; j < 3; ++j) {
            double s = 0;
            for (int k = 0; k < 3; ++k) s += Ki[3 * k + i] * M[3 * k + j];
            F[3 * i + j] = s;
        }
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(F[k])) return MVO_ERR_INVALID;
    return MVO_OK;
}

}  // extern "C"
