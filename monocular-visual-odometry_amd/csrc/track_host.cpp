// csrc/track_host.cpp -- host side of the tracking rows (include/mvo_hip.h "tracking"): device buffers, the
// sequential parts of cv::solvePnPRansac (subset drawing with cv::RNG, the adaptive iteration count) and the
// map residency used by getMappointsInCurrentView_.  Reference: src/vo/vo.cpp:16-49 and 270-357.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "mvo_internal.h"

struct mvo_track_state {
    // PnP: pairs, subsets, per-hypothesis results, refinement scratch
    DevBuf<double> d_Mg, d_mg;
    DevBuf<uint8_t> d_in;  // pairs + subsets of a solvePnPRansac call, contiguous like their pinned staging (one upload)
    DevBuf<double> d_models;
    DevBuf<int32_t> d_counts;
    DevBuf<uint8_t> d_masks;
    int last_loop_len = 0;  // iterations the RANSAC loop of the previous mvo_solve_pnp_ransac on this ctx ran (0: none yet)
    // record of the last solve (mvo_debug_get_pnp)
    std::vector<double> models;
    std::vector<int32_t> counts;
    int32_t info[6] = {-1, 0, 0, 0, 0, 0};
    // triangulation
    DevBuf<float> d_tri_in, d_tri_out;
    // essential-matrix RANSAC
    DevBuf<double> d_emq;  // q1 (2n) then q2 (2n)
    DevBuf<uint8_t> d_em_mask;
    DevBuf<int32_t> d_em_subsets, d_em_nm, d_em_counts;
    DevBuf<double> d_em_E;
    std::vector<int32_t> em_counts;  // record of the last call: [iterations evaluated x 10]
    int32_t em_info[5] = {-1, -1, 0, 0, 0};
    // homography RANSAC
    DevBuf<float> d_hpts;  // src (2n) then dst (2n)
    DevBuf<uint8_t> d_h_mask;
    DevBuf<int32_t> d_h_subsets, d_h_counts;
    DevBuf<double> d_h_H, d_h_out;
    std::vector<int32_t> h_counts;  // record of the last call: [iterations evaluated]
    int32_t h_info[6] = {-1, 0, 0, 0, 0, 0};
    // recoverPose after the essential-matrix RANSAC (record of the last call: mvo_debug_get_recover_pose)
    DevBuf<uint8_t> d_rp_masks;
    DevBuf<double> d_rp_out;
    DevBuf<int32_t> d_rp_cnt;
    int32_t rp_good[4] = {0, 0, 0, 0};
    int32_t rp_chosen = -1;
    double rp_R1R2t[21] = {};
    std::vector<uint8_t> rp_masks;
    int rp_n = 0;
    // E / H scores
    DevBuf<uint8_t> d_sc_in;  // pts1 (2n float), pts2 (2n float), the E list, the H list
    DevBuf<int32_t> d_sc_kept;
    DevBuf<uint8_t> d_sc_out;  // 2 scores, 2 kept counts
    // homography decomposition (record of the last call: mvo_debug_get_homography_decomposition) and the
    // triangulation of the initialisation's solutions ([5][n] points)
    DevBuf<double> d_hd_out;
    DevBuf<int32_t> d_hd_cnt;
    double hd_out[kHdOut] = {};
    int32_t hd_cnt[kHdCnt] = {};
    DevBuf<float> d_ip_pts;
    DevBuf<uint8_t> d_fin;  // k_init_finish's results
    // map points in view
    DevBuf<uint8_t> d_view_desc;
    DevBuf<int32_t> d_view_n;
};

int g_pnp_replay_skew = 0;

namespace {

mvo_track_state* state(mvo_ctx* ctx) {
    if (!ctx->track) ctx->track = new mvo_track_state();
    return ctx->track;
}

int ensure_pnp(mvo_ctx* ctx, int n, int n_hyp) {
    mvo_track_state* s = state(ctx);
    const size_t N = n, H = n_hyp;
    int r;
    if ((r = s->d_Mg.ensure(ctx, N * 3, 4096 * 3)) || (r = s->d_mg.ensure(ctx, N * 2, 4096 * 2)) ||
        (r = s->d_models.ensure(ctx, H * 12, 128 * 12)) || (r = s->d_counts.ensure(ctx, H, 128)) ||
        (r = s->d_in.ensure(ctx, N * 20 + H * 20 + 64, 4096)) || (r = s->d_masks.ensure(ctx, H * N, (size_t)1 << 20)))
        return r;
    return MVO_OK;
}

// cv::RNG (multiply-with-carry) as RANSACPointSetRegistrator::run seeds it: RNG rng((uint64)-1).
struct MwcRng {
    uint64_t state = 0xffffffffffffffffULL;
    uint32_t next() {
        state = (uint64_t)(uint32_t)state * 4164903690ULL + (uint32_t)(state >> 32);
        return (uint32_t)state;
    }
    int uniform(int lo, int hi) { return lo == hi ? lo : (int)(next() % (uint32_t)(hi - lo) + lo); }
};

// RANSACPointSetRegistrator::getSubset: draw until the slot differs from the earlier ones (PnP's checkSubset
// accepts every sample).
void draw_subsets(int count, int n_iters, int32_t* out) {
    MwcRng rng;
    for (int it = 0; it < n_iters; ++it) {
        int32_t* s = out + 5 * it;
        for (int i = 0; i < 5; ++i) {
            bool fresh;
            do {
                s[i] = rng.uniform(0, count);
                fresh = true;
                for (int j = 0; j < i; ++j) fresh = fresh && s[j] != s[i];
            } while (!fresh);
        }
    }
}

// cv::RANSACUpdateNumIters
int update_num_iters(double p, double ep, int model_points, int max_iters) {
    p = std::min(std::max(p, 0.), 1.);
    ep = std::min(std::max(ep, 0.), 1.);
    double num = std::max(1. - p, DBL_MIN);
    double denom = 1. - std::pow(1. - ep, model_points);
    if (denom < DBL_MIN) return 0;
    num = std::log(num);
    denom = std::log(denom);
    return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)std::lrint(num / denom);
}

// cv::Mat::inv() (DECOMP_LU) of a 4x4 matrix; `rows` = how many rows of the inverse the caller wants
bool invert_pose_lu(const double* T, double* out, int rows = 3) {
    double A[4][4], B[4][4];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            A[i][j] = T[4 * i + j];
            B[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int i = 0; i < 4; ++i) {
        int piv = i;
        for (int j = i + 1; j < 4; ++j)
            if (std::fabs(A[j][i]) > std::fabs(A[piv][i])) piv = j;
        if (std::fabs(A[piv][i]) < DBL_EPSILON * 100) return false;
        if (piv != i) {
            std::swap_ranges(A[i], A[i] + 4, A[piv]);
            std::swap_ranges(B[i], B[i] + 4, B[piv]);
        }
        const double d = -1 / A[i][i];
        for (int j = i + 1; j < 4; ++j) {
            const double alpha = A[j][i] * d;
            for (int c = i + 1; c < 4; ++c) A[j][c] += alpha * A[i][c];
            for (int c = 0; c < 4; ++c) B[j][c] += alpha * B[i][c];
        }
    }
    for (int i = 3; i >= 0; --i)
        for (int j = 0; j < 4; ++j) {
            double s = B[i][j];
            for (int c = i + 1; c < 4; ++c) s -= A[i][c] * B[c][j];
            B[i][j] = s / A[i][i];
        }
    for (int i = 0; i < rows; ++i)
        for (int j = 0; j < 4; ++j) out[4 * i + j] = B[i][j];
    return true;
}

// HomographyEstimatorCallback::checkSubset (OpenCV 4.x fundam.cpp) on the 4 drawn matches.  haveCollinearPoints
// tests the triples that contain the LAST point of the subset (the loop of fundam.cpp: i = count - 1), in either
// image; then the four triangle orientations must agree in both images for all four triangles or for none.
bool h_collinear(const float* p, const int32_t* idx) {
    const int i = 3;
    for (int j = 0; j < i; ++j) {
        const double dx1 = p[2 * idx[j]] - p[2 * idx[i]];
        const double dy1 = p[2 * idx[j] + 1] - p[2 * idx[i] + 1];
        for (int k = 0; k < j; ++k) {
            const double dx2 = p[2 * idx[k]] - p[2 * idx[i]];
            const double dy2 = p[2 * idx[k] + 1] - p[2 * idx[i] + 1];
            if (std::fabs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (std::fabs(dx1) + std::fabs(dy1) + std::fabs(dx2) + std::fabs(dy2)))
                return true;
        }
    }
    return false;
}

double h_det3(const float* p, int a, int b, int c) {  // cv::determinant(Matx33d) of rows (x, y, 1)
    const double m[9] = {p[2 * a], p[2 * a + 1], 1., p[2 * b], p[2 * b + 1], 1., p[2 * c], p[2 * c + 1], 1.};
    return m[0] * (m[4] * m[8] - m[7] * m[5]) - m[1] * (m[3] * m[8] - m[6] * m[5]) + m[2] * (m[3] * m[7] - m[6] * m[4]);
}

bool h_check_subset(const float* src, const float* dst, const int32_t* idx) {
    if (h_collinear(src, idx) || h_collinear(dst, idx)) return false;
    static const int tt[4][3] = {{0, 1, 2}, {1, 2, 3}, {0, 2, 3}, {0, 1, 3}};
    int negative = 0;
    for (int i = 0; i < 4; ++i) {
        const int* t = tt[i];
        negative += h_det3(src, idx[t[0]], idx[t[1]], idx[t[2]]) * h_det3(dst, idx[t[0]], idx[t[1]], idx[t[2]]) < 0;
    }
    return negative == 0 || negative == 4;
}

// RANSACPointSetRegistrator::getSubset (maxAttempts 1000) for up to max_iters iterations of findHomography's loop.
// Returns how many subsets were drawn before getSubset gave up (the loop breaks there; 0 = the call fails).
int draw_h_subsets(const float* src, const float* dst, int count, int max_iters, int32_t* out) {
    MwcRng rng;
    for (int it = 0; it < max_iters; ++it) {
        int32_t* s = out + 4 * it;
        bool found = false;
        for (int attempt = 0; attempt < 1000 && !found; ++attempt) {
            for (int i = 0; i < 4; ++i) {
                bool fresh;
                do {
                    s[i] = rng.uniform(0, count);
                    fresh = true;
                    for (int j = 0; j < i; ++j) fresh = fresh && s[j] != s[i];
                } while (!fresh);
            }
            found = h_check_subset(src, dst, s);
        }
        if (!found) return it;
    }
    return max_iters;
}

// The sequential loop of RANSACPointSetRegistrator::run over counts that exist so far: which model is the best and how many
// iterations the loop's own adaptive stopping rule (RANSACUpdateNumIters, starting from niters) still wants.
struct RansacLoop {
    int niters, max_good = 0, it = 0, best_it = -1, best_m = -1;
    // counts: per_hyp candidates per hypothesis (-1 = none) of the hypotheses [0, evaluated)
    void advance(const int32_t* counts, int evaluated, int per_hyp, int n, int model_points, double prob) {
        for (; it < niters && it < evaluated; ++it)
            for (int m = 0; m < per_hyp; ++m) {
                const int raw = counts[(size_t)it * per_hyp + m];
                const int good = n == model_points && raw >= 0 ? n : raw;
                if (good < 0) break;
                if (good > std::max(max_good, model_points - 1)) {
                    max_good = good;
                    best_it = it;
                    best_m = m;
                    niters = update_num_iters(prob, (double)(n - good) / n, model_points, niters);
                }
                if (n == model_points) break;  // count == modelPoints: the first model is the answer
            }
    }
};

// RansacLoop over device-evaluated hypotheses, shared by findEssentialMat and findHomography.  The hypotheses [0, total)
// are launched in two chunks (chunk_end); after each chunk the counts are read back and the loop is advanced until its
// own stopping rule is met.  rec receives every evaluated count; info = {best hypothesis, best candidate, iterations the
// sequential loop ran, hypotheses evaluated}.  The pinned staging may hold this call's uploads on entry.
template <class Launch>
int ransac_chunks(mvo_ctx* ctx, int n, int model_points, int total, int niters, int per_hyp, double prob,
                  const int (&chunk_end)[2], const int32_t* d_counts, Launch&& launch, std::vector<int32_t>& rec,
                  int32_t* info) {
    int evaluated = 0, r;
    RansacLoop loop{niters};
    bool first_wait = true;
    for (int c = 0; c < 2 && loop.it < loop.niters; ++c) {
        const int end = std::min(chunk_end[c], total);
        if (end <= evaluated) continue;
        if ((r = launch(evaluated, end))) return r;
        if (first_wait) {  // the staging area still holds the uploads of this call
            MVO_HIP(hipStreamSynchronize(ctx->stream));
            first_wait = false;
        }
        int32_t* h_counts = reinterpret_cast<int32_t*>(ctx->h_pin);
        MVO_HIP(hipMemcpyAsync(h_counts, d_counts + per_hyp * (size_t)evaluated, (size_t)(end - evaluated) * per_hyp * 4,
                               hipMemcpyDeviceToHost, ctx->stream));
        MVO_HIP(hipStreamSynchronize(ctx->stream));
        rec.insert(rec.end(), h_counts, h_counts + (size_t)(end - evaluated) * per_hyp);
        evaluated = end;
        loop.advance(rec.data(), evaluated, per_hyp, n, model_points, prob);
    }
    info[0] = loop.best_it;
    info[1] = loop.best_m;
    info[2] = loop.it;
    info[3] = evaluated;
    return MVO_OK;
}

// findEssentialMat(pts1, pts2, focal, pp, RANSAC, prob, threshold) on the device, shared by
// mvo_find_essential_inliers and mvo_esti_motion_by_essential.  Leaves the normalised points in d_emq, every
// hypothesis's candidates in d_em_E, the record in em_counts / em_info and, for n > 5 with a model, the RANSAC mask of
// the selected candidate in d_em_mask (launched, not yet read back).  n < 5: no model.
void reset_em_record(mvo_track_state* s) {
    s->em_counts.clear();
    s->em_info[0] = s->em_info[1] = -1;
    s->em_info[2] = s->em_info[3] = s->em_info[4] = 0;
}

int essential_ransac(mvo_ctx* ctx, const float* kp_prev, const float* kp_curr, int n, double fx, double fy, double cx,
                     double cy, double prob, double threshold) {
    mvo_track_state* s = state(ctx);
    reset_em_record(s);
    constexpr int kModel = 5, kMaxIters = 1000;  // createRANSACPointSetRegistrator(cb, 5, threshold, prob) -> maxIters 1000
    if (n < kModel) return MVO_OK;
    MVO_HIP(hipSetDevice(ctx->device));
    int r;
    if ((r = s->d_emq.ensure(ctx, (size_t)n * 4, 4096 * 4)) || (r = s->d_em_mask.ensure(ctx, n, 4096)) ||
        (r = s->d_em_subsets.ensure_exact(ctx, kMaxIters * 5)) || (r = s->d_em_nm.ensure_exact(ctx, kMaxIters)) ||
        (r = s->d_em_counts.ensure_exact(ctx, kMaxIters * 10)) || (r = s->d_em_E.ensure_exact(ctx, kMaxIters * 90)))
        return r;
    // findEssentialMat(points1, points2, focal, pp, ...): K = [focal 0 pp.x; 0 focal pp.y], pp a cv::Point2f built from
    // K(0,2), K(1,2) (epipolar_geometry.cpp:27-28); points to double, (p - c) / f; threshold /= (fx + fy) / 2
    const double focal = (fx + fy) / 2;
    const double pcx = (double)(float)cx, pcy = (double)(float)cy;
    const size_t bq = (size_t)n * 4 * sizeof(double), bs = (size_t)kMaxIters * 5 * sizeof(int32_t);
    if ((r = mvo_ensure_pinned(ctx, std::max(bq + bs, (size_t)kMaxIters * 40 + 2 * (size_t)n + 512)))) return r;
    MVO_HIP(hipStreamSynchronize(ctx->stream));
    double* q = reinterpret_cast<double*>(ctx->h_pin);
    for (int i = 0; i < n; ++i) {
        q[2 * i] = ((double)kp_prev[2 * i] - pcx) / focal;
        q[2 * i + 1] = ((double)kp_prev[2 * i + 1] - pcy) / focal;
        q[2 * (size_t)n + 2 * i] = ((double)kp_curr[2 * i] - pcx) / focal;
        q[2 * (size_t)n + 2 * i + 1] = ((double)kp_curr[2 * i + 1] - pcy) / focal;
    }
    int32_t* subsets = reinterpret_cast<int32_t*>(ctx->h_pin + bq);
    const int total = n == kModel ? 1 : kMaxIters;
    if (n == kModel)
        for (int i = 0; i < kModel; ++i) subsets[i] = i;
    else
        draw_subsets(n, kMaxIters, subsets);
    MVO_HIP(hipMemcpyAsync(s->d_emq, q, bq, hipMemcpyHostToDevice, ctx->stream));
    MVO_HIP(hipMemcpyAsync(s->d_em_subsets, subsets, (size_t)total * 5 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    const double thr = threshold / ((focal + focal) / 2);
    const float thr2 = (float)(thr * thr);
    const double* d_q1 = s->d_emq;
    const double* d_q2 = s->d_emq + 2 * (size_t)n;
    // The hypotheses are evaluated in growing chunks (a chunk costs ~0.25 ms whatever its size: one wave per hypothesis)
    const int chunk_end[2] = {256, kMaxIters};
    auto launch = [&](int begin, int end) {
        return track_launch_em_hypotheses(ctx, d_q1, d_q2, n, s->d_em_subsets + 5 * (size_t)begin, end - begin, thr2,
                                          s->d_em_E + 90 * (size_t)begin, s->d_em_nm + begin, s->d_em_counts + 10 * (size_t)begin);
    };
    if ((r = ransac_chunks(ctx, n, kModel, total, total, 10, prob, chunk_end, s->d_em_counts, launch, s->em_counts, s->em_info)))
        return r;
    const int best_it = s->em_info[0], best_m = s->em_info[1];
    if (best_it >= 0 && n != kModel)
        return track_launch_em_mask(ctx, d_q1, d_q2, n, s->d_em_E + 90 * (size_t)best_it + 9 * (size_t)best_m, thr2,
                                    s->d_em_mask);
    return MVO_OK;
}

// cv::invert(DECOMP_LU) of a 3 x 3 double matrix: for n <= 3 OpenCV takes the closed form, the adjugate times
// 1 / det3 (all zeros when det3 == 0), not the LU of larger matrices (invert_pose_lu).
void invert3(const double* M, double* out) {
    auto m = [&](int r, int c) { return M[3 * r + c]; };
    double d = m(0, 0) * (m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1)) - m(0, 1) * (m(1, 0) * m(2, 2) - m(1, 2) * m(2, 0)) +
               m(0, 2) * (m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0));
    if (d == 0.) {
        for (int k = 0; k < 9; ++k) out[k] = 0;
        return;
    }
    d = 1. / d;
    out[0] = (m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1)) * d;
    out[1] = (m(0, 2) * m(2, 1) - m(0, 1) * m(2, 2)) * d;
    out[2] = (m(0, 1) * m(1, 2) - m(0, 2) * m(1, 1)) * d;
    out[3] = (m(1, 2) * m(2, 0) - m(1, 0) * m(2, 2)) * d;
    out[4] = (m(0, 0) * m(2, 2) - m(0, 2) * m(2, 0)) * d;
    out[5] = (m(0, 2) * m(1, 0) - m(0, 0) * m(1, 2)) * d;
    out[6] = (m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0)) * d;
    out[7] = (m(0, 1) * m(2, 0) - m(0, 0) * m(2, 1)) * d;
    out[8] = (m(0, 0) * m(1, 1) - m(0, 1) * m(1, 0)) * d;
}

// C = A B (3 x 3, row-major), each entry summed k = 0..2 in order
void mul3(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double v = A[3 * i] * B[j];
            v = v + A[3 * i + 1] * B[3 + j];
            C[3 * i + j] = v + A[3 * i + 2] * B[6 + j];
        }
}

int ensure_tri(mvo_ctx* ctx, int n) {
    mvo_track_state* s = state(ctx);
    if (int r = s->d_tri_in.ensure(ctx, (size_t)n * 4, 4096 * 4)) return r;
    return s->d_tri_out.ensure(ctx, (size_t)n * 6, 4096 * 6);
}

int ensure_hd(mvo_ctx* ctx) {
    mvo_track_state* s = state(ctx);
    if (int r = s->d_hd_out.ensure_exact(ctx, kHdOut)) return r;
    return s->d_hd_cnt.ensure_exact(ctx, kHdCnt);
}

void reset_hd_record(mvo_track_state* s) {
    for (double& v : s->hd_out) v = 0;
    for (int32_t& v : s->hd_cnt) v = 0;
}

// The H that mvo_find_homography left on the device (found == 1) and its RANSAC mask (NULL: all four matches)
const double* device_h(const mvo_track_state* s, int n) { return n == 4 ? s->d_h_H + 9 * (size_t)s->h_info[0] : s->d_h_out.p; }
const uint8_t* device_h_mask(const mvo_track_state* s, int n) { return n == 4 ? nullptr : s->d_h_mask.p; }

// basics::invRt: [R t; 0 1].inv() by the LU of mvo_invert_pose (cv::Mat::inv leaves zeros for a singular matrix)
void inv_rt(double* R, double* t) {
    double T[16] = {R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2], 0, 0, 0, 1}, Ti[16];
    if (!invert_pose_lu(T, Ti, 4))
        for (double& v : Ti) v = 0;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) R[3 * i + j] = Ti[4 * i + j];
        t[i] = Ti[4 * i + 3];
    }
}

}  // namespace

void track_release(mvo_ctx* ctx) {
    delete ctx->track;
    ctx->track = nullptr;
}

// The initialisation's lifetime rule: what mvo_estimate_possible_relative_poses leaves on the device (d_sc_in, d_ip_pts,
// d_rp_out, d_hd_out, d_em_mask and the d_h_* buffers) stays valid until the next call of that family on the ctx; only such
// a call may regrow them.  The view hands those pointers out and grows nothing but d_fin.
int track_init_view(mvo_ctx* ctx, int n, int m, TrackInitView* v) {
    mvo_track_state* s = state(ctx);
    if (int r = s->d_fin.ensure(ctx, (size_t)m * 28, 1 << 16)) return r;
    v->out = s->d_fin;
    v->kp1 = reinterpret_cast<const float*>(s->d_sc_in.p);
    v->kp2 = reinterpret_cast<const float*>(s->d_sc_in + (size_t)n * 8);
    v->lists = reinterpret_cast<const int32_t*>(s->d_sc_in + (size_t)n * 16);
    v->pts = s->d_ip_pts;
    v->e_out = s->d_rp_out;
    v->h_out = s->d_hd_out;
    return MVO_OK;
}

extern "C" {

// ---------------------------------------------------------------------------------------------- map residency
int mvo_map_create(mvo_ctx* ctx, mvo_map** map) {
    if (!ctx || !map) return mvo_set_err(ctx, MVO_ERR_INVALID, "bad arguments", hipSuccess);
    *map = new mvo_map();
    return MVO_OK;
}

void mvo_map_release(mvo_ctx* ctx, mvo_map* map) {
    if (!map) return;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    delete map;
}

int mvo_map_upload(mvo_ctx* ctx, mvo_map* map, const float* pos, const uint8_t* desc, int n) {
    if (!ctx || !map || n < 0 || (n && (!pos || !desc)))
        return mvo_set_err(ctx, MVO_ERR_INVALID, "bad arguments", hipSuccess);
    MVO_HIP(hipSetDevice(ctx->device));
    const size_t n_pos = (size_t)n * 3, n_desc = (size_t)n * 32;
    int r;
    if (n_pos > map->d_pos.cap || n_desc > map->d_desc.cap) MVO_HIP(hipStreamSynchronize(ctx->stream));
    if ((r = map->d_pos.ensure(ctx, n_pos, 4096 * 3)) || (r = map->d_desc.ensure(ctx, n_desc, 4096 * 32))) return r;
    map->n = n;
    map->has_view = false;  // (mvo_map_upload_view: the view data belong to the arrays they were given for)
    if (n) {
        // staged through pinned memory so that the caller's arrays may be reused as soon as we return
        if ((r = mvo_ensure_pinned(ctx, (size_t)n * 44))) return r;
        MVO_HIP(hipStreamSynchronize(ctx->stream));
        std::memcpy(ctx->h_pin, pos, (size_t)n * 12);
        std::memcpy(ctx->h_pin + (size_t)n * 12, desc, (size_t)n * 32);
        MVO_HIP(hipMemcpyAsync(map->d_pos, ctx->h_pin, (size_t)n * 12, hipMemcpyHostToDevice, ctx->stream));
        MVO_HIP(hipMemcpyAsync(map->d_desc, ctx->h_pin + (size_t)n * 12, (size_t)n * 32, hipMemcpyHostToDevice,
                               ctx->stream));
        MVO_HIP(hipStreamSynchronize(ctx->stream));
    }
    return MVO_OK;
}

int mvo_map_update_positions(mvo_ctx* ctx, mvo_map* map, const float* pos, int first, int n) {
    if (!ctx || !map || first < 0 || n < 0 || first + n > map->n || (n && !pos))
        return mvo_set_err(ctx, MVO_ERR_INVALID, "bad arguments", hipSuccess);
    if (!n) return MVO_OK;
    MVO_HIP(hipSetDevice(ctx->device));
    int r = mvo_ensure_pinned(ctx, (size_t)n * 12);
    if (r) return r;
    MVO_HIP(hipStreamSynchronize(ctx->stream));
    std::memcpy(ctx->h_pin, pos, (size_t)n * 12);
    MVO_HIP(hipMemcpyAsync(map->d_pos + 3 * (size_t)first, ctx->h_pin, (size_t)n * 12, hipMemcpyHostToDevice,
                           ctx->stream));
    MVO_HIP(hipStreamSynchronize(ctx->stream));
    return MVO_OK;
}

int mvo_map_points_in_view(mvo_ctx* ctx, mvo_map* map, const double* T_w_c, double fx, double fy, double cx, double cy,
                           int cols, int rows, int32_t* idx, float* px, int cap, int* n, const void** d_desc_out) {
    if (!ctx || !map || !T_w_c || !n || cap < 0 || (cap && (!idx || !px)))
        return mvo_set_err(ctx, MVO_ERR_INVALID, "bad arguments", hipSuccess);
    *n = 0;
    if (d_desc_out) *d_desc_out = nullptr;
    TrackViewArgs a;
    if (!invert_pose_lu(T_w_c, a.T)) return mvo_set_err(ctx, MVO_ERR_INVALID, "T_w_c is singular", hipSuccess);
    a.fx = fx;
    a.fy = fy;
    a.cx = cx;
    a.cy = cy;
    a.cols = cols;
    a.rows = rows;
    if (map->n == 0) return MVO_OK;
    MVO_HIP(hipSetDevice(ctx->device));
    mvo_track_state* s = state(ctx);
    int r;
    if ((r = s->d_view_desc.ensure(ctx, (size_t)map->n * 32, 4096 * 32)) || (r = s->d_view_n.ensure_exact(ctx, 1))) return r;
    // the kernel writes the count, the indices and the pixels straight into the pinned buffer (the descriptors of the survivors
    // stay in HBM for the matcher): one synchronisation, no copy
    if ((r = mvo_ensure_pinned(ctx, 192 + (size_t)map->n * 12))) return r;
    MVO_HIP(hipStreamSynchronize(ctx->stream));  // (nothing of an earlier call may still be reading the staging buffer)
    int32_t* h_n = reinterpret_cast<int32_t*>(ctx->h_pin);
    int32_t* h_idx = reinterpret_cast<int32_t*>(ctx->h_pin + 64);
    float* h_px = reinterpret_cast<float*>(ctx->h_pin + 64 + ((size_t)map->n * 4 + 63) / 64 * 64);  // (float2 stores)
    if ((r = track_launch_map_in_view(ctx, map->d_pos, map->d_desc, map->n, a, h_idx, h_px, s->d_view_desc, h_n))) return r;
    MVO_HIP(hipStreamSynchronize(ctx->stream));
    const int cnt = *h_n;
    *n = cnt;
    if (d_desc_out) *d_desc_out = s->d_view_desc;
    if (ctx->prof) mvo_prof_collect(ctx);
    if (cnt > cap) return mvo_set_err(ctx, MVO_ERR_CAPACITY, "mvo_map_points_in_view: output buffers too small", hipSuccess);
    if (cnt) {
        std::memcpy(idx, h_idx, (size_t)cnt * 4);
        std::memcpy(px, h_px, (size_t)cnt * 8);
    }
    return MVO_OK;
}

// ---------------------------------------------------------------------------------------------- solvePnPRansac
int mvo_solve_pnp_ransac(mvo_ctx* ctx, const float* pts3d, const float* pts2d, int n, double fx, double fy, double cx,
                         double cy, int iterations, float reprojection_error, double confidence, double* rvec,
                         double* tvec, int32_t* inliers, int cap, int* n_inliers, int* found) {
    if (!ctx || n < 0 || (n && (!pts3d || !pts2d)) || !rvec || !tvec || !n_inliers || !found || cap < 0 ||
        (cap && !inliers))
        return mvo_set_err(ctx, MVO_ERR_INVALID, "bad arguments", hipSuccess);
    if (!(confidence > 0 && confidence < 1))  // CV_Assert in RANSACPointSetRegistrator::run
        return mvo_set_err(ctx, MVO_ERR_INVALID, "mvo_solve_pnp_ransac: confidence must be in (0, 1)", hipSuccess);
    *n_inliers = 0;
    *found = 0;
    for (int k = 0; k < 3; ++k) rvec[k] = tvec[k] = 0;
    constexpr int kModel = 5;
    mvo_track_state* s = state(ctx);
    s->models.clear();
    s->counts.clear();
    s->info[0] = -1;
    for (int k = 1; k < 6; ++k) s->info[k] = 0;
    if (n < kModel) return MVO_OK;  // vo.cpp:321 (kMinPtsForPnP) never gets here; solvePnPRansac would reject it
    if (cap < n) return mvo_set_err(ctx, MVO_ERR_CAPACITY, "mvo_solve_pnp_ransac: inlier buffer smaller than n", hipSuccess);
    const int n_hyp = n == kModel ? 1 : std::max(iterations, 1);
    MVO_HIP(hipSetDevice(ctx->device));
    int r = ensure_pnp(ctx, n, n_hyp);
    if (r) return r;
    // stage pairs + subsets: ONE upload; the kernels deliver their results into the pinned buffer themselves (models and
    // counts by the hypothesis kernel, the refined pose and the inlier mask by the refinement kernel): no copy comes back
    const size_t b3 = (size_t)n * 12, b2 = (size_t)n * 8, bs = (size_t)n_hyp * kModel * 4;
    const size_t o_out = (b3 + b2 + bs + 63) / 64 * 64, o_counts = o_out + 128, o_models = o_counts + ((size_t)n_hyp * 4 + 63) / 64 * 64,
                 o_mask = o_models + (size_t)n_hyp * 96;
    if ((r = mvo_ensure_pinned(ctx, o_mask + (size_t)n + 64))) return r;
    MVO_HIP(hipStreamSynchronize(ctx->stream));
    std::memcpy(ctx->h_pin, pts3d, b3);
    std::memcpy(ctx->h_pin + b3, pts2d, b2);
    int32_t* subsets = reinterpret_cast<int32_t*>(ctx->h_pin + b3 + b2);
    if (n == kModel)
        for (int i = 0; i < kModel; ++i) subsets[i] = i;
    else
        draw_subsets(n, n_hyp, subsets);
    MVO_HIP(hipMemcpyAsync(s->d_in, ctx->h_pin, b3 + b2 + bs, hipMemcpyHostToDevice, ctx->stream));
    const float* d_p3 = reinterpret_cast<const float*>(s->d_in.p);
    const float* d_p2 = reinterpret_cast<const float*>(s->d_in + b3);
    const int32_t* d_subsets = reinterpret_cast<const int32_t*>(s->d_in + b3 + b2);
    uint8_t* h_out = ctx->h_pin + o_out;
    uint8_t* h_counts = ctx->h_pin + o_counts;
    uint8_t* h_models = ctx->h_pin + o_models;
    uint8_t* h_mask = ctx->h_pin + o_mask;
    const TrackCamera cam{fx, fy, cx, cy};
    const float thr2 = (float)((double)reprojection_error * (double)reprojection_error);
    // How many hypotheses go first.  The sequential loop of RANSACPointSetRegistrator::run shortens itself as soon as a good model
    // turns up (three quarters of the pairs inliers: ~27 of the 100 iterations) -- a lone sequence evaluates all `iterations`
    // hypotheses at once anyway (they run side by side: the price of one), but where many sequences share the GPU a hypothesis is
    // 200 us of a CU: contexts in THROUGHPUT / SHARED mode evaluate the first 32, let the replay of the loop's bookkeeping say
    // whether the loop would have gone on, and only then launch the rest (one more round trip in that case).  The result is what
    // the sequential loop produces either way.  MVO_PNP_CHUNK: 0 = never, n > 0 = first n for every ctx (A/B).
    // A sequence whose loop ran long last time (few inliers among its pairs: the loop needs all its iterations) gets all hypotheses
    // at once again -- two chunks would only add a round trip and a second refinement; the inlier ratio of a sequence changes slowly
    // from frame to frame.  (Measured with 32 sequences: +8 % frames/s where the loop stops after ~27 iterations, -23 % where it
    // always needs 100 and the chunks were used blindly.)
    static const int env_chunk = std::getenv("MVO_PNP_CHUNK") ? std::atoi(std::getenv("MVO_PNP_CHUNK")) : -1;
    const bool chunked = n != kModel && n_hyp > 48 &&
                         (env_chunk >= 0 ? env_chunk > 0 : (ctx->ba_throughput_mode != 0 && s->last_loop_len > 0 && s->last_loop_len <= 28));
    const int first = chunked ? std::min(n_hyp, env_chunk > 0 ? env_chunk : 32) : n_hyp;
    if ((r = track_launch_pnp_hypotheses(ctx, d_p3, d_p2, n, d_subsets, first, cam, thr2, s->d_models, s->d_counts, s->d_masks,
                                         reinterpret_cast<double*>(h_models), reinterpret_cast<int32_t*>(h_counts))))
        return r;
    // The refinement kernel replays the sequential bookkeeping of RANSACPointSetRegistrator::run over the counts and
    // refines the model it selects; the host repeats the replay (its own libm) on the counts that come back with
    // the result and only launches again if it disagrees -- one host round trip per call.
    const int mode = n == kModel ? 1 : 0;
    const double dev_conf = g_pnp_replay_skew ? 0.5 : confidence;
    if ((r = track_launch_pnp_refine(ctx, d_p3, d_p2, s->d_masks, n, cam, s->d_models, s->d_counts, first, dev_conf,
                                     mode == 1 ? 0 : -1, mode, s->d_Mg, s->d_mg, h_mask, reinterpret_cast<double*>(h_out))))
        return r;
    auto fetch = [&]() -> int {
        MVO_HIP(hipStreamSynchronize(ctx->stream));
        return MVO_OK;
    };
    if ((r = fetch())) return r;
    int evaluated = first;
    int best = -1;
    if (mode == 1) {  // "model_points == npoints": the kernel result is the answer and every pair an inlier
        best = 0;
        s->info[1] = 1;
    } else {
        // the loop's bookkeeping with its own bound (n_hyp), over the counts that exist so far
        RansacLoop loop{n_hyp};
        for (;;) {
            loop.advance(reinterpret_cast<const int32_t*>(h_counts), evaluated, 1, n, kModel, confidence);
            if (loop.it >= loop.niters || evaluated >= n_hyp) break;
            // the sequential loop goes on behind the first chunk: the remaining hypotheses, then the refinement over all counts
            if ((r = track_launch_pnp_hypotheses(ctx, d_p3, d_p2, n, d_subsets + (size_t)kModel * evaluated, n_hyp - evaluated, cam, thr2,
                                                 s->d_models + 12 * (size_t)evaluated, s->d_counts + evaluated, s->d_masks + (size_t)evaluated * n,
                                                 reinterpret_cast<double*>(h_models) + 12 * (size_t)evaluated,
                                                 reinterpret_cast<int32_t*>(h_counts) + evaluated)))
                return r;
            if ((r = track_launch_pnp_refine(ctx, d_p3, d_p2, s->d_masks, n, cam, s->d_models, s->d_counts, n_hyp, dev_conf, -1, mode,
                                             s->d_Mg, s->d_mg, h_mask, reinterpret_cast<double*>(h_out))))
                return r;
            if ((r = fetch())) return r;
            evaluated = n_hyp;
        }
        best = loop.best_it;
        s->info[1] = s->last_loop_len = loop.it;
    }
    s->counts.assign(reinterpret_cast<int32_t*>(h_counts), reinterpret_cast<int32_t*>(h_counts) + evaluated);
    s->models.resize((size_t)evaluated * 12);
    std::memcpy(s->models.data(), h_models, (size_t)evaluated * 96);
    s->info[5] = evaluated;
    s->info[0] = best;
    double out[12];
    std::memcpy(out, h_out, sizeof(out));
    if (best >= 0 && (int)out[10] != best) {  // the device's replay chose differently: refine the right hypothesis
        s->info[5] = -evaluated;              // (visible to tests through mvo_debug_get_pnp)
        if ((r = track_launch_pnp_refine(ctx, d_p3, d_p2, s->d_masks, n, cam, s->d_models, s->d_counts, evaluated,
                                         confidence, best, mode, s->d_Mg, s->d_mg, h_mask, reinterpret_cast<double*>(h_out))))
            return r;
        if ((r = fetch())) return r;
        std::memcpy(out, h_out, sizeof(out));
    }
    if (ctx->prof) mvo_prof_collect(ctx);
    if (best < 0) return MVO_OK;  // no model with at least 5 inliers
    for (int k = 0; k < 3; ++k) {
        rvec[k] = out[k];
        tvec[k] = out[3 + k];
    }
    s->info[2] = (int)out[7];
    s->info[3] = (int)out[8];
    s->info[4] = (int)out[9];
    int cnt = 0;
    if (mode == 1) {
        for (int i = 0; i < n; ++i) inliers[cnt++] = i;
    } else {
        for (int i = 0; i < n; ++i)
            if (h_mask[i]) inliers[cnt++] = i;
    }
    *n_inliers = cnt;
    *found = 1;
    return MVO_OK;
}

// ---------------------------------------------------------------------------------------------- keyframe row
int mvo_triangulate_points(mvo_ctx* ctx, const float* kp_prev, const float* kp_curr, int n, double fx, double fy, double cx,
                           double cy, const double* R, const double* t, float* pts3d_in_prev, float* pts3d_in_curr) {
    if (!ctx || n < 0 || !R || !t || (n && (!kp_prev || !kp_curr || (!pts3d_in_prev && !pts3d_in_curr))))
        return mvo_set_err(ctx, MVO_ERR_INVALID, "bad arguments", hipSuccess);
    if (n == 0) return MVO_OK;
    MVO_HIP(hipSetDevice(ctx->device));
    mvo_track_state* s = state(ctx);
    int r = ensure_tri(ctx, n);
    if (r) return r;
    r = mvo_ensure_pinned(ctx, (size_t)n * 24);
    if (r) return r;
    MVO_HIP(hipStreamSynchronize(ctx->stream));
    std::memcpy(ctx->h_pin, kp_prev, (size_t)n * 8);
    std::memcpy(ctx->h_pin + (size_t)n * 8, kp_curr, (size_t)n * 8);
    MVO_HIP(hipMemcpyAsync(s->d_tri_in, ctx->h_pin, (size_t)n * 16, hipMemcpyHostToDevice, ctx->stream));
    const TrackCamera cam{fx, fy, cx, cy};
    if ((r = track_launch_triangulate(ctx, s->d_tri_in, s->d_tri_in + 2 * (size_t)n, n, cam, R, t, s->d_tri_out,
                                      s->d_tri_out + 3 * (size_t)n)))
        return r;
    MVO_HIP(hipMemcpyAsync(ctx->h_pin, s->d_tri_out, (size_t)n * 24, hipMemcpyDeviceToHost, ctx->stream));
    MVO_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->prof) mvo_prof_collect(ctx);
    if (pts3d_in_prev) std::memcpy(pts3d_in_prev, ctx->h_pin, (size_t)n * 12);
    if (pts3d_in_curr) std::memcpy(pts3d_in_curr, ctx->h_pin + (size_t)n * 12, (size_t)n * 12);
    return MVO_OK;
}

// geometry::helperFindInlierMatchesByEpipolarCons = the inlier mask of cv::findEssentialMat(RANSAC)
int mvo_find_essential_inliers(mvo_ctx* ctx, const float* kp_prev, const float* kp_curr, int n, double fx, double fy,
                               double cx, double cy, double prob, double threshold, int32_t* inliers, int cap,
                               int* n_inliers) {
    if (!ctx || n < 0 || !n_inliers || cap < 0 || (n && (!kp_prev || !kp_curr)) || (cap && !inliers))
        return mvo_set_err(ctx, MVO_ERR_INVALID, "bad arguments", hipSuccess);
    if (!(prob > 0 && prob < 1))
        return mvo_set_err(ctx, MVO_ERR_INVALID, "mvo_find_essential_inliers: prob must be in (0, 1)", hipSuccess);
    *n_inliers = 0;
    reset_em_record(state(ctx));
    if (n >= 5 && cap < n)
        return mvo_set_err(ctx, MVO_ERR_CAPACITY, "mvo_find_essential_inliers: inlier buffer smaller than n", hipSuccess);
    int r = essential_ransac(ctx, kp_prev, kp_curr, n, fx, fy, cx, cy, prob, threshold);
    if (r) return r;
    mvo_track_state* s = state(ctx);
    if (s->em_info[0] < 0) {
        if (ctx->prof) mvo_prof_collect(ctx);
        return MVO_OK;
    }
    int cnt = 0;
    if (n == 5) {
        for (int i = 0; i < n; ++i) inliers[cnt++] = i;
    } else {
        MVO_HIP(hipMemcpyAsync(ctx->h_pin, s->d_em_mask, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        MVO_HIP(hipStreamSynchronize(ctx->stream));
        for (int i = 0; i < n; ++i)
            if (ctx->h_pin[i]) inliers[cnt++] = i;
    }
    if (ctx->prof) mvo_prof_collect(ctx);
    *n_inliers = cnt;
    return MVO_OK;
}

// estiMotionByEssential (epipolar_geometry.cpp:17-57): findEssentialMat as above, E /= E(2,2), the inlier list
// from the RANSAC mask, recoverPose(E, pts1, pts2, R, t, focal, pp, mask), t / |t|.  E stays on the device
// between the RANSAC and k_recover_pose; one read-back brings the result, the counts and the masks.
int mvo_esti_motion_by_essential(mvo_ctx* ctx, const float* pts1, const float* pts2, int n, double fx, double fy,
                                 double cx, double cy, double prob, double threshold, double* E, double* R, double* t,
                                 int32_t* inliers, int cap, int* n_inliers, int* found) {
    if (!ctx || n < 0 || !E || !R || !t || !n_inliers || !found || cap < 0 || (n && (!pts1 || !pts2)) ||
        (cap && !inliers))
        return mvo_set_err(ctx, MVO_ERR_INVALID, "bad arguments", hipSuccess);
    if (!(prob > 0 && prob < 1))
        return mvo_set_err(ctx, MVO_ERR_INVALID, "mvo_esti_motion_by_essential: prob must be in (0, 1)", hipSuccess);
    *n_inliers = 0;
    *found = 0;
    for (int k = 0; k < 9; ++k) E[k] = R[k] = 0;
    for (int k = 0; k < 3; ++k) t[k] = 0;
    mvo_track_state* s = state(ctx);
    s->rp_n = 0;
    s->rp_chosen = -1;
    for (int k = 0; k < 4; ++k) s->rp_good[k] = 0;
    for (int k = 0; k < 21; ++k) s->rp_R1R2t[k] = 0;
    reset_em_record(s);
    if (n >= 5 && cap < n)
        return mvo_set_err(ctx, MVO_ERR_CAPACITY, "mvo_esti_motion_by_essential: inlier buffer smaller than n", hipSuccess);
    int r = essential_ransac(ctx, pts1, pts2, n, fx, fy, cx, cy, prob, threshold);
    if (r) return r;
    const int best_it = s->em_info[0], best_m = s->em_info[1];
    // n == 5 with several candidates: findEssentialMat returns them stacked (3k x 3) and decomposeEssentialMat asserts
    // (deviation 7): no model
    int n_candidates = 0;
    if (n == 5 && !s->em_counts.empty())
        for (int m = 0; m < 10; ++m) n_candidates += s->em_counts[m] >= 0;
    if (best_it < 0 || n_candidates > 1) {
        if (ctx->prof) mvo_prof_collect(ctx);
        return MVO_OK;
    }
    if ((r = s->d_rp_masks.ensure(ctx, n, 4096)) || (r = s->d_rp_out.ensure_exact(ctx, 48)) || (r = s->d_rp_cnt.ensure_exact(ctx, 8)))
        return r;
    const double* d_q1 = s->d_emq;
    const double* d_q2 = s->d_emq + 2 * (size_t)n;
    if ((r = track_launch_recover_pose(ctx, d_q1, d_q2, n, s->d_em_E + 90 * (size_t)best_it + 9 * (size_t)best_m,
                                       n == 5 ? nullptr : s->d_em_mask, s->d_rp_masks, s->d_rp_cnt, s->d_rp_out)))
        return r;
    // staging: out (42 doubles), counts (6 ints), the recoverPose masks (n), the RANSAC mask (n)
    double* h_out = reinterpret_cast<double*>(ctx->h_pin);
    int32_t* h_cnt = reinterpret_cast<int32_t*>(ctx->h_pin + 384);
    uint8_t* h_masks = ctx->h_pin + 448;
    uint8_t* h_ransac = h_masks + n;
    MVO_HIP(hipMemcpyAsync(h_out, s->d_rp_out, 42 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MVO_HIP(hipMemcpyAsync(h_cnt, s->d_rp_cnt, 6 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    MVO_HIP(hipMemcpyAsync(h_masks, s->d_rp_masks, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (n > 5) MVO_HIP(hipMemcpyAsync(h_ransac, s->d_em_mask, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    MVO_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->prof) mvo_prof_collect(ctx);
    int cnt = 0;
    for (int i = 0; i < n; ++i)
        if (n == 5 || h_ransac[i]) inliers[cnt++] = i;
    for (int k = 0; k < 9; ++k) {
        E[k] = h_out[k];
        R[k] = h_out[9 + k];
    }
    for (int k = 0; k < 3; ++k) t[k] = h_out[18 + k];
    std::memcpy(s->rp_R1R2t, h_out + 21, sizeof(s->rp_R1R2t));
    std::memcpy(s->rp_good, h_cnt, sizeof(s->rp_good));
    s->rp_chosen = h_cnt[5];
    s->rp_masks.assign(h_masks, h_masks + n);
    s->rp_n = n;
    *n_inliers = cnt;
    *found = 1;
    return MVO_OK;
}

int mvo_debug_get_recover_pose(mvo_ctx* ctx, int32_t* good, int32_t* chosen, double* R1R2t, uint8_t* masks, int cap) {
    if (!ctx || !ctx->track) return mvo_set_err(ctx, MVO_ERR_STATE, "no recoverPose call on this ctx yet", hipSuccess);
    const mvo_track_state* s = ctx->track;
    if (good) std::memcpy(good, s->rp_good, sizeof(s->rp_good));
    if (chosen) *chosen = s->rp_chosen;
    if (R1R2t) std::memcpy(R1R2t, s->rp_R1R2t, sizeof(s->rp_R1R2t));
    if (s->rp_n > cap) return mvo_set_err(ctx, MVO_ERR_CAPACITY, "mvo_debug_get_recover_pose: buffer too small", hipSuccess);
    if (masks && s->rp_n) std::memcpy(masks, s->rp_masks.data(), (size_t)s->rp_n);
    return s->rp_n;
}

// checkEssentialScore + checkHomographyScore (motion_estimation.cpp:501-664) with their 3 x 3 set-up on the host:
// K.inv() and H21.inv() by cv::invert's closed form for n <= 3 (invert3), F21 = (Kinv^T E) Kinv.
int mvo_check_init_scores(mvo_ctx* ctx, const float* pts1, const float* pts2, int n, double fx, double fy, double cx,
                          double cy, const double* E, const int32_t* inl_e, int n_e, const double* H,
                          const int32_t* inl_h, int n_h, double sigma, double* score_e, double* score_h, int32_t* kept_e,
                          int* n_kept_e, int32_t* kept_h, int* n_kept_h) {
    if (!ctx || n < 0 || n_e < 0 || n_h < 0 || !score_e || !score_h || !n_kept_e || !n_kept_h ||
        (n && (!pts1 || !pts2)) || (E && n_e && (!inl_e || !kept_e)) || (H && n_h && (!inl_h || !kept_h)))
        return mvo_set_err(ctx, MVO_ERR_INVALID, "bad arguments", hipSuccess);
    const int me = E ? n_e : 0, mh = H ? n_h : 0;
    for (int i = 0; i < me; ++i)
        if (inl_e[i] < 0 || inl_e[i] >= n) return mvo_set_err(ctx, MVO_ERR_INVALID, "mvo_check_init_scores: E list index out of range", hipSuccess);
    for (int i = 0; i < mh; ++i)
        if (inl_h[i] < 0 || inl_h[i] >= n) return mvo_set_err(ctx, MVO_ERR_INVALID, "mvo_check_init_scores: H list index out of range", hipSuccess);
    *score_e = *score_h = 0;
    *n_kept_e = *n_kept_h = 0;
    if (me + mh == 0) return MVO_OK;
    InitScoreArgs a{};
    a.inv_s2 = 1.0 / (sigma * sigma);
    a.has_e = E ? 1 : 0;
    a.has_h = H ? 1 : 0;
    if (E) {
        const double K[9] = {fx, 0, cx, 0, fy, cy, 0, 0, 1};
        double Ki[9], KiT[9], T[9];
        invert3(K, Ki);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) KiT[3 * i + j] = Ki[3 * j + i];
        mul3(KiT, E, T);
        mul3(T, Ki, a.f);
    }
    if (H) {
        for (int k = 0; k < 9; ++k) a.h[k] = H[k];
        invert3(H, a.hi);
    }
    MVO_HIP(hipSetDevice(ctx->device));
    mvo_track_state* s = state(ctx);
    const size_t bp = (size_t)n * 16, bl = (size_t)(me + mh) * 4;
    int r;
    if ((r = s->d_sc_in.ensure(ctx, bp + bl, 1 << 16)) || (r = s->d_sc_kept.ensure(ctx, me + mh, 4096)) ||
        (r = s->d_sc_out.ensure_exact(ctx, 64)))
        return r;
    const size_t o_out = (bp + bl + 63) / 64 * 64;
    if ((r = mvo_ensure_pinned(ctx, o_out + 64 + (size_t)(me + mh) * 4))) return r;
    MVO_HIP(hipStreamSynchronize(ctx->stream));
    std::memcpy(ctx->h_pin, pts1, (size_t)n * 8);
    std::memcpy(ctx->h_pin + (size_t)n * 8, pts2, (size_t)n * 8);
    if (me) std::memcpy(ctx->h_pin + bp, inl_e, (size_t)me * 4);
    if (mh) std::memcpy(ctx->h_pin + bp + (size_t)me * 4, inl_h, (size_t)mh * 4);
    MVO_HIP(hipMemcpyAsync(s->d_sc_in, ctx->h_pin, bp + bl, hipMemcpyHostToDevice, ctx->stream));
    const float* d_p1 = reinterpret_cast<const float*>(s->d_sc_in.p);
    const float* d_p2 = reinterpret_cast<const float*>(s->d_sc_in + (size_t)n * 8);
    const int32_t* d_lists = reinterpret_cast<const int32_t*>(s->d_sc_in + bp);
    double* d_scores = reinterpret_cast<double*>(s->d_sc_out.p);
    int32_t* d_nk = reinterpret_cast<int32_t*>(s->d_sc_out + 16);
    if ((r = track_launch_init_scores(ctx, d_p1, d_p2, d_lists, me, mh, a, d_scores, s->d_sc_kept, d_nk))) return r;
    uint8_t* h_out = ctx->h_pin + o_out;
    int32_t* h_kept = reinterpret_cast<int32_t*>(h_out + 64);
    MVO_HIP(hipMemcpyAsync(h_out, s->d_sc_out, 24, hipMemcpyDeviceToHost, ctx->stream));
    MVO_HIP(hipMemcpyAsync(h_kept, s->d_sc_kept, (size_t)(me + mh) * 4, hipMemcpyDeviceToHost, ctx->stream));
    MVO_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->prof) mvo_prof_collect(ctx);
    const double* sc = reinterpret_cast<const double*>(h_out);
    const int32_t* nk = reinterpret_cast<const int32_t*>(h_out + 16);
    *score_e = sc[0];
    *score_h = sc[1];
    *n_kept_e = nk[0];
    *n_kept_h = nk[1];
    if (nk[0]) std::memcpy(kept_e, h_kept, (size_t)nk[0] * 4);
    if (nk[1]) std::memcpy(kept_h, h_kept + me, (size_t)nk[1] * 4);
    return MVO_OK;
}

int mvo_debug_get_essential(mvo_ctx* ctx, int32_t* counts, int cap_iters, int32_t* info) {
    if (!ctx || !ctx->track) return mvo_set_err(ctx, MVO_ERR_STATE, "no essential-matrix call on this ctx yet", hipSuccess);
    const mvo_track_state* s = ctx->track;
    const int iters = (int)(s->em_counts.size() / 10);
    if (info) std::memcpy(info, s->em_info, sizeof(s->em_info));
    if (iters > cap_iters) return mvo_set_err(ctx, MVO_ERR_CAPACITY, "mvo_debug_get_essential: buffer too small", hipSuccess);
    if (counts && iters) std::memcpy(counts, s->em_counts.data(), s->em_counts.size() * 4);
    return iters;
}

// ---------------------------------------------------------------------------------------------- initialisation
// cv::findHomography(src, dst, RANSAC, threshold, noArray(), maxIters 2000, confidence) as estiMotionByHomography
// calls it: n < 4 -> no model; n == 4 -> runKernel on the four matches, all inliers; otherwise the RANSAC loop
// (getSubset with checkSubset, one wave per hypothesis on the device) and, when it found a model, the DLT re-fit on
// its inliers followed by the Levenberg-Marquardt refinement (k_h_refine).  The mask stays RANSAC's mask.
int mvo_find_homography(mvo_ctx* ctx, const float* src, const float* dst, int n, double threshold, double confidence,
                        double* H, int32_t* inliers, int cap, int* n_inliers, int* found) {
    if (!ctx || n < 0 || !H || !n_inliers || !found || cap < 0 || (n && (!src || !dst)) || (cap && !inliers))
        return mvo_set_err(ctx, MVO_ERR_INVALID, "bad arguments", hipSuccess);
    if (!(confidence > 0 && confidence < 1))
        return mvo_set_err(ctx, MVO_ERR_INVALID, "mvo_find_homography: confidence must be in (0, 1)", hipSuccess);
    *n_inliers = 0;
    *found = 0;
    for (int k = 0; k < 9; ++k) H[k] = 0;
    mvo_track_state* s = state(ctx);
    s->h_counts.clear();
    s->h_info[0] = -1;
    for (int k = 1; k < 6; ++k) s->h_info[k] = 0;
    constexpr int kModel = 4, kMaxIters = 2000;
    if (n < kModel) return MVO_OK;
    if (cap < n) return mvo_set_err(ctx, MVO_ERR_CAPACITY, "mvo_find_homography: inlier buffer smaller than n", hipSuccess);
    if (threshold <= 0) threshold = 3;  // findHomography's defaultRANSACReprojThreshold
    MVO_HIP(hipSetDevice(ctx->device));
    int r;
    if ((r = s->d_hpts.ensure(ctx, (size_t)n * 4, 4096 * 4)) || (r = s->d_h_mask.ensure(ctx, n, 4096)) ||
        (r = s->d_h_subsets.ensure_exact(ctx, kMaxIters * 4)) || (r = s->d_h_counts.ensure_exact(ctx, kMaxIters)) ||
        (r = s->d_h_H.ensure_exact(ctx, kMaxIters * 9)) || (r = s->d_h_out.ensure_exact(ctx, 16)))
        return r;
    const size_t bp = (size_t)n * 16, bs = (size_t)kMaxIters * 4 * sizeof(int32_t);
    if ((r = mvo_ensure_pinned(ctx, std::max(bp + bs, (size_t)kMaxIters * 4 + (size_t)n + 256)))) return r;
    MVO_HIP(hipStreamSynchronize(ctx->stream));
    std::memcpy(ctx->h_pin, src, (size_t)n * 8);
    std::memcpy(ctx->h_pin + (size_t)n * 8, dst, (size_t)n * 8);
    int32_t* subsets = reinterpret_cast<int32_t*>(ctx->h_pin + bp);
    int total = 1;
    if (n == kModel)
        for (int i = 0; i < kModel; ++i) subsets[i] = i;
    else
        total = draw_h_subsets(src, dst, n, kMaxIters, subsets);
    s->h_info[3] = total;
    if (total == 0) return MVO_OK;  // getSubset gave up at the first iteration: findHomography fails
    MVO_HIP(hipMemcpyAsync(s->d_hpts, ctx->h_pin, bp, hipMemcpyHostToDevice, ctx->stream));
    MVO_HIP(hipMemcpyAsync(s->d_h_subsets, subsets, (size_t)total * 4 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    const float* d_src = s->d_hpts;
    const float* d_dst = s->d_hpts + 2 * (size_t)n;
    const float thr2 = (float)(threshold * threshold);
    const int chunk_end[2] = {256, kMaxIters};
    auto launch = [&](int begin, int end) {
        return track_launch_h_hypotheses(ctx, d_src, d_dst, n, s->d_h_subsets + 4 * (size_t)begin, end - begin, thr2,
                                         s->d_h_H + 9 * (size_t)begin, s->d_h_counts + begin);
    };
    int32_t info[4];
    if ((r = ransac_chunks(ctx, n, kModel, total, n == kModel ? 1 : kMaxIters, 1, confidence, chunk_end, s->d_h_counts,
                           launch, s->h_counts, info)))
        return r;
    const int best = info[0];
    s->h_info[0] = best;
    s->h_info[1] = info[2];
    s->h_info[2] = info[3];
    if (best < 0) {
        if (ctx->prof) mvo_prof_collect(ctx);
        return MVO_OK;
    }
    double* h_out = reinterpret_cast<double*>(ctx->h_pin);
    uint8_t* h_mask = ctx->h_pin + 128;
    int cnt = 0;
    if (n == kModel) {
        MVO_HIP(hipMemcpyAsync(h_out, s->d_h_H + 9 * (size_t)best, 9 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        MVO_HIP(hipStreamSynchronize(ctx->stream));
        for (int i = 0; i < n; ++i) inliers[cnt++] = i;
    } else {
        if ((r = track_launch_h_mask(ctx, d_src, d_dst, n, s->d_h_H + 9 * (size_t)best, thr2, s->d_h_mask))) return r;
        if ((r = track_launch_h_refine(ctx, d_src, d_dst, s->d_h_mask, n, s->d_h_H + 9 * (size_t)best, s->d_h_out))) return r;
        MVO_HIP(hipMemcpyAsync(h_out, s->d_h_out, 11 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        MVO_HIP(hipMemcpyAsync(h_mask, s->d_h_mask, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        MVO_HIP(hipStreamSynchronize(ctx->stream));
        for (int i = 0; i < n; ++i)
            if (h_mask[i]) inliers[cnt++] = i;
        s->h_info[4] = (int32_t)h_out[9];
        s->h_info[5] = (int32_t)h_out[10];
    }
    for (int k = 0; k < 9; ++k) H[k] = h_out[k];
    if (ctx->prof) mvo_prof_collect(ctx);
    *n_inliers = cnt;
    *found = 1;
    return MVO_OK;
}

int mvo_debug_get_homography(mvo_ctx* ctx, int32_t* counts, int cap_iters, int32_t* info) {
    if (!ctx || !ctx->track) return mvo_set_err(ctx, MVO_ERR_STATE, "no homography call on this ctx yet", hipSuccess);
    const mvo_track_state* s = ctx->track;
    const int iters = (int)s->h_counts.size();
    if (info) std::memcpy(info, s->h_info, sizeof(s->h_info));
    if (iters > cap_iters) return mvo_set_err(ctx, MVO_ERR_CAPACITY, "mvo_debug_get_homography: buffer too small", hipSuccess);
    if (counts && iters) std::memcpy(counts, s->h_counts.data(), (size_t)iters * 4);
    return iters;
}

// estiMotionByHomography + removeWrongRtOfHomography (epipolar_geometry.cpp:59-128): mvo_find_homography, then
// k_h_decompose on the H and mask it left on the device; one read-back brings H / H(2,2), the decomposition, the
// rejection counts and the survivors.
int mvo_esti_motion_by_homography(mvo_ctx* ctx, const float* pts1, const float* pts2, int n, double fx, double fy,
                                  double cx, double cy, double threshold, double confidence, double* H,
                                  int32_t* inliers, int cap, int* n_inliers, double* Rs, double* ts, double* normals,
                                  int* n_solutions, int* found) {
    if (!ctx || !Rs || !ts || !normals || !n_solutions) return mvo_set_err(ctx, MVO_ERR_INVALID, "bad arguments", hipSuccess);
    *n_solutions = 0;
    for (int k = 0; k < 36; ++k) Rs[k] = 0;
    for (int k = 0; k < 12; ++k) ts[k] = normals[k] = 0;
    reset_hd_record(state(ctx));
    int r = mvo_find_homography(ctx, pts1, pts2, n, threshold, confidence, H, inliers, cap, n_inliers, found);
    if (r || !*found) return r;
    mvo_track_state* s = state(ctx);
    if ((r = ensure_hd(ctx))) return r;
    const TrackCamera cam{fx, fy, cx, cy};
    if ((r = track_launch_h_decompose(ctx, s->d_hpts, s->d_hpts + 2 * (size_t)n, device_h_mask(s, n), n, device_h(s, n), cam,
                                      s->d_hd_cnt, s->d_hd_out)))
        return r;
    double* h_out = reinterpret_cast<double*>(ctx->h_pin);
    int32_t* h_cnt = reinterpret_cast<int32_t*>(ctx->h_pin + kHdOut * sizeof(double));
    MVO_HIP(hipMemcpyAsync(h_out, s->d_hd_out, kHdOut * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MVO_HIP(hipMemcpyAsync(h_cnt, s->d_hd_cnt, kHdCnt * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    MVO_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->prof) mvo_prof_collect(ctx);
    std::memcpy(s->hd_out, h_out, sizeof(s->hd_out));
    std::memcpy(s->hd_cnt, h_cnt, sizeof(s->hd_cnt));
    for (int k = 0; k < 9; ++k) H[k] = s->hd_out[kHdHs + k];
    const int k_surv = s->hd_cnt[7];
    for (int j = 0; j < k_surv; ++j) {
        const int c = s->hd_cnt[8 + j];
        for (int k = 0; k < 9; ++k) Rs[9 * j + k] = s->hd_out[kHdR + 9 * c + k];
        for (int k = 0; k < 3; ++k) {
            ts[3 * j + k] = s->hd_out[kHdTn + 3 * c + k];
            normals[3 * j + k] = s->hd_out[kHdN + 3 * c + k];
        }
    }
    *n_solutions = k_surv;
    return MVO_OK;
}

int mvo_debug_get_homography_decomposition(mvo_ctx* ctx, double* Hn, double* w, int32_t* branch, double* Rs,
                                           double* ts, double* normals, int32_t* rejected) {
    if (!ctx || !ctx->track) return mvo_set_err(ctx, MVO_ERR_STATE, "no homography decomposition on this ctx yet", hipSuccess);
    const mvo_track_state* s = ctx->track;
    const int count = s->hd_cnt[5];
    if (Hn) std::memcpy(Hn, s->hd_out + kHdHn, 9 * sizeof(double));
    if (w) std::memcpy(w, s->hd_out + kHdW, 3 * sizeof(double));
    if (branch) {
        branch[0] = count == 1 ? 1 : 0;
        branch[1] = count == 4 ? s->hd_cnt[6] : -1;
    }
    if (Rs) std::memcpy(Rs, s->hd_out + kHdR, 36 * sizeof(double));
    if (ts) std::memcpy(ts, s->hd_out + kHdT, 12 * sizeof(double));
    if (normals) std::memcpy(normals, s->hd_out + kHdN, 12 * sizeof(double));
    if (rejected) std::memcpy(rejected, s->hd_cnt, 4 * sizeof(int32_t));
    return count;
}

// helperEstimatePossibleRelativePosesByEpipolarGeometry (motion_estimation.cpp:10-157), is_calc_homo = true.  The E
// and H branches run as the single calls do and leave their models and masks on the device; k_h_decompose and
// k_init_triangulate (every slot in one launch) follow in stream order, and one read-back brings the decomposition and
// the points.  The scores are mvo_check_init_scores on the two lists; the choice and invRt are host scalars.
int mvo_estimate_possible_relative_poses(mvo_ctx* ctx, const float* pts1, const float* pts2, int n, double fx,
                                         double fy, double cx, double cy, double prob, double threshold,
                                         double h_threshold, double h_confidence, double sigma,
                                         int motion_cam2_to_cam1, mvo_init_poses* out) {
    if (!ctx || !out || n < 0 || (n && (!pts1 || !pts2)) || out->cap_inliers < 0 || out->cap_pts < 0 ||
        (out->cap_inliers && (!out->inliers_e || !out->inliers_h)) || (out->cap_pts && !out->pts3d))
        return mvo_set_err(ctx, MVO_ERR_INVALID, "bad arguments", hipSuccess);
    if (out->cap_inliers < n)
        return mvo_set_err(ctx, MVO_ERR_CAPACITY, "mvo_estimate_possible_relative_poses: inlier buffers smaller than n", hipSuccess);
    for (int k = 0; k < 9; ++k) out->E[k] = out->H[k] = 0;
    out->found_e = out->found_h = out->n_inliers_e = out->n_inliers_h = 0;
    out->n_slots = 1;
    for (int j = 0; j < 5; ++j) {
        out->present[j] = 0;
        out->h_candidate[j] = -1;
        out->pts_offset[j] = out->pts_count[j] = 0;
        for (int k = 0; k < 9; ++k) out->R[j][k] = 0;
        for (int k = 0; k < 3; ++k) out->t[j][k] = out->normal[j][k] = 0;
    }
    out->score_e = out->score_h = out->ratio = 0;
    out->best = -1;
    mvo_track_state* s = state(ctx);
    reset_hd_record(s);
    // estiMotionByEssential, then estiMotionByHomography (the reference's order)
    double R_e[9], t_e[3], H_raw[9];
    int r = mvo_esti_motion_by_essential(ctx, pts1, pts2, n, fx, fy, cx, cy, prob, threshold, out->E, R_e, t_e,
                                         out->inliers_e, out->cap_inliers, &out->n_inliers_e, &out->found_e);
    if (r) return r;
    r = mvo_find_homography(ctx, pts1, pts2, n, h_threshold, h_confidence, H_raw, out->inliers_h, out->cap_inliers,
                            &out->n_inliers_h, &out->found_h);
    if (r) return r;
    if (n == 0) {  // no model, no slot: both scores 0, a NaN ratio, best = -1
        out->ratio = out->score_h / (out->score_e + out->score_h);
        return MVO_OK;
    }
    if ((r = ensure_tri(ctx, n)) || (r = ensure_hd(ctx))) return r;
    const size_t n_pts = (size_t)5 * n * 3;
    if ((r = s->d_ip_pts.ensure(ctx, n_pts, 1 << 16))) return r;
    const size_t o_out = ((size_t)n * 16 + 63) / 64 * 64, o_pts = o_out + 1024;  // out (744 B), cnt (48 B), points
    if ((r = mvo_ensure_pinned(ctx, o_pts + n_pts * sizeof(float)))) return r;
    MVO_HIP(hipStreamSynchronize(ctx->stream));
    std::memcpy(ctx->h_pin, pts1, (size_t)n * 8);
    std::memcpy(ctx->h_pin + (size_t)n * 8, pts2, (size_t)n * 8);
    MVO_HIP(hipMemcpyAsync(s->d_tri_in, ctx->h_pin, (size_t)n * 16, hipMemcpyHostToDevice, ctx->stream));
    const float* d_p1 = s->d_tri_in;
    const float* d_p2 = s->d_tri_in + 2 * (size_t)n;
    const TrackCamera cam{fx, fy, cx, cy};
    if (out->found_h &&
        (r = track_launch_h_decompose(ctx, d_p1, d_p2, device_h_mask(s, n), n, device_h(s, n), cam, s->d_hd_cnt, s->d_hd_out)))
        return r;
    if ((r = track_launch_init_triangulate(ctx, d_p1, d_p2, n, cam, out->found_e ? s->d_rp_out : nullptr,
                                           n == 5 ? nullptr : s->d_em_mask, out->found_h ? s->d_hd_out : nullptr,
                                           s->d_hd_cnt, device_h_mask(s, n), s->d_ip_pts)))
        return r;
    double* h_out = reinterpret_cast<double*>(ctx->h_pin + o_out);
    int32_t* h_cnt = reinterpret_cast<int32_t*>(ctx->h_pin + o_out + kHdOut * sizeof(double));
    float* h_pts = reinterpret_cast<float*>(ctx->h_pin + o_pts);
    if (out->found_h) {
        MVO_HIP(hipMemcpyAsync(h_out, s->d_hd_out, kHdOut * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        MVO_HIP(hipMemcpyAsync(h_cnt, s->d_hd_cnt, kHdCnt * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (out->found_e || out->found_h)
        MVO_HIP(hipMemcpyAsync(h_pts, s->d_ip_pts, n_pts * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    MVO_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->prof) mvo_prof_collect(ctx);
    if (out->found_h) {
        std::memcpy(s->hd_out, h_out, sizeof(s->hd_out));
        std::memcpy(s->hd_cnt, h_cnt, sizeof(s->hd_cnt));
        for (int k = 0; k < 9; ++k) out->H[k] = s->hd_out[kHdHs + k];
    }
    // the solution table: slot 0 = E (absent without a model), slots 1..k = the surviving H candidates
    const int k_surv = out->found_h ? s->hd_cnt[7] : 0;
    int need = out->found_e ? out->n_inliers_e : 0;
    need += k_surv * out->n_inliers_h;
    if (need > out->cap_pts)
        return mvo_set_err(ctx, MVO_ERR_CAPACITY, "mvo_estimate_possible_relative_poses: point buffer too small", hipSuccess);
    int off = 0;
    auto gather = [&](int slot, int src_slot, const int32_t* list, int m) {
        out->pts_offset[slot] = off;
        out->pts_count[slot] = m;
        for (int j = 0; j < m; ++j)
            std::memcpy(out->pts3d + 3 * (size_t)(off + j), h_pts + 3 * ((size_t)src_slot * n + list[j]), 12);
        off += m;
    };
    if (out->found_e) {
        out->present[0] = 1;
        std::memcpy(out->R[0], R_e, sizeof(R_e));
        std::memcpy(out->t[0], t_e, sizeof(t_e));
        gather(0, 0, out->inliers_e, out->n_inliers_e);
    }
    for (int j = 0; j < k_surv; ++j) {
        const int c = s->hd_cnt[8 + j], slot = 1 + j;
        out->present[slot] = 1;
        out->h_candidate[slot] = c;
        for (int k = 0; k < 9; ++k) out->R[slot][k] = s->hd_out[kHdR + 9 * c + k];
        for (int k = 0; k < 3; ++k) {
            out->t[slot][k] = s->hd_out[kHdTn + 3 * c + k];
            out->normal[slot][k] = s->hd_out[kHdN + 3 * c + k];
        }
        gather(slot, 1 + c, out->inliers_h, out->n_inliers_h);
    }
    out->n_slots = 1 + k_surv;
    // checkEssentialScore / checkHomographyScore; an absent model scores 0 (deviations 9 and 10)
    std::vector<int32_t> kept((size_t)out->n_inliers_e + out->n_inliers_h + 2);
    int n_kept_e = 0, n_kept_h = 0;
    if ((r = mvo_check_init_scores(ctx, pts1, pts2, n, fx, fy, cx, cy, out->found_e ? out->E : nullptr, out->inliers_e,
                                   out->n_inliers_e, out->found_h ? out->H : nullptr, out->inliers_h, out->n_inliers_h,
                                   sigma, &out->score_e, &out->score_h, kept.data(), &n_kept_e,
                                   kept.data() + out->n_inliers_e, &n_kept_h)))
        return r;
    out->ratio = out->score_h / (out->score_e + out->score_h);
    // the choice (motion_estimation.cpp:141-155); a slot that does not exist gives -1 (deviation 11)
    if (out->ratio > 0.5) {
        if (k_surv > 0) {
            int best = 1;
            double largest = std::fabs(out->normal[1][2]);
            for (int j = 2; j <= k_surv; ++j) {
                const double z = std::fabs(out->normal[j][2]);
                if (z > largest) {
                    largest = z;
                    best = j;
                }
            }
            out->best = best;
        }
    } else if (out->found_e) {
        out->best = 0;
    }
    if (!motion_cam2_to_cam1)
        for (int j = 0; j < 5; ++j)
            if (out->present[j]) inv_rt(out->R[j], out->t[j]);
    return MVO_OK;
}

int mvo_retain_good_triangulation(const float* pts3d_in_curr, int n, const double* T_w_c_curr, const double* T_w_c_ref,
                                  double min_triang_angle, double max_ratio_to_median, int32_t* keep, int* n_keep,
                                  double* angles) {
    if (n < 0 || !n_keep || !T_w_c_curr || !T_w_c_ref || (n && (!pts3d_in_curr || !keep))) return MVO_ERR_INVALID;
    *n_keep = 0;
    if (n == 0) return MVO_OK;  // vo.cpp:198-199
    std::vector<double> ang(n);
    for (int i = 0; i < n; ++i) {
        const float* pc = pts3d_in_curr + 3 * (size_t)i;
        double to_curr[3], to_ref[3];
        for (int r = 0; r < 3; ++r) {  // preTranslatePoint3f(p_in_curr, T_w_c) -> float, then the two rays
            const double* row = T_w_c_curr + 4 * r;
            double acc = 0;
            acc += row[0] * (double)pc[0];
            acc += row[1] * (double)pc[1];
            acc += row[2] * (double)pc[2];
            acc += row[3] * 1.0;
            const double pw = (double)(float)acc;
            to_curr[r] = T_w_c_curr[4 * r + 3] - pw;
            to_ref[r] = T_w_c_ref[4 * r + 3] - pw;
        }
        double dot = 0, n1 = 0, n2 = 0;
        for (int r = 0; r < 3; ++r) dot += to_curr[r] * to_ref[r];
        for (int r = 0; r < 3; ++r) n1 = n1 + to_curr[r] * to_curr[r];
        for (int r = 0; r < 3; ++r) n2 = n2 + to_ref[r] * to_ref[r];
        ang[i] = std::acos(dot / (std::sqrt(n1) * std::sqrt(n2))) / 3.1415926 * 180.0;  // vo.cpp:210
    }
    std::vector<double> sorted(ang);
    std::sort(sorted.begin(), sorted.end());
    const double median = sorted[n / 2];
    int cnt = 0;
    for (int i = 0; i < n; ++i) {
        if (angles) angles[i] = ang[i];
        if (ang[i] < min_triang_angle || ang[i] / median > max_ratio_to_median) continue;  // vo.cpp:233-235
        keep[cnt++] = i;
    }
    *n_keep = cnt;
    return MVO_OK;
}

int mvo_rodrigues(const double* rvec, double* R) {
    if (!rvec || !R) return MVO_ERR_INVALID;
    const double x = rvec[0], y = rvec[1], z = rvec[2];
    const double theta = std::sqrt(x * x + y * y + z * z);
    if (theta < DBL_EPSILON) {
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
        return MVO_OK;
    }
    const double c = std::cos(theta), s = std::sin(theta), c1 = 1. - c, it = 1. / theta;
    const double rx = x * it, ry = y * it, rz = z * it;
    const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
    const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
    for (int k = 0; k < 9; ++k) R[k] = c * ((k % 4 == 0) ? 1.0 : 0.0) + c1 * rrt[k] + s * r_x[k];
    return MVO_OK;
}

int mvo_invert_pose(const double* T, double* T_inv) {
    if (!T || !T_inv) return MVO_ERR_INVALID;
    double tmp[16];
    if (!invert_pose_lu(T, tmp, 4)) return MVO_ERR_INVALID;
    std::memcpy(T_inv, tmp, sizeof(tmp));
    return MVO_OK;
}

int mvo_debug_get_pnp(mvo_ctx* ctx, double* models, int32_t* counts, int cap, int32_t* info) {
    if (!ctx || !ctx->track) return mvo_set_err(ctx, MVO_ERR_STATE, "no PnP solve on this ctx yet", hipSuccess);
    const mvo_track_state* s = ctx->track;
    const int h = (int)s->counts.size();
    if (info) std::memcpy(info, s->info, sizeof(s->info));
    if (h > cap) return mvo_set_err(ctx, MVO_ERR_CAPACITY, "mvo_debug_get_pnp: buffers too small", hipSuccess);
    if (models && h) std::memcpy(models, s->models.data(), (size_t)h * 96);
    if (counts && h) std::memcpy(counts, s->counts.data(), (size_t)h * 4);
    return h;
}
}
