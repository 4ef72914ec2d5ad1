// csrc/track_kernels.hip -- tracking rows between the matcher and bundle adjustment:
//   k_map_in_view      VisualOdometry::getMappointsInCurrentView_ (src/vo/vo.cpp:16-49): project the resident map,
//                      keep what is in front of the camera and inside the image, gather the descriptors.
//   k_pnp_hypotheses   the RANSAC loop of cv::solvePnPRansac (vo.cpp:326-329): one workgroup of three waves per
//                      hypothesis runs the 5-point EPnP kernel (one wave per beta variant) and scores every pair.
//   k_pnp_refine       the final cv::solvePnP(SOLVEPNP_ITERATIVE) on the inliers: DLT start + Levenberg-Marquardt.
//   k_triangulate      geometry::helperTriangulatePoints (motion_estimation.cpp:214-247) on a keyframe's matches.
//   k_em_hypotheses    the RANSAC loop of cv::findEssentialMat (epipolar_geometry.cpp:36-39): one wave per five-point
//   k_em_mask          hypothesis; the inlier mask of the selected candidate.
//   k_h_hypotheses     the RANSAC loop of cv::findHomography (estiMotionByHomography, monocular initialisation): one
//   k_h_mask           wave per 4-point DLT hypothesis; the inlier mask of the selected one;
//   k_h_refine         the DLT on all inliers + LMSolver (10 iterations) that findHomography runs after RANSAC.
//   k_recover_pose     recoverPose after findEssentialMat (estiMotionByEssential): one lane per (match, combination).
//   k_init_scores      checkEssentialScore and checkHomographyScore (the E/H choice of the initialisation).
//   k_h_decompose      decomposeHomographyMat + filterHomographyDecompByVisibleRefpoints after findHomography
//                      (estiMotionByHomography, removeWrongRtOfHomography): one lane per match, the H inliers vote.
//   k_init_triangulate doTriangulation of every candidate solution of the initialisation in one launch.
//   k_init_finish      the chosen solution's points in the current camera, the cosine of every triangulation angle and
//                      the pixel distance of every match (estimateMotionAnd3DPoints_, isVoGoodToInit_; init_wave.h).
// The arithmetic lives in pnp_wave.h (wave-level SPMD code); this file binds it to threads and LDS.
#include "mvo_internal.h"

#include <algorithm>
#include <cstdlib>

#define PW_FN __device__ __forceinline__
#define PW_LANES(l, NL) for (int l = (int)threadIdx.x, pw_once_ = 1; pw_once_; pw_once_ = 0)
#define PW_WAVES(w, NW) for (int w = (int)(threadIdx.x >> 6), pw_once_ = 1; pw_once_; pw_once_ = 0)
#define PW_SYNC() __syncthreads()
#define PW_UNROLL _Pragma("unroll")
#include "em_wave.h"
#include "h_wave.h"
#include "hd_wave.h"
#include "init_wave.h"

// ------------------------------------------------------------------------------------------------ map in view
// One workgroup walks the map in chunks of 1024 points and appends the survivors in map order (the reference
// iterates Map::map_points_ and push_backs).  p_cam = (float)(T_c_w * p) accumulated in double like
// basics::preTranslatePoint3f (opencv_funcs.cpp:67-78); pixel = (float)(fx * x / z + cx) like geometry::cam2pixel
// (camera.cpp:23-28); the tests are `p_cam.z < 0` and the strict image bounds of vo.cpp:31-36.
__global__ __launch_bounds__(1024) void k_map_in_view(const float* __restrict__ pos, const uint4* __restrict__ desc,
                                                       int n, TrackViewArgs a, int32_t* __restrict__ idx,
                                                       float2* __restrict__ px, uint4* __restrict__ desc_out,
                                                       int32_t* __restrict__ n_out) {
    __shared__ int wave_cnt[16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int base = 0;
    for (int start = 0; start < n; start += 1024) {
        const int i = start + (int)threadIdx.x;
        bool in = false;
        float u = 0.f, v = 0.f;
        if (i < n) {
            const double p[4] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], 1.0};
            double res[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                double acc = 0.0;
#pragma unroll
                for (int j = 0; j < 4; ++j) acc += a.T[4 * r + j] * p[j];
                res[r] = acc;
            }
            const float pcx = (float)res[0], pcy = (float)res[1], pcz = (float)res[2];
            in = !(pcz < 0);
            u = (float)(a.fx * pcx / pcz + a.cx);
            v = (float)(a.fy * pcy / pcz + a.cy);
            in = in && (u > 0 && v > 0 && u < (float)a.cols && v < (float)a.rows);
        }
        const unsigned long long b = __ballot(in);
        if (lane == 0) wave_cnt[w] = __popcll(b);
        __syncthreads();
        int off = base, total = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int c = wave_cnt[q];
            off += q < w ? c : 0;
            total += c;
        }
        if (in) {
            const int o = off + __popcll(b & ((1ull << lane) - 1ull));
            idx[o] = i;
            px[o] = make_float2(u, v);
            desc_out[2 * o] = desc[2 * i];
            desc_out[2 * o + 1] = desc[2 * i + 1];
        }
        base += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *n_out = base;
}

int track_launch_map_in_view(mvo_ctx* ctx, const float* d_pos, const uint8_t* d_desc, int n, const TrackViewArgs& a,
                             int32_t* d_idx, float* d_px, uint8_t* d_desc_out, int32_t* d_n) {
    ProfScope ps(ctx, "k_map_in_view");
    hipLaunchKernelGGL(k_map_in_view, dim3(1), dim3(1024), 0, ctx->stream, d_pos, (const uint4*)d_desc, n, a, d_idx,
                       (float2*)d_px, (uint4*)d_desc_out, d_n);
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}

// ------------------------------------------------------------------------------------------------ PnP RANSAC
__device__ __forceinline__ void pnp_hypothesis_body(const float* __restrict__ p3, const float* __restrict__ p2, int n,
                                                        const int32_t* __restrict__ subsets, TrackCamera cam, float thr2,
                                                        double* __restrict__ models, int32_t* __restrict__ counts,
                                                        uint8_t* __restrict__ masks, double* __restrict__ h_models,
                                                        int32_t* __restrict__ h_counts, pw::HypLds& lds) {
    const int h = blockIdx.x;
    const pw::Camera c{cam.fx, cam.fy, cam.cx, cam.cy};
    double R[3][3], t[3];
    pw::epnp_hypothesis(lds, p3, p2, subsets + pw::kModelPoints * h, c, R, t);
    const int good = pw::score_model(lds, p3, p2, n, c, R, t, thr2, masks + (size_t)h * n);
    if (threadIdx.x == 0) {
        double* m = models + 12 * (size_t)h;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) m[3 * i + j] = R[i][j];
            m[9 + i] = t[i];
        }
        counts[h] = good;
        // the same record straight into the caller's pinned buffer (the refinement kernel reads the device copy: its replay of
        // the RANSAC bookkeeping is a chain of dependent loads)
        double* hm = h_models + 12 * (size_t)h;
#pragma unroll
        for (int i = 0; i < 12; ++i) hm[i] = m[i];
        h_counts[h] = good;
    }
}

// Two builds of the same body: the compiler's free choice (256 VGPR + 52 AGPR = ONE wave per SIMD: fastest for a lone frame on an
// empty chip, 200 us) and a build held to two waves per SIMD (40 registers spilled to scratch): next to the resident solver grid
// the 100 hypotheses of a frame share a few CUs, where a workgroup that holds a CU to itself is what limits the frame rate.
__global__ __launch_bounds__(pw::kHypLanes) void k_pnp_hypotheses(const float* __restrict__ p3, const float* __restrict__ p2, int n,
                                                        const int32_t* __restrict__ subsets, TrackCamera cam, float thr2,
                                                        double* __restrict__ models, int32_t* __restrict__ counts,
                                                        uint8_t* __restrict__ masks, double* __restrict__ h_models,
                                                        int32_t* __restrict__ h_counts) {
    __shared__ pw::HypLds lds;
    pnp_hypothesis_body(p3, p2, n, subsets, cam, thr2, models, counts, masks, h_models, h_counts, lds);
}
__global__ __launch_bounds__(pw::kHypLanes) MVO_WAVES_PER_EU(2, 2) void k_pnp_hypotheses_occ2(
    const float* __restrict__ p3, const float* __restrict__ p2, int n, const int32_t* __restrict__ subsets, TrackCamera cam, float thr2,
    double* __restrict__ models, int32_t* __restrict__ counts, uint8_t* __restrict__ masks, double* __restrict__ h_models,
    int32_t* __restrict__ h_counts) {
    __shared__ pw::HypLds lds;
    pnp_hypothesis_body(p3, p2, n, subsets, cam, thr2, models, counts, masks, h_models, h_counts, lds);
}

// Picks the best hypothesis (the RANSAC loop's bookkeeping replayed over the counts, or `forced_best` >= 0), keeps
// its mask in best_mask for the host and refines it.  out: param[6] = (rvec, tvec), n_inliers, dlt used, LM
// iterations, LM evaluations, best hypothesis (-1: none reached 5 inliers), iterations the sequential loop runs.
__global__ __launch_bounds__(pw::kRefLanes) void k_pnp_refine(const float* __restrict__ p3, const float* __restrict__ p2,
                                                              const uint8_t* __restrict__ masks, int n, TrackCamera cam,
                                                              const double* __restrict__ models,
                                                              const int32_t* __restrict__ counts, int n_hyp,
                                                              double confidence, int forced_best, int mode, double* Mg,
                                                              double* mg, uint8_t* __restrict__ best_mask,
                                                              double* __restrict__ out) {
    __shared__ pw::RefLds lds;
    const pw::Camera c{cam.fx, cam.fy, cam.cx, cam.cy};
    int best = forced_best, iters_run = mode == 1 ? 1 : 0;
    if (forced_best < 0) pw::ransac_replay(counts, n_hyp, n, confidence, &best, &iters_run);
    if (best < 0) {
        if (threadIdx.x == 0) {
            for (int k = 0; k < 10; ++k) out[k] = 0;
            out[10] = -1;
            out[11] = iters_run;
        }
        return;
    }
    const uint8_t* mask = masks + (size_t)best * n;
    const double* model = models + 12 * (size_t)best;
    for (int i = threadIdx.x; i < n; i += pw::kRefLanes) best_mask[i] = mask[i];
    double R0[3][3], t0[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) R0[i][j] = model[3 * i + j];
        t0[i] = model[9 + i];
    }
    pw::RefineResult res;
    pw::refine_pose(lds, p3, p2, mask, n, c, R0, t0, mode, Mg, mg, res);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) out[k] = res.param[k];
        out[6] = res.n_inliers;
        out[7] = res.used_dlt;
        out[8] = res.lm_iters;
        out[9] = res.lm_evals;
        out[10] = best;
        out[11] = iters_run;
    }
}

// ------------------------------------------------------------------------------------------------ triangulation
// geometry::helperTriangulatePoints (motion_estimation.cpp:214-247): one lane per match.
struct TrackPose {
    double R[9], t[3];
};
__global__ __launch_bounds__(256) void k_triangulate(const float2* __restrict__ kp1, const float2* __restrict__ kp2, int n,
                                                      TrackCamera cam, TrackPose pose, float* __restrict__ pts_prev,
                                                      float* __restrict__ pts_curr) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const pw::Camera c{cam.fx, cam.fy, cam.cx, cam.cy};
    const float a[2] = {kp1[i].x, kp1[i].y}, b[2] = {kp2[i].x, kp2[i].y};
    float pp[3], pc[3];
    pw::triangulate_match(a, b, c, pose.R, pose.t, pp, pc);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        pts_prev[3 * i + r] = pp[r];
        pts_curr[3 * i + r] = pc[r];
    }
}

int track_launch_triangulate(mvo_ctx* ctx, const float* d_kp1, const float* d_kp2, int n, const TrackCamera& cam,
                             const double* R, const double* t, float* d_prev, float* d_curr) {
    TrackPose pose;
    for (int k = 0; k < 9; ++k) pose.R[k] = R[k];
    for (int k = 0; k < 3; ++k) pose.t[k] = t[k];
    ProfScope ps(ctx, "k_triangulate");
    hipLaunchKernelGGL(k_triangulate, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, (const float2*)d_kp1,
                       (const float2*)d_kp2, n, cam, pose, d_prev, d_curr);
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}

// ------------------------------------------------------------------------------------------------ essential matrix
// cv::findEssentialMat's RANSAC loop (epipolar_geometry.cpp:36-39): one wave per hypothesis solves the five-point
// problem and counts the Sampson inliers of each of its (<= 10) candidates.
__global__ __launch_bounds__(pw::kEmLanes) void k_em_hypotheses(const double* __restrict__ q1, const double* __restrict__ q2,
                                                               int n, const int32_t* __restrict__ subsets, float thr2,
                                                               double* __restrict__ E, int32_t* __restrict__ n_models,
                                                               int32_t* __restrict__ counts) {
    __shared__ pw::EmLds lds;
    const size_t h = blockIdx.x;
    const int nm = pw::five_point_hypothesis(lds, q1, q2, subsets + 5 * h, E + 90 * h);
    __threadfence_block();
    __syncthreads();  // the candidates were written by lanes 0..8, every lane reads them for the scoring
    pw::score_essentials(lds, q1, q2, n, E + 90 * h, nm, thr2, counts + 10 * h);
    if (threadIdx.x == 0) n_models[h] = nm;
}

// inlier mask of the selected candidate (the bestMask of RANSACPointSetRegistrator::run)
__global__ __launch_bounds__(256) void k_em_mask(const double* __restrict__ q1, const double* __restrict__ q2, int n,
                                                 const double* __restrict__ E, float thr2, uint8_t* __restrict__ mask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double e[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] = E[k];
    mask[i] = pw::sampson_inlier(e, q1[2 * i], q1[2 * i + 1], q2[2 * i], q2[2 * i + 1], thr2) ? 1 : 0;
}

int track_launch_em_hypotheses(mvo_ctx* ctx, const double* d_q1, const double* d_q2, int n, const int32_t* d_subsets,
                               int n_hyp, float thr2, double* d_E, int32_t* d_nm, int32_t* d_counts) {
    ProfScope ps(ctx, "k_em_hypotheses");
    hipLaunchKernelGGL(k_em_hypotheses, dim3(n_hyp), dim3(pw::kEmLanes), 0, ctx->stream, d_q1, d_q2, n, d_subsets, thr2,
                       d_E, d_nm, d_counts);
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}

int track_launch_em_mask(mvo_ctx* ctx, const double* d_q1, const double* d_q2, int n, const double* d_E, float thr2,
                         uint8_t* d_mask) {
    ProfScope ps(ctx, "k_em_mask");
    hipLaunchKernelGGL(k_em_mask, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d_q1, d_q2, n, d_E, thr2, d_mask);
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}

int track_launch_pnp_hypotheses(mvo_ctx* ctx, const float* d_p3, const float* d_p2, int n, const int32_t* d_subsets,
                                int n_hyp, const TrackCamera& cam, float thr2, double* d_models, int32_t* d_counts,
                                uint8_t* d_masks, double* h_models, int32_t* h_counts) {
    ProfScope ps(ctx, "k_pnp_hypotheses");
    static const int env_occ = std::getenv("MVO_PNP_OCC") ? std::atoi(std::getenv("MVO_PNP_OCC")) : 0;  // 0: by mode, 1 / 2: forced
    const bool occ2 = env_occ ? env_occ == 2 : ctx->ba_throughput_mode != 0;
    hipLaunchKernelGGL(occ2 ? k_pnp_hypotheses_occ2 : k_pnp_hypotheses, dim3(n_hyp), dim3(pw::kHypLanes), 0, ctx->stream, d_p3, d_p2, n, d_subsets, cam, thr2,
                       d_models, d_counts, d_masks, h_models, h_counts);
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}

int track_launch_pnp_refine(mvo_ctx* ctx, const float* d_p3, const float* d_p2, const uint8_t* d_masks, int n,
                            const TrackCamera& cam, const double* d_models, const int32_t* d_counts, int n_hyp,
                            double confidence, int forced_best, int mode, double* d_Mg, double* d_mg,
                            uint8_t* d_best_mask, double* d_out) {
    ProfScope ps(ctx, "k_pnp_refine");
    hipLaunchKernelGGL(k_pnp_refine, dim3(1), dim3(pw::kRefLanes), 0, ctx->stream, d_p3, d_p2, d_masks, n, cam, d_models,
                       d_counts, n_hyp, confidence, forced_best, mode, d_Mg, d_mg, d_best_mask, d_out);
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}

// ------------------------------------------------------------------------------------------------ homography
// cv::findHomography's RANSAC loop: one wave per hypothesis runs HomographyEstimatorCallback::runKernel on its 4
// matches and counts the inliers over all n (-1: degenerate subset, runKernel returned no model).
__global__ __launch_bounds__(pw::kHLanes) void k_h_hypotheses(const float* __restrict__ src, const float* __restrict__ dst,
                                                             int n, const int32_t* __restrict__ subsets, float thr2,
                                                             double* __restrict__ H, int32_t* __restrict__ counts) {
    __shared__ pw::HDltLds lds;
    const size_t h = blockIdx.x;
    double Hh[9];
    const bool ok = pw::h_hypothesis(lds, src, dst, subsets + 4 * h, Hh);
    const int good = ok ? pw::h_count(lds, src, dst, n, Hh, thr2) : -1;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) H[9 * h + k] = ok ? Hh[k] : 0.0;
        counts[h] = good;
    }
}

// inlier mask of the selected hypothesis (the bestMask of RANSACPointSetRegistrator::run)
__global__ __launch_bounds__(256) void k_h_mask(const float* __restrict__ src, const float* __restrict__ dst, int n,
                                                const double* __restrict__ H, float thr2, uint8_t* __restrict__ mask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float Hf[9];
    for (int k = 0; k < 9; ++k) Hf[k] = (float)H[k];
    mask[i] = pw::h_error(Hf, src[2 * i], src[2 * i + 1], dst[2 * i], dst[2 * i + 1]) <= thr2 ? 1 : 0;
}

// findHomography after RANSAC (n > 4): runKernel on the inliers (kept when it yields a model), then the LM on the
// 8 free entries.  out: H[9], then (double) LM iterations, DLT re-fit used.
__global__ __launch_bounds__(pw::kHLanes) void k_h_refine(const float* __restrict__ src, const float* __restrict__ dst,
                                                         const uint8_t* __restrict__ mask, int n,
                                                         const double* __restrict__ H_ransac, double* __restrict__ out) {
    __shared__ pw::HRefLds lds;
    double H[9], Hn[9];
    for (int k = 0; k < 9; ++k) H[k] = H_ransac[k];
    const bool dlt = pw::h_dlt_inliers(lds, src, dst, mask, n, Hn);
    if (dlt)
        for (int k = 0; k < 9; ++k) H[k] = Hn[k];
    const int iters = pw::h_refine_lm(lds, src, dst, mask, n, H);
    if (threadIdx.x == 0) {
        for (int k = 0; k < 9; ++k) out[k] = H[k];
        out[9] = iters;
        out[10] = dlt ? 1 : 0;
    }
}

int track_launch_h_hypotheses(mvo_ctx* ctx, const float* d_src, const float* d_dst, int n, const int32_t* d_subsets,
                              int n_hyp, float thr2, double* d_H, int32_t* d_counts) {
    ProfScope ps(ctx, "k_h_hypotheses");
    hipLaunchKernelGGL(k_h_hypotheses, dim3(n_hyp), dim3(pw::kHLanes), 0, ctx->stream, d_src, d_dst, n, d_subsets, thr2,
                       d_H, d_counts);
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}

int track_launch_h_mask(mvo_ctx* ctx, const float* d_src, const float* d_dst, int n, const double* d_H, float thr2,
                        uint8_t* d_mask) {
    ProfScope ps(ctx, "k_h_mask");
    hipLaunchKernelGGL(k_h_mask, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d_src, d_dst, n, d_H, thr2, d_mask);
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}

int track_launch_h_refine(mvo_ctx* ctx, const float* d_src, const float* d_dst, const uint8_t* d_mask, int n,
                          const double* d_H, double* d_out) {
    ProfScope ps(ctx, "k_h_refine");
    hipLaunchKernelGGL(k_h_refine, dim3(1), dim3(pw::kHLanes), 0, ctx->stream, d_src, d_dst, d_mask, n, d_H, d_out);
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}

// ------------------------------------------------------------------------------------------------ recoverPose
// One lane per (match i, combination c): lane g of the grid takes i = g / 4, c = g % 4.  Every lane scales E and
// decomposes it itself (uniform, a few hundred flops).  mask[i] gets bit c when the match passes combination c and
// the RANSAC mask (NULL: every match is a RANSAC inlier).  The four counts are integer sums (exact in any order): per
// wave a ballot, per workgroup an add, across workgroups an atomic add; the last workgroup to arrive makes the choice.
// cnt: [0..3] counts, [4] arrivals (both zero on entry), [5] chosen combination.  out: E (scaled, 9), R (9), t (3),
// R1 R2 t of the decomposition (21).
__global__ __launch_bounds__(256) void k_recover_pose(const double* __restrict__ q1, const double* __restrict__ q2, int n,
                                                      const double* __restrict__ E_raw,
                                                      const uint8_t* __restrict__ ransac_mask, uint8_t* __restrict__ masks,
                                                      int32_t* cnt, double* __restrict__ out) {
    __shared__ uint8_t bits[256];
    __shared__ int wave_cnt[4][4];
    __shared__ int last;
    const int t = threadIdx.x;
    double e_raw[9], E[9], D[21];
#pragma unroll
    for (int k = 0; k < 9; ++k) e_raw[k] = E_raw[k];
    pw::rp_scale9(e_raw, e_raw[8], E);
    pw::decompose_essential(E, D);
    const int g = blockIdx.x * 256 + t, i = g >> 2, c = g & 3;
    bool pass = false;
    if (i < n) {
        double P[12];
        pw::rp_combination(D, c, P);
        pass = pw::rp_cheirality(q1[2 * i], q1[2 * i + 1], q2[2 * i], q2[2 * i + 1], P, pw::kRpDistanceThresh) &&
               (!ransac_mask || ransac_mask[i]);
    }
    bits[t] = pass ? (uint8_t)(1u << c) : (uint8_t)0;
    const unsigned long long b = __ballot(pass);
    if ((t & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) wave_cnt[t >> 6][k] = __popcll(b & (0x1111111111111111ull << k));
    }
    __syncthreads();
    if (t < 64) {
        const int m = blockIdx.x * 64 + t;
        if (m < n) masks[m] = bits[4 * t] | bits[4 * t + 1] | bits[4 * t + 2] | bits[4 * t + 3];
    }
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            __hip_atomic_fetch_add(cnt + k, wave_cnt[0][k] + wave_cnt[1][k] + wave_cnt[2][k] + wave_cnt[3][k],
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        last = __hip_atomic_fetch_add(cnt + 4, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (!last || t != 0) return;
    __threadfence();
    int32_t good[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) good[k] = __hip_atomic_load(cnt + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int chosen = pw::rp_choose(good);
    double R[9], tn[3];
    pw::rp_finish(D, chosen, R, tn);
    for (int k = 0; k < 9; ++k) out[k] = E[k];
    for (int k = 0; k < 9; ++k) out[9 + k] = R[k];
    for (int k = 0; k < 3; ++k) out[18 + k] = tn[k];
    for (int k = 0; k < 21; ++k) out[21 + k] = D[k];
    cnt[5] = chosen;
}

int track_launch_recover_pose(mvo_ctx* ctx, const double* d_q1, const double* d_q2, int n, const double* d_E,
                              const uint8_t* d_ransac_mask, uint8_t* d_masks, int32_t* d_cnt, double* d_out) {
    MVO_HIP(hipMemsetAsync(d_cnt, 0, 6 * sizeof(int32_t), ctx->stream));
    ProfScope ps(ctx, "k_recover_pose");
    hipLaunchKernelGGL(k_recover_pose, dim3((n + 63) / 64), dim3(256), 0, ctx->stream, d_q1, d_q2, n, d_E, d_ransac_mask,
                       d_masks, d_cnt, d_out);
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}

// ------------------------------------------------------------------------------------------------ E / H scores
// Workgroup 0 scores the E list, workgroup 1 the H list, one wave each.  Lane l takes the list positions
// l, l + 64, ... (one lane per listed match) and accumulates its terms from 0.0, term 1 before term 2; the 64
// partials are then added in lane order.  The kept entries are appended in list order (ballot prefix per round).
__global__ __launch_bounds__(64) void k_init_scores(const float2* __restrict__ kp1, const float2* __restrict__ kp2,
                                                    const int32_t* __restrict__ lists, int n_e, int n_h, InitScoreArgs a,
                                                    double* __restrict__ scores, int32_t* __restrict__ kept,
                                                    int32_t* __restrict__ n_kept) {
    __shared__ double part[64];
    const int which = blockIdx.x, l = threadIdx.x;
    const int32_t* list = lists + (which ? n_e : 0);
    int32_t* out = kept + (which ? n_e : 0);
    const int m = which ? (a.has_h ? n_h : 0) : (a.has_e ? n_e : 0);
    double acc = 0.0;
    int base = 0;
    for (int start = 0; start < m; start += 64) {
        const int i = start + l;
        bool good = false;
        if (i < m) {
            const int j = list[i];
            const double u1 = kp1[j].x, v1 = kp1[j].y, u2 = kp2[j].x, v2 = kp2[j].y;
            double t1, t2;
            if (which == 0) {
                pw::score_e_terms(a.f, u1, v1, u2, v2, a.inv_s2, &t1, &t2, &good);
                acc = acc + t1;
                acc = acc + t2;
            } else {
                bool add1, add2;
                pw::score_h_terms(a.h, a.hi, u1, v1, u2, v2, a.inv_s2, &t1, &add1, &t2, &add2, &good);
                if (add1) acc = acc + t1;
                if (add2) acc = acc + t2;
            }
        }
        const unsigned long long b = __ballot(good);
        if (good) out[base + __popcll(b & ((1ull << l) - 1ull))] = list[i];
        base += __popcll(b);
    }
    part[l] = acc;
    __syncthreads();
    if (l == 0) {
        double s = 0.0;
        for (int q = 0; q < 64; ++q) s = s + part[q];
        scores[which] = s;
        n_kept[which] = base;
    }
}

int track_launch_init_scores(mvo_ctx* ctx, const float* d_kp1, const float* d_kp2, const int32_t* d_lists, int n_e,
                             int n_h, const InitScoreArgs& a, double* d_scores, int32_t* d_kept, int32_t* d_n_kept) {
    ProfScope ps(ctx, "k_init_scores");
    hipLaunchKernelGGL(k_init_scores, dim3(2), dim3(64), 0, ctx->stream, (const float2*)d_kp1, (const float2*)d_kp2,
                       d_lists, n_e, n_h, a, d_scores, d_kept, d_n_kept);
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}

// ------------------------------------------------------------------------------------------------ H decomposition
// One lane per match i; the lanes of H inliers (mask[i], NULL: every match) test their match against every candidate
// (filterHomographyDecompByVisibleRefpoints).  Every lane scales H and decomposes it itself (uniform, a few hundred
// flops and one 3 x 3 Jacobi SVD).  The rejection counts are integer sums (exact in any order): per wave a ballot, per
// workgroup an add, across workgroups an atomic add; the last workgroup to arrive writes the decomposition, the
// normalised t and the survivors (count 0, in candidate order).  cnt: kHdCnt ints, out: kHdOut doubles (layouts in
// mvo_internal.h).
__global__ __launch_bounds__(256) void k_h_decompose(const float2* __restrict__ kp1, const float2* __restrict__ kp2,
                                                     const uint8_t* __restrict__ mask, int n,
                                                     const double* __restrict__ H_raw, TrackCamera cam, int32_t* cnt,
                                                     double* __restrict__ out) {
    __shared__ int wave_cnt[4][4];
    __shared__ int last;
    const int t = threadIdx.x;
    double h[9], Hs[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = H_raw[k];
    pw::rp_scale9(h, h[8], Hs);
    pw::HDecomp d;
    pw::hd_decompose(Hs, cam.fx, cam.fy, cam.cx, cam.cy, d);
    const int i = blockIdx.x * 256 + t;
    bool rej[4] = {false, false, false, false};
    if (i < n && (!mask || mask[i])) {
        // pixel2CamNormPlane, a cv::Point2f, then the CV_64FC2 copy the filter works on
        const double x1 = (float)((kp1[i].x - cam.cx) / cam.fx), y1 = (float)((kp1[i].y - cam.cy) / cam.fy);
        const double x2 = (float)((kp2[i].x - cam.cx) / cam.fx), y2 = (float)((kp2[i].y - cam.cy) / cam.fy);
#pragma unroll
        for (int c = 0; c < 4; ++c) rej[c] = c < d.count && pw::hd_rejects(x1, y1, x2, y2, d.R[c], d.n[c]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const unsigned long long b = __ballot(rej[c]);
        if ((t & 63) == 0) wave_cnt[t >> 6][c] = __popcll(b);
    }
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            __hip_atomic_fetch_add(cnt + c, wave_cnt[0][c] + wave_cnt[1][c] + wave_cnt[2][c] + wave_cnt[3][c],
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        last = __hip_atomic_fetch_add(cnt + 4, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (!last || t != 0) return;
    __threadfence();
    int k_surv = 0;
    for (int c = 0; c < d.count; ++c)
        if (__hip_atomic_load(cnt + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) cnt[8 + k_surv++] = c;
    for (int k = 0; k < 9; ++k) {
        out[kHdHs + k] = Hs[k];
        out[kHdHn + k] = d.Hn[k];
    }
    for (int k = 0; k < 3; ++k) out[kHdW + k] = d.w[k];
    for (int c = 0; c < 4; ++c) {
        double tn[3] = {0, 0, 0};
        if (c < d.count) pw::hd_normalise_t(d.t[c], tn);
        for (int k = 0; k < 9; ++k) out[kHdR + 9 * c + k] = d.R[c][k];
        for (int k = 0; k < 3; ++k) {
            out[kHdT + 3 * c + k] = d.t[c][k];
            out[kHdN + 3 * c + k] = d.n[c][k];
            out[kHdTn + 3 * c + k] = tn[k];
        }
    }
    cnt[5] = d.count;
    cnt[6] = d.branch;
    cnt[7] = k_surv;
}

int track_launch_h_decompose(mvo_ctx* ctx, const float* d_kp1, const float* d_kp2, const uint8_t* d_mask, int n,
                             const double* d_H, const TrackCamera& cam, int32_t* d_cnt, double* d_out) {
    MVO_HIP(hipMemsetAsync(d_cnt, 0, 5 * sizeof(int32_t), ctx->stream));
    ProfScope ps(ctx, "k_h_decompose");
    hipLaunchKernelGGL(k_h_decompose, dim3((std::max(n, 1) + 255) / 256), dim3(256), 0, ctx->stream,
                       (const float2*)d_kp1, (const float2*)d_kp2, d_mask, n, d_H, cam, d_cnt, d_out);
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}

// ------------------------------------------------------------------------------------------------ init triangulation
// doTriangulation of every solution of helperEstimatePossibleRelativePosesByEpipolarGeometry: blockIdx.y = slot (0: the
// E motion R, t of k_recover_pose's out; 1..4: the H candidates of k_h_decompose, R and the normalised t), one lane per
// match; the lanes of the slot's inliers (mask, NULL: every match) write pts[slot][i] (the point in camera 1, as
// pw::triangulate_match gives it).  e_out == NULL: no E slot; h_out == NULL: no H slots; H slots past the candidate
// count are skipped.
__global__ __launch_bounds__(256) void k_init_triangulate(const float2* __restrict__ kp1, const float2* __restrict__ kp2,
                                                          int n, TrackCamera cam, const double* __restrict__ e_out,
                                                          const uint8_t* __restrict__ e_mask,
                                                          const double* __restrict__ h_out,
                                                          const int32_t* __restrict__ h_cnt,
                                                          const uint8_t* __restrict__ h_mask, float* __restrict__ pts) {
    const int slot = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double R[9], tv[3];
    if (slot == 0) {
        if (!e_out || (e_mask && !e_mask[i])) return;
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = e_out[9 + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) tv[k] = e_out[18 + k];
    } else {
        const int c = slot - 1;
        if (!h_out || c >= h_cnt[5] || (h_mask && !h_mask[i])) return;
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = h_out[kHdR + 9 * c + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) tv[k] = h_out[kHdTn + 3 * c + k];
    }
    const pw::Camera c{cam.fx, cam.fy, cam.cx, cam.cy};
    const float a[2] = {kp1[i].x, kp1[i].y}, b[2] = {kp2[i].x, kp2[i].y};
    float pp[3], pc[3];
    pw::triangulate_match(a, b, c, R, tv, pp, pc);
    float* o = pts + 3 * ((size_t)slot * n + i);
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = pp[r];
}

int track_launch_init_triangulate(mvo_ctx* ctx, const float* d_kp1, const float* d_kp2, int n, const TrackCamera& cam,
                                  const double* d_e_out, const uint8_t* d_e_mask, const double* d_h_out,
                                  const int32_t* d_h_cnt, const uint8_t* d_h_mask, float* d_pts) {
    if (n == 0) return MVO_OK;
    ProfScope ps(ctx, "k_init_triangulate");
    hipLaunchKernelGGL(k_init_triangulate, dim3((n + 255) / 256, 5), dim3(256), 0, ctx->stream, (const float2*)d_kp1,
                       (const float2*)d_kp2, n, cam, d_e_out, d_e_mask, d_h_out, d_h_cnt, d_h_mask, d_pts);
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}

// ------------------------------------------------------------------------------------------------ init finish
// The chosen solution of the initialisation, one lane per entry of its inlier list (list[j] = index of the match):
// pts = that solution's row of k_init_triangulate's output (indexed by match), R / t = where k_recover_pose or
// k_h_decompose left the solution's motion.  p_curr: m x 3 float, cosang and pixdist: m doubles (pw::init_finish_point).
__global__ __launch_bounds__(256) void k_init_finish(const float* __restrict__ pts, const int32_t* __restrict__ list, int m,
                                                      const double* __restrict__ R_dev, const double* __restrict__ t_dev,
                                                      const float2* __restrict__ kp1, const float2* __restrict__ kp2,
                                                      pw::InitFinishPoses T, float* __restrict__ p_curr,
                                                      double* __restrict__ cosang, double* __restrict__ pixdist) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    double R[9], tv[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = R_dev[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) tv[k] = t_dev[k];
    const int i = list[j];
    const float p1[3] = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
    const float a[2] = {kp1[i].x, kp1[i].y}, b[2] = {kp2[i].x, kp2[i].y};
    float pc[3];
    double c, d;
    pw::init_finish_point(p1, R, tv, T, a, b, pc, &c, &d);
#pragma unroll
    for (int r = 0; r < 3; ++r) p_curr[3 * (size_t)j + r] = pc[r];
    cosang[j] = c;
    pixdist[j] = d;
}

int track_launch_init_finish(mvo_ctx* ctx, const float* d_pts, const int32_t* d_list, int m, const double* d_R,
                             const double* d_t, const float* d_kp1, const float* d_kp2, const double* T_w_c_curr,
                             const double* T_w_c_ref, float* d_p_curr, double* d_cosang, double* d_pixdist) {
    if (m == 0) return MVO_OK;
    pw::InitFinishPoses T;
    for (int k = 0; k < 16; ++k) {
        T.curr[k] = T_w_c_curr[k];
        T.ref[k] = T_w_c_ref[k];
    }
    ProfScope ps(ctx, "k_init_finish");
    hipLaunchKernelGGL(k_init_finish, dim3((m + 255) / 256), dim3(256), 0, ctx->stream, d_pts, d_list, m, d_R, d_t,
                       (const float2*)d_kp1, (const float2*)d_kp2, T, d_p_curr, d_cosang, d_pixdist);
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}
