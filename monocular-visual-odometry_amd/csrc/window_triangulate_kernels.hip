// csrc/window_triangulate_kernels.hip -- new map points for the keypoints of a keyframe that have none, from every buffered frame
// at once (include/mvo_hip.h: mvo_window_triangulate_search, mvo_window_triangulate).  ORB-SLAM's LocalMapping::
// CreateNewMapPoints searches every neighbouring keyframe along epipolar lines, triangulates and verifies; the reference
// triangulates against the reference keyframe only (triangulateWithReferenceKeyframe, vo_addFrame.cpp:104-116).  The arithmetic
// is declared in DESIGN.md section 20; tests/window_triangulate_numpy.py restates it.
//   k_window_epipolar_search  grid = (groups of 64 keypoints of curr) x (train groups) x (frames); blockIdx.z is the frame.  A
//                    workgroup reads its frame's row of the table (F, the active flag, the descriptors, the parked keypoints, nt,
//                    the slice) with wave-uniform loads, and is from there on k_knn2_epipolar (epipolar_kernels.hip) on that
//                    frame: the line of section 14, its gate, guided_knn2() (guided_knn2.h) with its partials, arrival counters
//                    and outputs offset by the frame.  A keypoint that is not free, a frame that failed the baseline test and a
//                    line with a^2 + b^2 = 0 are not active; a wave none of whose lanes is active skips its slice.
//   k_window_verify  one lane per surviving pair: pw::triangulate_match (pnp_wave.h; the arithmetic of k_triangulate) with the
//                    pair's frame row (R, t), then the six tests, every one evaluated, status = the OR of the failed bits.
// Every f64 operation below is one IEEE operation in the written order (the build has -ffp-contract=off).
#include "guided_knn2.h"

#include <cfloat>
#include <cmath>

#define PW_FN __device__ __forceinline__
#define PW_LANES(l, NL) for (int l = (int)threadIdx.x, pw_once_ = 1; pw_once_; pw_once_ = 0)
#define PW_WAVES(w, NW) for (int w = (int)(threadIdx.x >> 6), pw_once_ = 1; pw_once_; pw_once_ = 0)
#define PW_SYNC() __syncthreads()
#define PW_UNROLL _Pragma("unroll")
#include "pnp_wave.h"

struct WindowGate {  // the gate of section 14 (EpipolarGate, epipolar_kernels.hip) on trains parked as three doubles
    static constexpr bool kSkipIdleWave = true;
    const double* __restrict__ tg;
    double a, b, c, nrm;
    bool active;  // free, the frame active, nrm > 0
    __device__ __forceinline__ GuidedTrain load(int j) const { return {tg[3 * (size_t)j], tg[3 * (size_t)j + 1], tg[3 * (size_t)j + 2]}; }
    __device__ __forceinline__ bool pass(double u, double v, double tol) const {
        const double num = (a * u + b * v) + c;
        return (num * num <= tol * nrm) && active;
    }
};

// out_*: n_frames blocks of one row per keypoint of curr.  part / part_cnt: n_frames x gridDim.y x nq; arrive: n_frames x gridDim.x
__global__ __launch_bounds__(256) void k_window_epipolar_search(const uint4* __restrict__ q, const float2* __restrict__ qxy,
                                                                const uint8_t* __restrict__ qfree, int nq,
                                                                const WindowFrame* __restrict__ frames,
                                                                unsigned long long* __restrict__ part, int32_t* __restrict__ part_cnt,
                                                                int32_t* __restrict__ arrive, int32_t* __restrict__ out_idx,
                                                                int32_t* __restrict__ out_dist, int32_t* __restrict__ out_cnt) {
    const int f = blockIdx.z;  // workgroup-uniform: everything read through fr is a scalar load
    const WindowFrame& fr = frames[f];
    const int qi = blockIdx.x * 64 + (threadIdx.x & 63);
    const int qc = min(qi, nq - 1);
    const float2 p = qxy[qc];
    const double x = (double)p.x, y = (double)p.y;
    const double a = (fr.F[0] * x + fr.F[1] * y) + fr.F[2];
    const double b = (fr.F[3] * x + fr.F[4] * y) + fr.F[5];
    const double c = (fr.F[6] * x + fr.F[7] * y) + fr.F[8];
    const double nrm = a * a + b * b;
    const bool active = qfree[qc] != 0 && fr.active != 0 && nrm > 0;  // (false for NaN as well)
    const WindowGate gate = {fr.tg, a, b, c, nrm, active};
    const size_t rows = (size_t)f * nq;  // this frame's block of rows
    const GuidedPartials pf = {part + rows * gridDim.y, part_cnt + rows * gridDim.y, arrive + (size_t)f * gridDim.x};
    const GuidedResult r = guided_knn2(gate, q, nq, fr.d, fr.nt, fr.slice, pf, out_idx + 2 * rows, out_dist + 2 * rows);
    if (!r.deliver) return;
    out_cnt[rows + qi] = active ? r.cnt : -1;
}

__device__ __forceinline__ double window_dot3(double ax, double ay, double az, double bx, double by, double bz) {
    return (ax * bx + ay * by) + az * bz;
}
// squared reprojection error of the f32 point (x, y, z) against the pixel (u, v)
__device__ __forceinline__ double window_reproj2(const WindowVerifyArgs& a, const float (&p)[3], float u, float v) {
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    const double eu = ((a.fx * x) / z + a.cx) - (double)u;
    const double ev = ((a.fy * y) / z + a.cy) - (double)v;
    return eu * eu + ev * ev;
}

__global__ __launch_bounds__(64) void k_window_verify(const WindowPairIn* __restrict__ pairs, int n, const WindowFrame* __restrict__ frames,
                                                       WindowVerifyArgs a, WindowPairOut* __restrict__ out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const WindowPairIn pr = pairs[i];
    const WindowFrame& fr = frames[pr.frame];
    const double R[9] = {fr.R[0], fr.R[1], fr.R[2], fr.R[3], fr.R[4], fr.R[5], fr.R[6], fr.R[7], fr.R[8]};
    const double t[3] = {fr.tr[0], fr.tr[1], fr.tr[2]};
    const pw::Camera cam{a.fx, a.fy, a.cx, a.cy};
    const float kf[2] = {pr.uf, pr.vf}, kc[2] = {pr.uc, pr.vc};
    float pf[3], pc[3];
    pw::triangulate_match(kf, kc, cam, R, t, pf, pc);
    int status = 0;
    const bool finite = isfinite(pf[0]) && isfinite(pf[1]) && isfinite(pf[2]) && isfinite(pc[0]) && isfinite(pc[1]) && isfinite(pc[2]);
    status |= finite ? 0 : 1;
    status |= (pf[2] > 0 && pc[2] > 0) ? 0 : 2;
    const double v1x = (double)pc[0], v1y = (double)pc[1], v1z = (double)pc[2];
    const double v2x = v1x - t[0], v2y = v1y - t[1], v2z = v1z - t[2];
    const double dot = window_dot3(v1x, v1y, v1z, v2x, v2y, v2z);
    const double n1 = window_dot3(v1x, v1y, v1z, v1x, v1y, v1z);
    const double n2 = window_dot3(v2x, v2y, v2z, v2x, v2y, v2z);
    const double cos2 = (dot * dot) / (n1 * n2);
    status |= (dot > 0 && cos2 < a.c2max) ? 0 : 4;
    const double sf = (double)pr.sf, sc = (double)pr.sc;
    const double sf2 = sf * sf, sc2 = sc * sc;
    status |= (window_reproj2(a, pf, pr.uf, pr.vf) <= a.chi2 * sf2) ? 0 : 8;
    status |= (window_reproj2(a, pc, pr.uc, pr.vc) <= a.chi2 * sc2) ? 0 : 16;
    const double df2 = window_dot3((double)pf[0], (double)pf[1], (double)pf[2], (double)pf[0], (double)pf[1], (double)pf[2]);
    const double sa = df2 * sf2, sb = n1 * sc2;
    status |= (sa * a.rf2 >= sb && sa <= sb * a.rf2) ? 0 : 32;
    WindowPairOut o;
#pragma unroll
    for (int k = 0; k < 3; ++k) o.p_curr[k] = pc[k], o.p_frame[k] = pf[k];
    o.cos2 = cos2;
    o.status = status, o.pad = 0;
    out[i] = o;
}

// nq >= 1, 1 <= n_frames <= 64, every nt <= 65535, 1 <= ngroups <= GK_MAX_GROUPS (the caller's checks); out: n_frames x nq x idx[2],
// then as many dist[2], then n_frames x nq counts
int window_launch_search(mvo_ctx* ctx, const uint8_t* d_desc, const float* d_xy, const uint8_t* d_free, int nq, const WindowFrame* d_frames,
                         int n_frames, int ngroups, GuidedPartials part, int32_t* out) {
    const size_t rows = (size_t)n_frames * nq;
    ProfScope ps(ctx, "k_window_epipolar_search");
    hipLaunchKernelGGL(k_window_epipolar_search, dim3((nq + 63) / 64, ngroups, n_frames), dim3(256), 0, ctx->stream, (const uint4*)d_desc,
                       (const float2*)d_xy, d_free, nq, d_frames, part.key, part.cnt, part.arrive, out, out + 2 * rows, out + 4 * rows);
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}

// n >= 1; out: n records
int window_launch_verify(mvo_ctx* ctx, const WindowPairIn* d_pairs, int n, const WindowFrame* d_frames, const WindowVerifyArgs& a,
                         WindowPairOut* out) {
    ProfScope ps(ctx, "k_window_verify");
    hipLaunchKernelGGL(k_window_verify, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, d_pairs, n, d_frames, a, out);
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}
