// csrc/epipolar_kernels.hip -- pose-guided matching (include/mvo_hip.h: mvo_match_knn2_epipolar*): the 2-NN of k_knn2
// (match_kernels.hip) in which a (query, train) pair competes only if the train keypoint lies within a tolerance of the
// query's epipolar line.  What the reference asks for and does not have (README.md:212 "doing guided matching based on
// the estimated camera motion", README.md:272 "Utilize epipolar constraint to do feature matching").  The arithmetic is
// declared in DESIGN.md section 14; tests/epipolar_numpy.py restates it.
//   k_knn2_epipolar  one launch per call: guided_knn2() (guided_knn2.h) behind this prologue and gate.
//                    prologue: the query's line (a, b, c) from F and a^2 + b^2; a line with a^2 + b^2 = 0 or NaN has no
//                    candidates.  A train is parked as (double)u, (double)v, tol2.  gate: 7 f64 operations.
//                    outputs: idx, dist (the body) and the candidate count.
// Every f64 operation below is one IEEE operation in the written order (the build has -ffp-contract=off).
#include "guided_knn2.h"

struct EpipolarGate {
    static constexpr bool kSkipIdleWave = false;
    const float2* __restrict__ txy;
    const double* __restrict__ tol2;
    double a, b, c, nrm;
    bool active;  // nrm > 0
    __device__ __forceinline__ GuidedTrain load(int j) const {
        const float2 tp = txy[j];
        return {(double)tp.x, (double)tp.y, tol2[j]};
    }
    __device__ __forceinline__ bool pass(double u, double v, double tol) const {
        const double num = (a * u + b * v) + c;
        return (num * num <= tol * nrm) && active;  // (active first puts an exec mask around the f64 operations of every train)
    }
};

__global__ __launch_bounds__(256) void k_knn2_epipolar(const uint4* __restrict__ q, const float2* __restrict__ qxy, int nq,
                                                       const uint4* __restrict__ t, const float2* __restrict__ txy,
                                                       const double* __restrict__ tol2, int nt, EpipolarArgs A, int slice,
                                                       unsigned long long* __restrict__ part, int32_t* __restrict__ part_cnt,
                                                       int32_t* __restrict__ arrive, int32_t* __restrict__ out_idx,
                                                       int32_t* __restrict__ out_dist, int32_t* __restrict__ out_cnt) {
    const int qi = blockIdx.x * 64 + (threadIdx.x & 63);
    const float2 p = qxy[min(qi, nq - 1)];
    const double x = (double)p.x, y = (double)p.y;
    const double a = (A.f[0] * x + A.f[1] * y) + A.f[2];
    const double b = (A.f[3] * x + A.f[4] * y) + A.f[5];
    const double c = (A.f[6] * x + A.f[7] * y) + A.f[8];
    const double nrm = a * a + b * b;
    const EpipolarGate gate = {txy, tol2, a, b, c, nrm, nrm > 0};  // (false for NaN as well)
    const GuidedResult r = guided_knn2(gate, q, nq, t, nt, slice, {part, part_cnt, arrive}, out_idx, out_dist);
    if (r.deliver) out_cnt[qi] = r.cnt;
}

// nt >= 1, nt <= 65535 (the caller's check); out: nq x (idx[2], dist[2]) then nq counts
int epipolar_launch_knn2(mvo_ctx* ctx, const uint8_t* d_q, const float* d_qxy, int nq, const uint8_t* d_t, const float* d_txy,
                         const double* d_tol2, int nt, const EpipolarArgs& a, GuidedPartials part, int32_t* out) {
    if (nq <= 0) return MVO_OK;
    const int ngroups = guided_groups(nt);
    ProfScope ps(ctx, "k_knn2_epipolar");
    hipLaunchKernelGGL(k_knn2_epipolar, dim3((nq + 63) / 64, ngroups), dim3(256), 0, ctx->stream, (const uint4*)d_q,
                       (const float2*)d_qxy, nq, (const uint4*)d_t, (const float2*)d_txy, d_tol2, nt, a, guided_slice(nt, ngroups),
                       part.key, part.cnt, part.arrive, out, out + 2 * (size_t)nq, out + 4 * (size_t)nq);
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}
