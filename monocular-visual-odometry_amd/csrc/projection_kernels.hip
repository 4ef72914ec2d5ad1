// csrc/projection_kernels.hip -- tracking by projection (include/mvo_hip.h: mvo_map_match_knn2_projection*): the resident map
// is projected with a predicted pose and every map point in view takes its two nearest frame keypoints, in 256-bit Hamming
// space, among those within a radius of its projection.  The guided matching the reference asks for (README.md:212 "doing
// guided matching based on the estimated camera motion") on the step that runs on every frame (vo.cpp:267-289).  The
// arithmetic is declared in DESIGN.md section 15; tests/projection_numpy.py restates it.
//   k_map_match_projection  one launch per call; it stands for k_map_in_view, the compaction, the descriptor gather and the
//                    matcher launch: guided_knn2() (guided_knn2.h), one lane per map point, behind this prologue and gate.
//                    prologue: the projection of k_map_in_view (track_kernels.hip), operation for operation; a point not in
//                    view has no candidates, and a wave none of whose points is in view skips its slice.  A frame keypoint
//                    is parked as (double)x, (double)y, r2.  gate: 5 f64 operations (a disc of a few px holds one or two
//                    keypoints in two thousand).  outputs: idx, dist (the body), the candidate count or -1, the pixel.
// Every f64 operation below is one IEEE operation in the written order (the build has -ffp-contract=off).
#include "guided_knn2.h"

struct ProjectionGate {
    static constexpr bool kSkipIdleWave = true;
    const double* __restrict__ tg;
    double ud, vd;
    bool active;  // in view
    __device__ __forceinline__ GuidedTrain load(int j) const { return {tg[3 * (size_t)j], tg[3 * (size_t)j + 1], tg[3 * (size_t)j + 2]}; }
    __device__ __forceinline__ bool pass(double tx, double ty, double r2) const {
        const double du = tx - ud, dv = ty - vd;
        const double d2 = du * du + dv * dv;
        return active && (d2 <= r2);
    }
};

// tg: nt x ((double)x, (double)y, r2).  out_*: one row per map point.
__global__ __launch_bounds__(256) void k_map_match_projection(const float* __restrict__ pos, const uint4* __restrict__ desc, int n_map,
                                                              TrackViewArgs a, const uint4* __restrict__ t,
                                                              const double* __restrict__ tg, int nt, int slice,
                                                              unsigned long long* __restrict__ part, int32_t* __restrict__ part_cnt,
                                                              int32_t* __restrict__ arrive, int32_t* __restrict__ out_idx,
                                                              int32_t* __restrict__ out_dist, int32_t* __restrict__ out_cnt,
                                                              float2* __restrict__ out_px) {
    const int qi = blockIdx.x * 64 + (threadIdx.x & 63);
    const int qc = min(qi, n_map - 1);
    // the projection of k_map_in_view
    const double p[4] = {pos[3 * (size_t)qc], pos[3 * (size_t)qc + 1], pos[3 * (size_t)qc + 2], 1.0};
    double res[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += a.T[4 * r + j] * p[j];
        res[r] = acc;
    }
    const float pcx = (float)res[0], pcy = (float)res[1], pcz = (float)res[2];
    const float u = (float)(a.fx * pcx / pcz + a.cx);
    const float v = (float)(a.fy * pcy / pcz + a.cy);
    const bool in_view = !(pcz < 0) && (u > 0 && v > 0 && u < (float)a.cols && v < (float)a.rows);
    const ProjectionGate gate = {tg, (double)u, (double)v, in_view};
    const GuidedResult r = guided_knn2(gate, desc, n_map, t, nt, slice, {part, part_cnt, arrive}, out_idx, out_dist);
    if (!r.deliver) return;
    out_cnt[qi] = in_view ? r.cnt : -1;
    out_px[qi] = in_view ? make_float2(u, v) : make_float2(0.f, 0.f);
}

// n_map >= 1, 0 <= nt <= 65535 (the caller's check); out: n_map x idx[2], n_map x dist[2], n_map x px[2]
// (f32, 8-byte aligned), n_map counts
int projection_launch(mvo_ctx* ctx, const float* d_pos, const uint8_t* d_desc, int n_map, const TrackViewArgs& a, const uint8_t* d_t,
                      const double* d_tg, int nt, GuidedPartials part, int32_t* out) {
    const int ngroups = guided_groups(nt);
    ProfScope ps(ctx, "k_map_match_projection");
    hipLaunchKernelGGL(k_map_match_projection, dim3((n_map + 63) / 64, ngroups), dim3(256), 0, ctx->stream, d_pos, (const uint4*)d_desc,
                       n_map, a, (const uint4*)d_t, d_tg, nt, guided_slice(nt, ngroups), part.key, part.cnt, part.arrive, out,
                       out + 2 * (size_t)n_map, out + 6 * (size_t)n_map, (float2*)(out + 4 * (size_t)n_map));
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}
