// csrc/local_map_kernels.hip -- tracking the local map (include/mvo_hip.h: mvo_map_match_knn2_local*): the resident map is
// projected with the OPTIMISED pose and every map point that faces the camera within its range of distances takes its two
// nearest frame keypoints, in 256-bit Hamming space, among those of its predicted pyramid level (or the one below) within a
// radius of a few pixels at that level.  ORB-SLAM's second search, Tracking::SearchLocalPoints: Frame::isInFrustum and
// ORBmatcher::SearchByProjection(F, vpMapPoints, th).  The arithmetic is declared in DESIGN.md section 22;
// tests/local_map_numpy.py restates it.
//   k_map_match_local  one launch per call: guided_knn2() (guided_knn2.h), one lane per map point, behind this prologue and gate.
//                    prologue: the projection of k_map_in_view (track_kernels.hip), operation for operation; the distance to
//                    the camera centre, the range test, the viewing cosine, the predicted level (a count over the level
//                    table, which travels in the kernel arguments: no logarithm, no table in memory) and the squared radius,
//                    all in registers.  A point that is not active has no candidates, and a wave none of whose points is
//                    active skips its slice.  A frame keypoint is parked as (double)x, (double)y, (double)level.  gate: 5 f64
//                    operations and two compares of the level.  outputs: idx, dist (the body), the candidate count or -1, the
//                    pixel, the level, the viewing cosine.
// Every f64 operation below is one IEEE operation in the written order (the build has -ffp-contract=off).
#include "guided_knn2.h"

struct LocalMapGate {
    static constexpr bool kSkipIdleWave = true;
    const double* __restrict__ tg;
    double ud, vd, r2;
    double lv, lv_below;  // the predicted level and the one below it, as the keypoints' levels are parked
    bool active;          // in view, in range, facing, not skipped
    __device__ __forceinline__ GuidedTrain load(int j) const { return {tg[3 * (size_t)j], tg[3 * (size_t)j + 1], tg[3 * (size_t)j + 2]}; }
    __device__ __forceinline__ bool pass(double tx, double ty, double tl) const {
        const double du = tx - ud, dv = ty - vd;
        const double d2 = du * du + dv * dv;
        // (bitwise on purpose: with && and || the compiler nests four exec-mask branches around three compares per keypoint)
        return active & (d2 <= r2) & ((tl == lv) | (tl == lv_below));
    }
};

// tg: nt x ((double)x, (double)y, (double)t_level).  skip: n_map bytes.  out_*: one row per map point.
__global__ __launch_bounds__(256) void k_map_match_local(const float* __restrict__ pos, const uint4* __restrict__ desc,
                                                         const float* __restrict__ normal, const float* __restrict__ max_dist,
                                                         const uint8_t* __restrict__ skip, int n_map, LocalMapArgs a,
                                                         const uint4* __restrict__ t, const double* __restrict__ tg, int nt, int slice,
                                                         unsigned long long* __restrict__ part, int32_t* __restrict__ part_cnt,
                                                         int32_t* __restrict__ arrive, int32_t* __restrict__ out_idx,
                                                         int32_t* __restrict__ out_dist, int32_t* __restrict__ out_cnt,
                                                         float2* __restrict__ out_px, int32_t* __restrict__ out_lv,
                                                         double* __restrict__ out_vc) {
    const int qi = blockIdx.x * 64 + (threadIdx.x & 63);
    const int qc = min(qi, n_map - 1);
    // the projection of k_map_in_view
    const double p[4] = {pos[3 * (size_t)qc], pos[3 * (size_t)qc + 1], pos[3 * (size_t)qc + 2], 1.0};
    double res[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += a.view.T[4 * r + j] * p[j];
        res[r] = acc;
    }
    const float pcx = (float)res[0], pcy = (float)res[1], pcz = (float)res[2];
    const float u = (float)(a.view.fx * pcx / pcz + a.view.cx);
    const float v = (float)(a.view.fy * pcy / pcz + a.view.cy);
    const bool in_view = !(pcz < 0) && (u > 0 && v > 0 && u < (float)a.view.cols && v < (float)a.view.rows);
    // the distance to the camera centre and the range the point was made for
    const double dx = p[0] - a.O[0], dy = p[1] - a.O[1], dz = p[2] - a.O[2];
    double s = dx * dx;
    s = s + dy * dy;
    s = s + dz * dz;
    const double dist = sqrt(s);
    const double md = (double)max_dist[qc];
    const double lo = 0.8 * (md / a.level_scale[LM_MAX_LEVELS - 1]);  // (entries behind n_levels repeat the last level's)
    const double hi = 1.2 * md;
    const bool in_range = md > 0 && dist >= lo && dist <= hi;
    // the viewing cosine against the mean normal
    const double nx = (double)normal[3 * (size_t)qc], ny = (double)normal[3 * (size_t)qc + 1], nz = (double)normal[3 * (size_t)qc + 2];
    const double dot = (dx * nx + dy * ny) + dz * nz;
    const double vc = dot / dist;
    const bool facing = vc >= a.min_view_cos;
    // the predicted level: a count, and the scale of that level by selects (no indexed read of the argument table)
    int lv = 0;
#pragma unroll
    for (int l = 0; l < LM_MAX_LEVELS - 1; ++l) lv += (l < a.n_levels - 1 && dist * a.level_scale[l] < md) ? 1 : 0;
    double ls = a.level_scale[0];
#pragma unroll
    for (int l = 1; l < LM_MAX_LEVELS; ++l) ls = (lv == l) ? a.level_scale[l] : ls;
    const double r = (((vc > a.near_cos) ? a.radius_near : a.radius_far) * a.radius_scale) * ls;
    const bool active = in_view && in_range && facing && !skip[qc];
    const LocalMapGate gate = {tg, (double)u, (double)v, r * r, (double)lv, (double)(lv - 1), active};
    const GuidedResult g = guided_knn2(gate, desc, n_map, t, nt, slice, {part, part_cnt, arrive}, out_idx, out_dist);
    if (!g.deliver) return;
    out_cnt[qi] = active ? g.cnt : -1;
    out_px[qi] = active ? make_float2(u, v) : make_float2(0.f, 0.f);
    out_lv[qi] = active ? lv : -1;
    out_vc[qi] = active ? vc : 0.0;
}

// n_map >= 1, 0 <= nt <= 65535 (the caller's check); out: n_map x idx[2], n_map x dist[2], n_map x px[2] (f32), n_map counts,
// n_map levels, n_map viewing cosines (f64: 32 n_map bytes in front keep them 8-byte aligned)
int local_map_launch(mvo_ctx* ctx, const float* d_pos, const uint8_t* d_desc, const float* d_normal, const float* d_max_dist, int n_map,
                     const LocalMapArgs& a, const uint8_t* d_t, const double* d_tg, const uint8_t* d_skip, int nt, GuidedPartials part,
                     int32_t* out) {
    const int ngroups = guided_groups(nt);
    ProfScope ps(ctx, "k_map_match_local");
    hipLaunchKernelGGL(k_map_match_local, dim3((n_map + 63) / 64, ngroups), dim3(256), 0, ctx->stream, d_pos, (const uint4*)d_desc,
                       d_normal, d_max_dist, d_skip, n_map, a, (const uint4*)d_t, d_tg, nt, guided_slice(nt, ngroups), part.key, part.cnt,
                       part.arrive, out, out + 2 * (size_t)n_map, out + 6 * (size_t)n_map, (float2*)(out + 4 * (size_t)n_map),
                       out + 7 * (size_t)n_map, (double*)(out + 8 * (size_t)n_map));
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}
