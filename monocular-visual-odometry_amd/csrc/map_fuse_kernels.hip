// csrc/map_fuse_kernels.hip -- the search behind the fusion of duplicate map points (include/mvo_hip.h: mvo_map_fuse_search,
// mvo_map_fuse): every resident map point against every keypoint of every buffered frame, in one launch.  ORB-SLAM's
// ORBmatcher::Fuse projects the map points into each neighbouring keyframe in turn; the reference has no such step
// (pushCurrPointsToMap_, vo.cpp:528-576, only ever creates points).  The arithmetic is declared in DESIGN.md section 19;
// tests/map_fuse_numpy.py restates it.
//   k_map_fuse_search  grid = (groups of 64 map points) x (train groups) x (frames); blockIdx.z is the frame.  A workgroup
//                    reads its frame's row of the table (the inverted pose, the descriptors, the parked keypoints, nt, the
//                    slice) with wave-uniform loads, and is from there on k_map_match_projection (projection_kernels.hip) on
//                    that frame: the projection of k_map_in_view, the disc gate of section 15, guided_knn2() (guided_knn2.h)
//                    with its partials, arrival counters and outputs offset by the frame.  One thing more: a point already
//                    seen in the frame (bit f of its mask) is not active, exactly like a point not in view.  The train groups
//                    are chosen once from the largest frame; a frame with fewer keypoints has shorter slices, and a wave whose
//                    slice is empty falls through the loop of the body.
// Every f64 operation below is one IEEE operation in the written order (the build has -ffp-contract=off).
#include "guided_knn2.h"

struct FuseGate {  // the gate of section 15 (ProjectionGate, projection_kernels.hip)
    static constexpr bool kSkipIdleWave = true;
    const double* __restrict__ tg;
    double ud, vd;
    bool active;  // in view and not yet seen in this frame
    __device__ __forceinline__ GuidedTrain load(int j) const { return {tg[3 * (size_t)j], tg[3 * (size_t)j + 1], tg[3 * (size_t)j + 2]}; }
    __device__ __forceinline__ bool pass(double tx, double ty, double r2) const {
        const double du = tx - ud, dv = ty - vd;
        const double d2 = du * du + dv * dv;
        return active && (d2 <= r2);
    }
};

// out_*: n_frames blocks of one row per map point.  part / part_cnt: n_frames x gridDim.y x n_map; arrive: n_frames x gridDim.x
__global__ __launch_bounds__(256) void k_map_fuse_search(const float* __restrict__ pos, const uint4* __restrict__ desc, int n_map,
                                                         MapFuseArgs a, const MapFuseFrame* __restrict__ frames,
                                                         const unsigned long long* __restrict__ seen,
                                                         unsigned long long* __restrict__ part, int32_t* __restrict__ part_cnt,
                                                         int32_t* __restrict__ arrive, int32_t* __restrict__ out_idx,
                                                         int32_t* __restrict__ out_dist, int32_t* __restrict__ out_cnt,
                                                         float2* __restrict__ out_px) {
    const int f = blockIdx.z;  // workgroup-uniform: everything read through fr is a scalar load
    const MapFuseFrame& fr = frames[f];
    const int qi = blockIdx.x * 64 + (threadIdx.x & 63);
    const int qc = min(qi, n_map - 1);
    // the projection of k_map_in_view
    const double p[4] = {pos[3 * (size_t)qc], pos[3 * (size_t)qc + 1], pos[3 * (size_t)qc + 2], 1.0};
    double res[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += fr.T[4 * r + j] * p[j];
        res[r] = acc;
    }
    const float pcx = (float)res[0], pcy = (float)res[1], pcz = (float)res[2];
    const float u = (float)(a.fx * pcx / pcz + a.cx);
    const float v = (float)(a.fy * pcy / pcz + a.cy);
    const bool in_view = !(pcz < 0) && (u > 0 && v > 0 && u < (float)a.cols && v < (float)a.rows);
    const bool active = in_view && !((seen[qc] >> f) & 1ull);
    const FuseGate gate = {fr.tg, (double)u, (double)v, active};
    const size_t rows = (size_t)f * n_map;  // this frame's block of rows
    const GuidedPartials pf = {part + rows * gridDim.y, part_cnt + rows * gridDim.y, arrive + (size_t)f * gridDim.x};
    const GuidedResult r = guided_knn2(gate, desc, n_map, fr.t, fr.nt, fr.slice, pf, out_idx + 2 * rows, out_dist + 2 * rows);
    if (!r.deliver) return;
    out_cnt[rows + qi] = active ? r.cnt : -1;
    out_px[rows + qi] = active ? make_float2(u, v) : make_float2(0.f, 0.f);
}

// n_map >= 1, 1 <= n_frames <= 64, every nt <= 65535, 1 <= ngroups <= GK_MAX_GROUPS (the caller's checks); out: n_frames x n_map
// x idx[2], then as many dist[2], then as many px[2] (f32, 8-byte aligned), then n_frames x n_map counts
int map_fuse_launch(mvo_ctx* ctx, const float* d_pos, const uint8_t* d_desc, int n_map, const MapFuseArgs& a, const MapFuseFrame* d_frames,
                    int n_frames, int ngroups, const unsigned long long* d_seen, GuidedPartials part, int32_t* out) {
    const size_t rows = (size_t)n_frames * n_map;
    ProfScope ps(ctx, "k_map_fuse_search");
    hipLaunchKernelGGL(k_map_fuse_search, dim3((n_map + 63) / 64, ngroups, n_frames), dim3(256), 0, ctx->stream, d_pos,
                       (const uint4*)d_desc, n_map, a, d_frames, d_seen, part.key, part.cnt, part.arrive, out, out + 2 * rows,
                       out + 6 * rows, (float2*)(out + 4 * rows));
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}
