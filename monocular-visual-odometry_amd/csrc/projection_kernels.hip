// csrc/projection_kernels.hip -- tracking by projection (include/mvo_hip.h: mvo_map_match_knn2_projection*): the resident map
// is projected with a predicted pose and every map point in view takes its two nearest frame keypoints, in 256-bit Hamming
// space, among those within a radius of its projection.  The guided matching the reference asks for (README.md:212 "doing
// guided matching based on the estimated camera motion") on the step that runs on every frame (vo.cpp:267-289).  The
// arithmetic is declared in DESIGN.md section 15; tests/projection_numpy.py restates it.
//   k_map_match_projection  one launch per call; it stands for k_map_in_view, the compaction, the descriptor gather and the
//                    matcher launch.  One LANE per map point: the prologue is the projection of k_map_in_view
//                    (track_kernels.hip), operation for operation; u, v, in_view and the 256 descriptor bits stay in
//                    registers.  grid = (groups of 64 map points) x (train groups); a workgroup is 4 waves, each with its
//                    own slice of the frame keypoints.  A wave parks 64 keypoints at a time, lane j = keypoint j: the
//                    descriptor and (double)x, (double)y, r2, and broadcasts keypoint j with v_readlane.  The gate comes
//                    FIRST (5 f64 operations); only where a lane of the wave passes (a disc of a few px holds one or two
//                    keypoints in two thousand) are the eight descriptor dwords broadcast and the distance taken.  Keys
//                    (distance << 16 | train index) go through the min / max top-2 network: the key order IS the tie rule.
//                    A wave none of whose points is in view skips its slice.  The four waves meet in LDS; with more than
//                    one train group the partials go out write-through and the workgroup that arrives last for its group
//                    of map points folds them (arrival counter, self re-arming), as k_knn2_epipolar does.
// Every f64 operation below is one IEEE operation in the written order (the build has -ffp-contract=off).
#include "mvo_internal.h"

#include <climits>

typedef unsigned long long u64;

#define PK_CHUNK 256  // trains per train group at which another group is opened (projection_groups)

__device__ __forceinline__ uint32_t pk_rl(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }
__device__ __forceinline__ double pk_rl(double v, int lane) {
    return __hiloint2double((int)pk_rl((uint32_t)__double2hiint(v), lane), (int)pk_rl((uint32_t)__double2loint(v), lane));
}
__device__ __forceinline__ void pk_fold(uint32_t& b0, uint32_t& b1, uint32_t o0, uint32_t o1) {  // two sorted pairs
    const uint32_t c1 = min(max(b0, o0), min(b1, o1));
    b0 = min(b0, o0);
    b1 = c1;
}

// tg: nt x ((double)x, (double)y, r2).  out_*: one row per map point.
__global__ __launch_bounds__(256) void k_map_match_projection(const float* __restrict__ pos, const uint4* __restrict__ desc, int n_map,
                                                              TrackViewArgs a, const uint4* __restrict__ t,
                                                              const double* __restrict__ tg, int nt, int slice,
                                                              u64* __restrict__ part, int32_t* __restrict__ part_cnt,
                                                              int32_t* __restrict__ arrive, int32_t* __restrict__ out_idx,
                                                              int32_t* __restrict__ out_dist, int32_t* __restrict__ out_cnt,
                                                              float2* __restrict__ out_px) {
    __shared__ u64 lkey[4][64];
    __shared__ int32_t lcnt[4][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int qi = blockIdx.x * 64 + lane;
    const int qc = min(qi, n_map - 1);
    const uint4 qa = desc[2 * (size_t)qc], qb = desc[2 * (size_t)qc + 1];
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
    const double ud = (double)u, vd = (double)v;
    const int j0 = min(nt, (blockIdx.y * 4 + wave) * slice);
    const int j1 = __ballot(in_view) == 0 ? j0 : min(nt, j0 + slice);  // wave-uniform
    uint32_t b0 = 0xffffffffu, b1 = 0xffffffffu;
    int cnt = 0;
    for (int c0 = j0; c0 < j1; c0 += 64) {
        const int cn = min(64, j1 - c0);  // wave-uniform
        const int tl = min(c0 + lane, nt - 1);
        const uint4 ta = t[2 * (size_t)tl], tb = t[2 * (size_t)tl + 1];
        const double tx = tg[3 * (size_t)tl], ty = tg[3 * (size_t)tl + 1], tr = tg[3 * (size_t)tl + 2];
        for (int j = 0; j < cn; ++j) {
            const double du = pk_rl(tx, j) - ud, dv = pk_rl(ty, j) - vd;
            const double d2 = du * du + dv * dv, r2 = pk_rl(tr, j);
            const bool pass = in_view && (d2 <= r2);
            if (__ballot(pass) == 0) continue;  // wave-uniform: no map point of this wave projects near keypoint c0 + j
            const uint32_t d = __popc(qa.x ^ pk_rl(ta.x, j)) + __popc(qa.y ^ pk_rl(ta.y, j)) + __popc(qa.z ^ pk_rl(ta.z, j)) +
                               __popc(qa.w ^ pk_rl(ta.w, j)) + __popc(qb.x ^ pk_rl(tb.x, j)) + __popc(qb.y ^ pk_rl(tb.y, j)) +
                               __popc(qb.z ^ pk_rl(tb.z, j)) + __popc(qb.w ^ pk_rl(tb.w, j));
            const uint32_t key = pass ? ((d << 16) | (uint32_t)(c0 + j)) : 0xffffffffu;
            b1 = min(b1, max(b0, key));
            b0 = min(b0, key);
            cnt += pass ? 1 : 0;
        }
    }
    lkey[wave][lane] = ((u64)b1 << 32) | b0;
    lcnt[wave][lane] = cnt;
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        const u64 o = lkey[w][lane];
        pk_fold(b0, b1, (uint32_t)o, (uint32_t)(o >> 32));
        cnt += lcnt[w][lane];
    }
    const int ngroups = gridDim.y;  // wave-uniform
    if (ngroups > 1) {
        if (qi < n_map) {
            __hip_atomic_store(part + ((size_t)blockIdx.y * n_map + qi), ((u64)b1 << 32) | b0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(part_cnt + ((size_t)blockIdx.y * n_map + qi), cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        MVO_WAIT_VM0();  // the write-through stores are complete before this workgroup is counted
        __builtin_amdgcn_wave_barrier();  // ... those of EVERY lane: lane 0 counts the workgroup only after all 64 have stored
        int last = 0;
        if (lane == 0) {
            last = __hip_atomic_fetch_add(arrive + blockIdx.x, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ngroups - 1;
            if (last) __hip_atomic_store(arrive + blockIdx.x, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-armed
        }
        if (!__builtin_amdgcn_readfirstlane(last)) return;
        b0 = b1 = 0xffffffffu;
        cnt = 0;
        for (int g = 0; g < ngroups; ++g) {
            const u64 o = __hip_atomic_load(part + ((size_t)g * n_map + qc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            pk_fold(b0, b1, (uint32_t)o, (uint32_t)(o >> 32));
            cnt += __hip_atomic_load(part_cnt + ((size_t)g * n_map + qc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (qi >= n_map) return;
    const bool h0 = b0 != 0xffffffffu, h1 = b1 != 0xffffffffu;  // (a point not in view has neither)
    out_idx[2 * qi] = h0 ? (int)(b0 & 0xffffu) : -1;
    out_idx[2 * qi + 1] = h1 ? (int)(b1 & 0xffffu) : -1;
    out_dist[2 * qi] = h0 ? (int)(b0 >> 16) : INT_MAX;
    out_dist[2 * qi + 1] = h1 ? (int)(b1 >> 16) : INT_MAX;
    out_cnt[qi] = in_view ? cnt : -1;
    out_px[qi] = in_view ? make_float2(u, v) : make_float2(0.f, 0.f);
}

int projection_groups(int nt) { return nt <= PK_CHUNK ? 1 : (nt >= PK_MAX_GROUPS * PK_CHUNK ? PK_MAX_GROUPS : (nt + PK_CHUNK - 1) / PK_CHUNK); }

// n_map >= 1, 0 <= nt <= 65535 (the caller's check); out: n_map x idx[2], n_map x dist[2], n_map x px[2]
// (f32, 8-byte aligned), n_map counts
int projection_launch(mvo_ctx* ctx, const float* d_pos, const uint8_t* d_desc, int n_map, const TrackViewArgs& a, const uint8_t* d_t,
                      const double* d_tg, int nt, u64* d_part, int32_t* d_part_cnt, int32_t* d_arrive, int32_t* out) {
    const int ngroups = projection_groups(nt);
    const int slice = (nt + 4 * ngroups - 1) / (4 * ngroups);
    ProfScope ps(ctx, "k_map_match_projection");
    hipLaunchKernelGGL(k_map_match_projection, dim3((n_map + 63) / 64, ngroups), dim3(256), 0, ctx->stream, d_pos, (const uint4*)d_desc,
                       n_map, a, (const uint4*)d_t, d_tg, nt, slice, d_part, d_part_cnt, d_arrive, out, out + 2 * (size_t)n_map,
                       out + 6 * (size_t)n_map, (float2*)(out + 4 * (size_t)n_map));
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}
