// csrc/map_refresh_kernels.hip -- a map point as the summary of its observations (include/mvo_hip.h: mvo_map_refresh): the
// resident descriptor becomes the medoid of the observations' descriptors (ORB-SLAM's MapPoint::ComputeDistinctiveDescriptors:
// the observation with the least median Hamming distance to the others), the normal the mean of the unit viewing directions
// (MapPoint::UpdateNormalAndDepth).  The reference copies both from the frame that created the point and never writes them
// again (vo.cpp:528-576).  The arithmetic is declared in DESIGN.md section 17; tests/map_refresh_numpy.py restates it.
//   k_map_refresh   one launch per call.  One WAVE per map point, four waves per workgroup; lane k < m holds observation k:
//                   its eight descriptor dwords and its camera centre stay in registers.  Observation j is broadcast with
//                   v_readlane (j is wave-uniform), the distance is v_xor + v_bcnt.  Lane k parks its row D[k][0 .. m-1] in
//                   its own column of the wave's 64 x 64 u16 tile in LDS (lane-contiguous: no bank conflict) and reads back
//                   only what it wrote itself, so nothing is published to another lane and no barrier is needed.  The median
//                   is found by COUNTING: the element at sorted index r is the least v with #{j : D[k][j] <= v} > r, nine
//                   halvings of [0, 256] with m LDS reads each -- no sort, no private array, no scratch.  The medoid is a
//                   wave-wide minimum over keys (med << 8 | k): the key order IS the tie rule.  The normal's sum runs over
//                   v_readlane'd values in observation order, 3 m additions whose operands are wave-uniform (every lane
//                   carries the same sum; lane 0 writes it): the order is the contract, there is no butterfly.
// Every f64 operation below is one IEEE operation in the written order (the build has -ffp-contract=off).
#include "mvo_internal.h"

__device__ __forceinline__ uint32_t mr_rl(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }
__device__ __forceinline__ double mr_rl(double v, int lane) {
    return __hiloint2double((int)mr_rl((uint32_t)__double2hiint(v), lane), (int)mr_rl((uint32_t)__double2loint(v), lane));
}

// obs_start: n + 1 entries, ascending, every difference in [0, MR_MAX_OBS], the last one the number of observation rows (the
// host's checks).  out_*: one row per map point, in pinned host memory.
__global__ __launch_bounds__(256) void k_map_refresh(const float* __restrict__ pos, uint4* desc, int n,
                                                     const uint4* __restrict__ obs_desc, const double* __restrict__ obs_cam,
                                                     const int32_t* __restrict__ obs_start, int32_t* __restrict__ out_choice,
                                                     uint4* __restrict__ out_desc, double* __restrict__ out_norm) {
    __shared__ uint16_t tile[4][MR_MAX_OBS * 64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x * 4 + wave;  // wave-uniform
    if (i >= n) return;
    const int o0 = __builtin_amdgcn_readfirstlane(obs_start[i]);
    const int m = __builtin_amdgcn_readfirstlane(obs_start[i + 1]) - o0;
    if (m == 0) {  // nothing saw the point: the resident bytes stay and are reported
        if (lane < 2) out_desc[2 * (size_t)i + lane] = desc[2 * (size_t)i + lane];
        if (lane == 0) {
            out_choice[i] = -1;
            out_norm[3 * (size_t)i] = 0.0, out_norm[3 * (size_t)i + 1] = 0.0, out_norm[3 * (size_t)i + 2] = 0.0;
        }
        return;
    }
    const size_t ok = (size_t)o0 + min(lane, m - 1);  // (lanes m .. 63 carry a copy of the last observation; their key loses)
    const uint4 qa = obs_desc[2 * ok], qb = obs_desc[2 * ok + 1];
    const double cx = obs_cam[3 * ok], cy = obs_cam[3 * ok + 1], cz = obs_cam[3 * ok + 2];
    uint16_t* col = tile[wave] + lane;
    for (int j = 0; j < m; ++j) {
        const uint32_t d = __popc(qa.x ^ mr_rl(qa.x, j)) + __popc(qa.y ^ mr_rl(qa.y, j)) + __popc(qa.z ^ mr_rl(qa.z, j)) +
                           __popc(qa.w ^ mr_rl(qa.w, j)) + __popc(qb.x ^ mr_rl(qb.x, j)) + __popc(qb.y ^ mr_rl(qb.y, j)) +
                           __popc(qb.z ^ mr_rl(qb.z, j)) + __popc(qb.w ^ mr_rl(qb.w, j));
        col[j * 64] = (uint16_t)d;
    }
    // med = the element at index r of the sorted row: the least v in [0, 256] with more than r entries <= v
    const int r = (m - 1) / 2;
    int lo = 0, hi = 256;
#pragma unroll 1
    for (int it = 0; it < 9; ++it) {  // 257 values: 9 halvings leave one
        const int mid = (lo + hi) >> 1;
        int c = 0;
        for (int j = 0; j < m; ++j) c += (int)col[j * 64] <= mid ? 1 : 0;
        const bool enough = c > r;
        hi = enough ? mid : hi;
        lo = enough ? lo : mid + 1;
    }
    uint32_t key = lane < m ? ((uint32_t)lo << 8) | (uint32_t)lane : 0xffffffffu;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) key = min(key, __shfl_xor(key, s));
    const int choice = (int)(key & 0xffu);
    if (lane == choice) {
        desc[2 * (size_t)i] = qa, desc[2 * (size_t)i + 1] = qb;
        out_desc[2 * (size_t)i] = qa, out_desc[2 * (size_t)i + 1] = qb;
    }
    // the unit viewing direction of this lane's observation
    const double px = (double)pos[3 * (size_t)i], py = (double)pos[3 * (size_t)i + 1], pz = (double)pos[3 * (size_t)i + 2];
    const double dx = px - cx, dy = py - cy, dz = pz - cz;
    double s2 = dx * dx;
    s2 = s2 + dy * dy;
    s2 = s2 + dz * dz;
    const double len = sqrt(s2);
    const double ux = dx / len, uy = dy / len, uz = dz / len;
    double Sx = 0.0, Sy = 0.0, Sz = 0.0;
    for (int k = 0; k < m; ++k) {  // observation order
        Sx = Sx + mr_rl(ux, k);
        Sy = Sy + mr_rl(uy, k);
        Sz = Sz + mr_rl(uz, k);
    }
    double t2 = Sx * Sx;
    t2 = t2 + Sy * Sy;
    t2 = t2 + Sz * Sz;
    const double tl = sqrt(t2);
    if (lane == 0) {
        out_choice[i] = choice;
        out_norm[3 * (size_t)i] = Sx / tl, out_norm[3 * (size_t)i + 1] = Sy / tl, out_norm[3 * (size_t)i + 2] = Sz / tl;
    }
}

// n >= 1; the observation arrays and the n + 1 starts are on the device, the three outputs in pinned host memory
int map_refresh_launch(mvo_ctx* ctx, const float* d_pos, uint8_t* d_desc, int n, const uint8_t* d_obs_desc, const double* d_obs_cam,
                       const int32_t* d_obs_start, int32_t* out_choice, uint8_t* out_desc, double* out_norm) {
    ProfScope ps(ctx, "k_map_refresh");
    hipLaunchKernelGGL(k_map_refresh, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, d_pos, (uint4*)d_desc, n, (const uint4*)d_obs_desc,
                       d_obs_cam, d_obs_start, out_choice, (uint4*)out_desc, out_norm);
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}
