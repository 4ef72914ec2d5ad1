// csrc/epipolar_kernels.hip -- pose-guided matching (include/mvo_hip.h: mvo_match_knn2_epipolar*): the 2-NN of k_knn2
// (match_kernels.hip) in which a (query, train) pair competes only if the train keypoint lies within a tolerance of the
// query's epipolar line.  What the reference asks for and does not have (README.md:212 "doing guided matching based on
// the estimated camera motion", README.md:272 "Utilize epipolar constraint to do feature matching").  The arithmetic is
// declared in DESIGN.md section 14; tests/epipolar_numpy.py restates it.
//   k_knn2_epipolar  one launch per call.  One LANE per query: its line (a, b, c), a^2 + b^2 and its 256 descriptor bits
//                    stay in registers.  grid = (groups of 64 queries) x (train groups); a workgroup is 4 waves, each
//                    with its own train slice.  A wave parks 64 trains at a time in registers, lane j = train j: the
//                    descriptor and (double)u, (double)v, tol2, and broadcasts train j with v_readlane, as k_knn2 does.
//                    The gate comes FIRST (7 f64 operations); only when a lane of the wave passes (a few trains in a
//                    hundred) are the eight descriptor dwords broadcast and the distance taken (v_xor + v_bcnt).
//                    Passing pairs become keys (distance << 16 | train index) folded by the min / max network of
//                    k_knn2_mfma: the key order IS the tie rule (equal distances keep the lower train index).  The four
//                    waves meet in LDS; with more than one train group the partials go out write-through and the
//                    workgroup that arrives last for its query group folds them (arrival counter, self re-arming).
// Every f64 operation below is one IEEE operation in the written order (the build has -ffp-contract=off).
#include "mvo_internal.h"

#include <climits>

typedef unsigned long long u64;

#define EK_CHUNK 256  // trains per train group at which another group is opened (ek_groups)

__device__ __forceinline__ uint32_t ek_rl(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }
__device__ __forceinline__ double ek_rl(double v, int lane) {
    return __hiloint2double((int)ek_rl((uint32_t)__double2hiint(v), lane), (int)ek_rl((uint32_t)__double2loint(v), lane));
}
__device__ __forceinline__ void ek_fold(uint32_t& b0, uint32_t& b1, uint32_t o0, uint32_t o1) {  // two sorted pairs
    const uint32_t c1 = min(max(b0, o0), min(b1, o1));
    b0 = min(b0, o0);
    b1 = c1;
}

__global__ __launch_bounds__(256) void k_knn2_epipolar(const uint4* __restrict__ q, const float2* __restrict__ qxy, int nq,
                                                       const uint4* __restrict__ t, const float2* __restrict__ txy,
                                                       const double* __restrict__ tol2, int nt, EpipolarArgs A, int slice,
                                                       u64* __restrict__ part, int32_t* __restrict__ part_cnt,
                                                       int32_t* __restrict__ arrive, int32_t* __restrict__ out_idx,
                                                       int32_t* __restrict__ out_dist, int32_t* __restrict__ out_cnt) {
    __shared__ u64 lkey[4][64];
    __shared__ int32_t lcnt[4][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int qi = blockIdx.x * 64 + lane;
    const int qc = min(qi, nq - 1);
    const uint4 qa = q[2 * (size_t)qc], qb = q[2 * (size_t)qc + 1];
    const float2 p = qxy[qc];
    const double x = (double)p.x, y = (double)p.y;
    const double a = (A.f[0] * x + A.f[1] * y) + A.f[2];
    const double b = (A.f[3] * x + A.f[4] * y) + A.f[5];
    const double c = (A.f[6] * x + A.f[7] * y) + A.f[8];
    const double nrm = a * a + b * b;
    const bool line_ok = nrm > 0;  // false for NaN as well
    const int j0 = min(nt, (blockIdx.y * 4 + wave) * slice), j1 = min(nt, j0 + slice);
    uint32_t b0 = 0xffffffffu, b1 = 0xffffffffu;
    int cnt = 0;
    for (int c0 = j0; c0 < j1; c0 += 64) {
        const int cn = min(64, j1 - c0);  // wave-uniform
        const int tl = min(c0 + lane, nt - 1);
        const uint4 ta = t[2 * (size_t)tl], tb = t[2 * (size_t)tl + 1];
        const float2 tp = txy[tl];
        const double tu = (double)tp.x, tv = (double)tp.y, tt = tol2[tl];
        for (int j = 0; j < cn; ++j) {
            const double u = ek_rl(tu, j), v = ek_rl(tv, j), tol = ek_rl(tt, j);
            const double num = (a * u + b * v) + c;
            const bool pass = line_ok && (num * num <= tol * nrm);
            if (__ballot(pass) == 0) continue;  // wave-uniform: no query of this wave has train c0 + j near its line
            const uint32_t d = __popc(qa.x ^ ek_rl(ta.x, j)) + __popc(qa.y ^ ek_rl(ta.y, j)) + __popc(qa.z ^ ek_rl(ta.z, j)) +
                               __popc(qa.w ^ ek_rl(ta.w, j)) + __popc(qb.x ^ ek_rl(tb.x, j)) + __popc(qb.y ^ ek_rl(tb.y, j)) +
                               __popc(qb.z ^ ek_rl(tb.z, j)) + __popc(qb.w ^ ek_rl(tb.w, j));
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
        ek_fold(b0, b1, (uint32_t)o, (uint32_t)(o >> 32));
        cnt += lcnt[w][lane];
    }
    const int ngroups = gridDim.y;  // wave-uniform
    if (ngroups > 1) {
        if (qi < nq) {
            __hip_atomic_store(part + ((size_t)blockIdx.y * nq + qi), ((u64)b1 << 32) | b0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(part_cnt + ((size_t)blockIdx.y * nq + qi), cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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
            const u64 o = __hip_atomic_load(part + ((size_t)g * nq + qc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ek_fold(b0, b1, (uint32_t)o, (uint32_t)(o >> 32));
            cnt += __hip_atomic_load(part_cnt + ((size_t)g * nq + qc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (qi >= nq) return;
    const bool h0 = b0 != 0xffffffffu, h1 = b1 != 0xffffffffu;
    out_idx[2 * qi] = h0 ? (int)(b0 & 0xffffu) : -1;
    out_idx[2 * qi + 1] = h1 ? (int)(b1 & 0xffffu) : -1;
    out_dist[2 * qi] = h0 ? (int)(b0 >> 16) : INT_MAX;
    out_dist[2 * qi + 1] = h1 ? (int)(b1 >> 16) : INT_MAX;
    out_cnt[qi] = cnt;
}

int epipolar_groups(int nt) { return nt <= EK_CHUNK ? 1 : (nt >= EK_MAX_GROUPS * EK_CHUNK ? EK_MAX_GROUPS : (nt + EK_CHUNK - 1) / EK_CHUNK); }

// nt >= 1, nt <= 65535 (the caller's check); out: nq x (idx[2], dist[2]) then nq counts
int epipolar_launch_knn2(mvo_ctx* ctx, const uint8_t* d_q, const float* d_qxy, int nq, const uint8_t* d_t, const float* d_txy,
                         const double* d_tol2, int nt, const EpipolarArgs& a, u64* d_part, int32_t* d_part_cnt, int32_t* d_arrive,
                         int32_t* out) {
    if (nq <= 0) return MVO_OK;
    const int ngroups = epipolar_groups(nt);
    const int slice = (nt + 4 * ngroups - 1) / (4 * ngroups);
    ProfScope ps(ctx, "k_knn2_epipolar");
    hipLaunchKernelGGL(k_knn2_epipolar, dim3((nq + 63) / 64, ngroups), dim3(256), 0, ctx->stream, (const uint4*)d_q,
                       (const float2*)d_qxy, nq, (const uint4*)d_t, (const float2*)d_txy, d_tol2, nt, a, slice, d_part, d_part_cnt,
                       d_arrive, out, out + 2 * (size_t)nq, out + 4 * (size_t)nq);
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}
