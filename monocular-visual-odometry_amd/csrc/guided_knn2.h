// csrc/guided_knn2.h -- the one body of the pose-gated Hamming 2-NN kernels (k_knn2_epipolar, k_map_match_projection): a
// (query, train) pair competes only if the kernel's GATE lets it.  A kernel is its prologue, a gate and one call of
// guided_knn2(); what the body does is the same for every gate:
//   One LANE per query: the gate's state and the 256 descriptor bits stay in registers.  grid = (groups of 64 queries) x
//   (train groups, guided_groups(nt)); a workgroup is 4 waves, each with its own slice of the trains.  A wave parks 64 trains
//   at a time in registers, lane j = train j: the descriptor and the gate's three doubles (Gate::load), and broadcasts train j
//   with v_readlane, as k_knn2 (match_kernels.hip) does.  The gate comes FIRST (Gate::pass on the three broadcast doubles);
//   only when a lane of the wave passes are the eight descriptor dwords broadcast and the distance taken (v_xor + v_bcnt).
//   Passing pairs become keys (distance << 16 | train index) folded by the min / max top-2 network (knn2_insert): the key
//   order IS the tie rule (equal distances keep the lower train index).  The four waves meet in LDS; with more than one train
//   group the partials go out write-through and the workgroup that arrives last for its query group folds them (arrival
//   counter, self re-arming).  That workgroup's first wave delivers idx / dist and hands the candidate count back to the
//   kernel, which writes its own further outputs.
// A gate has: bool active (false: this lane's query has no candidates whatever the train); static constexpr bool
// kSkipIdleWave (a wave none of whose lanes is active skips its slice); GuidedTrain load(int train) const; bool pass(double x,
// double y, double z) const.
#ifndef MVO_GUIDED_KNN2_H
#define MVO_GUIDED_KNN2_H
#include "mvo_internal.h"

#include <climits>

#define GK_CHUNK 256  // trains per train group at which another group is opened

inline int guided_groups(int nt) { return nt <= GK_CHUNK ? 1 : (nt >= GK_MAX_GROUPS * GK_CHUNK ? GK_MAX_GROUPS : (nt + GK_CHUNK - 1) / GK_CHUNK); }
inline int guided_slice(int nt, int ngroups) { return (nt + 4 * ngroups - 1) / (4 * ngroups); }  // trains per wave

__device__ __forceinline__ uint32_t knn2_rl(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }
__device__ __forceinline__ double knn2_rl(double v, int lane) {
    return __hiloint2double((int)knn2_rl((uint32_t)__double2hiint(v), lane), (int)knn2_rl((uint32_t)__double2loint(v), lane));
}
__device__ __forceinline__ void knn2_insert(uint32_t& b0, uint32_t& b1, uint32_t key) {  // one key into a sorted pair
    b1 = min(b1, max(b0, key));
    b0 = min(b0, key);
}
__device__ __forceinline__ void knn2_fold(uint32_t& b0, uint32_t& b1, uint32_t o0, uint32_t o1) {  // two sorted pairs
    const uint32_t c1 = min(max(b0, o0), min(b1, o1));
    b0 = min(b0, o0);
    b1 = c1;
}

struct GuidedTrain {  // what a gate keeps of a train, as the parking lane loads it
    double x, y, z;
};
struct GuidedResult {
    bool deliver;  // this lane writes the outputs of query blockIdx.x * 64 + lane
    int cnt;       // ... whose candidates number cnt
};

// q: nq x 32 bytes, t: nt x 32 bytes (nq >= 1, nt <= 65535); out_idx / out_dist: nq x 2
template <class Gate>
__device__ __forceinline__ GuidedResult guided_knn2(const Gate& gate, const uint4* __restrict__ q, int nq, const uint4* __restrict__ t,
                                                    int nt, int slice, GuidedPartials part, int32_t* __restrict__ out_idx,
                                                    int32_t* __restrict__ out_dist) {
    __shared__ unsigned long long lkey[4][64];
    __shared__ int32_t lcnt[4][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int qi = blockIdx.x * 64 + lane;
    const int qc = min(qi, nq - 1);
    const uint4 qa = q[2 * (size_t)qc], qb = q[2 * (size_t)qc + 1];
    const int j0 = min(nt, (blockIdx.y * 4 + wave) * slice);
    const int j1 = Gate::kSkipIdleWave && __ballot(gate.active) == 0 ? j0 : min(nt, j0 + slice);  // wave-uniform
    uint32_t b0 = 0xffffffffu, b1 = 0xffffffffu;
    int cnt = 0;
    for (int c0 = j0; c0 < j1; c0 += 64) {
        const int cn = min(64, j1 - c0);  // wave-uniform
        const int tl = min(c0 + lane, nt - 1);
        const uint4 ta = t[2 * (size_t)tl], tb = t[2 * (size_t)tl + 1];
        const GuidedTrain g = gate.load(tl);
        for (int j = 0; j < cn; ++j) {
            const bool pass = gate.pass(knn2_rl(g.x, j), knn2_rl(g.y, j), knn2_rl(g.z, j));
            if (__ballot(pass) == 0) continue;  // wave-uniform: no query of this wave lets train c0 + j through
            const uint32_t d = __popc(qa.x ^ knn2_rl(ta.x, j)) + __popc(qa.y ^ knn2_rl(ta.y, j)) + __popc(qa.z ^ knn2_rl(ta.z, j)) +
                               __popc(qa.w ^ knn2_rl(ta.w, j)) + __popc(qb.x ^ knn2_rl(tb.x, j)) + __popc(qb.y ^ knn2_rl(tb.y, j)) +
                               __popc(qb.z ^ knn2_rl(tb.z, j)) + __popc(qb.w ^ knn2_rl(tb.w, j));
            knn2_insert(b0, b1, pass ? ((d << 16) | (uint32_t)(c0 + j)) : 0xffffffffu);
            cnt += pass ? 1 : 0;
        }
    }
    lkey[wave][lane] = ((unsigned long long)b1 << 32) | b0;
    lcnt[wave][lane] = cnt;
    __syncthreads();
    if (wave != 0) return {false, 0};
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        const unsigned long long o = lkey[w][lane];
        knn2_fold(b0, b1, (uint32_t)o, (uint32_t)(o >> 32));
        cnt += lcnt[w][lane];
    }
    const int ngroups = gridDim.y;  // wave-uniform
    if (ngroups > 1) {
        if (qi < nq) {
            __hip_atomic_store(part.key + ((size_t)blockIdx.y * nq + qi), ((unsigned long long)b1 << 32) | b0, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(part.cnt + ((size_t)blockIdx.y * nq + qi), cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        MVO_WAIT_VM0();  // the write-through stores are complete before this workgroup is counted
        __builtin_amdgcn_wave_barrier();  // ... those of EVERY lane: lane 0 counts the workgroup only after all 64 have stored
        int last = 0;
        if (lane == 0) {
            last = __hip_atomic_fetch_add(part.arrive + blockIdx.x, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ngroups - 1;
            if (last) __hip_atomic_store(part.arrive + blockIdx.x, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-armed
        }
        if (!__builtin_amdgcn_readfirstlane(last)) return {false, 0};
        b0 = b1 = 0xffffffffu;
        cnt = 0;
        for (int g = 0; g < ngroups; ++g) {
            const unsigned long long o = __hip_atomic_load(part.key + ((size_t)g * nq + qc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            knn2_fold(b0, b1, (uint32_t)o, (uint32_t)(o >> 32));
            cnt += __hip_atomic_load(part.cnt + ((size_t)g * nq + qc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (qi >= nq) return {false, 0};
    const bool h0 = b0 != 0xffffffffu, h1 = b1 != 0xffffffffu;  // (a query that is not active has neither)
    out_idx[2 * qi] = h0 ? (int)(b0 & 0xffffu) : -1;
    out_idx[2 * qi + 1] = h1 ? (int)(b1 & 0xffffu) : -1;
    out_dist[2 * qi] = h0 ? (int)(b0 >> 16) : INT_MAX;
    out_dist[2 * qi + 1] = h1 ? (int)(b1 >> 16) : INT_MAX;
    return {true, cnt};
}

#endif
