// csrc/orb_distribute_kernels.hip -- gfx950 kernels of the ORB-SLAM style detector (the host side is
// orb_distribute_host.cpp).  Two launches per frame behind k_pyramid:
//   k_fast_cells   one workgroup = one cell of the cell table (about cell_size x cell_size scored pixels of one level, every
//                  level in ONE launch).  The cell's pixels plus the 3-px ring its FAST circles read are staged in LDS as dwords;
//                  quick test at min_threshold on every scored pixel, the few that pass are queued and scored densely (as in
//                  k_fast_harris); 3 x 3 non-maximum suppression on a score tile with a ring of zeros (a neighbour outside the
//                  cell counts as 0), one ballot per cell row; a workgroup-wide "some survivor reaches ini_threshold" flag picks
//                  the threshold; the survivors go row-major as 8-byte records into the cell's slot of the pinned host buffer,
//                  their count beside them.  A cell is the unit of the candidate order, so nothing has to be merged: no second
//                  pass, no protocol between workgroups.
//   k_ic_angle     one wave per KEPT key point (after the quadtree on the host: <= nfeatures + 2 nlevels of them, not every
//                  candidate): intensity-centroid moments over the 749-px disc of the raw level, cv::fastAtan2.
// Integer work except the one float expression of the angle (-ffp-contract=off, like orb_kernels.hip).
#include "mvo_internal.h"
#include "orb_device.h"

typedef unsigned long long u64;

#define DC_PATCH (DC_MAX_SCORED + 6)       // staged rows / columns of a cell: the scored pixels + 3 on every side
#define DC_PIX_DW ((DC_PATCH + 3 + 3) / 4)  // dwords per staged row: the patch starts up to 3 bytes into its first dword
#define DC_PIX_PITCH (4 * DC_PIX_DW)
#define DC_SC_PITCH 68                     // bytes per row of the score tile (scored pixels + ring <= 65)
static_assert(DC_MAX_SCORED <= 63, "one 64-bit ballot per cell row, one lane per cell row in the scan");
static_assert(DC_MAX_SCORED + 2 <= DC_SC_PITCH && (DC_MAX_SCORED + 2) * (DC_MAX_SCORED + 2) < 65536, "score tile / queue entries");

__global__ __launch_bounds__(256) void k_fast_cells(const uint8_t* __restrict__ raw, PyrInfo P, const DistCell* __restrict__ cells,
                                                    int thr_min, int thr_ini, int32_t* __restrict__ counts,
                                                    u64* __restrict__ records) {
    __shared__ uint32_t pix[DC_PATCH * DC_PIX_DW];
    __shared__ uint8_t sc[(DC_MAX_SCORED + 2) * DC_SC_PITCH];
    __shared__ uint16_t fq[DC_MAX_SCORED * DC_MAX_SCORED];
    __shared__ int fq_n;
    __shared__ u64 rowmask[64], rowstrong[64];
    __shared__ int rowstart[64];
    const int tid = threadIdx.x;
    const DistCell cell = cells[blockIdx.x];
    const LevelInfo L = P.lv[cell.level];
    const int sw = cell.pw - 6, sh = cell.ph - 6;  // scored pixels: 1 .. DC_MAX_SCORED each way (checked by the host)
    // stage ph rows of the patch; every row starts at the dword that holds bordered column x0 + MVO_BORDER (inside the level's
    // frame and its 64-byte row stride: x0 + pw <= w - 16)
    const int bx = cell.x0 + MVO_BORDER, xoff = bx & 3;
    const int ndw = (xoff + cell.pw + 3) >> 2;
    const uint8_t* base = raw + L.off + (size_t)(cell.y0 + MVO_BORDER) * L.stride + (bx & ~3);
    for (int i = tid; i < cell.ph * ndw; i += 256) {
        const int r = i / ndw, c = i - r * ndw;
        pix[r * DC_PIX_DW + c] = *reinterpret_cast<const uint32_t*>(base + (size_t)r * L.stride + 4 * c);
    }
    if (tid == 0) fq_n = 0;
    __syncthreads();
    const uint8_t* pb = reinterpret_cast<const uint8_t*>(pix) + xoff;  // pb[r * DC_PIX_PITCH + c] = level pixel (x0 + c, y0 + r)
    constexpr int CX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
    constexpr int CY[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
    // score tile (sh + 2) x (sw + 2): entry (sr, sx) is scored pixel (sx - 1, sr - 1) = patch position (sr + 2, sx + 2); its ring
    // is written as zeros
    const int tw = sw + 2, nt = (sh + 2) * tw;
    for (int i0 = 0; i0 < nt; i0 += 256) {
        const int i = i0 + tid;
        bool pass = false;
        if (i < nt) {
            const int sr = i / tw, sx = i - sr * tw;
            if (sr >= 1 && sr <= sh && sx >= 1 && sx <= sw) {
                const uint8_t* c = pb + (sr + 2) * DC_PIX_PITCH + (sx + 2);
                const int v = c[0];
                int d[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) d[k] = v - (int)c[CX[k] + CY[k] * DC_PIX_PITCH];
                pass = fast_quick_test(d, thr_min);
            }
            if (!pass) sc[sr * DC_SC_PITCH + sx] = 0;
        }
        const u64 pm = __ballot(pass);
        if (pm) {  // (wave-uniform) one LDS atomic per wave, the lanes take consecutive places
            int at = 0;
            if ((tid & 63) == 0) at = __hip_atomic_fetch_add(&fq_n, (int)__popcll(pm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            at = __shfl(at, 0);
            if (pass) fq[at + (int)__popcll(pm & ((1ull << (tid & 63)) - 1))] = (uint16_t)i;
        }
    }
    __syncthreads();
    for (int q = tid; q < fq_n; q += 256) {
        const int i = fq[q];
        const int sr = i / tw, sx = i - sr * tw;
        const uint8_t* c = pb + (sr + 2) * DC_PIX_PITCH + (sx + 2);
        const int v = c[0];
        int d[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) d[k] = v - (int)c[CX[k] + CY[k] * DC_PIX_PITCH];
        sc[sr * DC_SC_PITCH + sx] = (uint8_t)fast_score_full(d, thr_min);
    }
    __syncthreads();
    // non-maximum suppression: lane = column of the cell, wave = every fourth row; the suppression does not depend on the
    // threshold, so the survivors at min_threshold and those of them that reach ini_threshold come from one pass
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int ly = wave; ly < sh; ly += 4) {
        bool flag = false, strong = false;
        if (lane < sw) {
            const uint8_t* s = sc + (ly + 1) * DC_SC_PITCH + (lane + 1);
            const int v = s[0];
            flag = v > 0 && v > s[-1] && v > s[1] && v > s[-DC_SC_PITCH - 1] && v > s[-DC_SC_PITCH] && v > s[-DC_SC_PITCH + 1] &&
                   v > s[DC_SC_PITCH - 1] && v > s[DC_SC_PITCH] && v > s[DC_SC_PITCH + 1];
            strong = flag && v >= thr_ini;
        }
        const u64 m = __ballot(flag), ms = __ballot(strong);
        if (lane == 0) {
            rowmask[ly] = m;
            rowstrong[ly] = ms;
        }
    }
    __syncthreads();
    if (tid < 64) {  // lane = cell row: the threshold of the cell, then an exclusive scan of the row counts
        const u64 ms = tid < sh ? rowstrong[tid] : 0ull;
        const bool any_strong = __ballot(ms != 0) != 0;
        const u64 m = tid < sh ? (any_strong ? ms : rowmask[tid]) : 0ull;
        rowmask[tid] = m;
        const int cnt = (int)__popcll(m);
        int inc = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(inc, o);
            if (lane >= o) inc += u;
        }
        rowstart[tid] = inc - cnt;
        if (tid == 63) counts[blockIdx.x] = min(inc, cell.cap);
    }
    __syncthreads();
    u64* out = records + cell.slot;
    for (int ly = wave; ly < sh; ly += 4) {
        const u64 m = rowmask[ly];
        if ((m >> lane) & 1) {
            const int k = rowstart[ly] + (int)__popcll(m & ((1ull << lane) - 1));
            const unsigned xy = (unsigned)(cell.x0 + 3 + lane) | (unsigned)(cell.y0 + 3 + ly) << 16;
            const unsigned ls = (unsigned)cell.level << 16 | sc[(ly + 1) * DC_SC_PITCH + (lane + 1)];
            // (strict 3 x 3 maxima: at most cap of them; the slot is host memory, one 8-byte store per record)
            if (k < cell.cap) out[k] = (u64)xy | (u64)ls << 32;
        }
    }
}

// One wave per kept key point: m10 = sum u I, m01 = sum v I over the disc of the RAW level (its 15-px reach stays inside the
// level: x, y >= edge_threshold >= 19), the same integer sums and float expression as k_fast_harris.
__global__ __launch_bounds__(256) void k_ic_angle(const uint8_t* __restrict__ raw, PyrInfo P, const signed char* __restrict__ disc,
                                                  int ndisc, const u64* __restrict__ kps, int n, float* __restrict__ angles) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ki = blockIdx.x * 4 + wave;
    if (ki >= n) return;
    const u64 rec = kps[ki];
    const int x = (int)(rec & 0xffffu), y = (int)((rec >> 16) & 0xffffu);
    const LevelInfo L = P.lv[__builtin_amdgcn_readfirstlane((int)(rec >> 48))];  // (wave-uniform: scalar loads)
    const uint8_t* c = raw + L.off + (size_t)(y + MVO_BORDER) * L.stride + (x + MVO_BORDER);
    int m10 = 0, m01 = 0;
    for (int k = lane; k < ndisc; k += 64) {
        const int u = disc[2 * k], v = disc[2 * k + 1];
        const int val = c[v * L.stride + u];
        m10 += u * val;
        m01 += v * val;
    }
    m10 = wave_sum(m10);
    m01 = wave_sum(m01);
    if (lane == 0) angles[ki] = fast_atan2_deg((float)m01, (float)m10);
}

// ================================================================================================ launchers
// counts / records: the pinned host buffer (one int32 per cell, the cells' record slots)
int dist_launch_cells(mvo_ctx* ctx, const DistCell* d_cells, int n_cells, int thr_min, int thr_ini, int32_t* counts,
                      DistRecord* records) {
    if (n_cells <= 0) return MVO_OK;
    ProfScope ps(ctx, "k_fast_cells");
    hipLaunchKernelGGL(k_fast_cells, dim3(n_cells), dim3(256), 0, ctx->stream, ctx->d_raw, ctx->pyr, d_cells, thr_min, thr_ini, counts,
                       reinterpret_cast<u64*>(records));
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}

// kps / angles: pinned host memory (one 8-byte load and one 4-byte store per wave: no copy dispatch)
int dist_launch_ic_angle(mvo_ctx* ctx, const signed char* d_disc, int disc_n, const DistRecord* kps, int n, float* angles) {
    if (n <= 0) return MVO_OK;
    ProfScope ps(ctx, "k_ic_angle");
    hipLaunchKernelGGL(k_ic_angle, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, ctx->d_raw, ctx->pyr, d_disc, disc_n,
                       reinterpret_cast<const u64*>(kps), n, angles);
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}
