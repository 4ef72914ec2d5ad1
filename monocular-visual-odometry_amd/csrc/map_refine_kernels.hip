// csrc/map_refine_kernels.hip -- a map point's position re-estimated from all its observations with the poses fixed
// (include/mvo_hip.h: mvo_map_refine_positions): the half of the alternation the bundle adjustment leaves out.  The reference
// sets the position once, from two views (vo.cpp:528-576), and its BA keeps the points fixed (config.yaml:123).  The arithmetic
// is declared in DESIGN.md section 18; tests/map_refine_numpy.py restates it.
//   k_map_refine   one launch per call.  One WAVE per map point, four waves per workgroup; lane k < m holds observation k: its
//                  pixel and the three rows of its frame's T_c_w stay in registers (the n_frames x 12 doubles are staged once
//                  per workgroup in LDS and read after the barrier).  Every lane carries the same p, lambda, H, b, chi2: the
//                  ten sums of an evaluation run over v_readlane'd terms in observation order (10 m additions whose operands
//                  are wave-uniform: the order is the contract, there is no butterfly), the 3 x 3 Cholesky is redundant per
//                  lane.  All control flow is wave-uniform; lanes m .. 63 carry a copy of the last observation, which no sum
//                  reads and the depth ballot masks.  Lane 0 writes the resident position and the per-point outputs, lane k its
//                  observation's outlier flag, straight into the ctx's pinned staging.
// Every f64 operation below is one IEEE operation in the written order (the build has -ffp-contract=off).
#include "mvo_internal.h"

__device__ __forceinline__ double mf_rl(double v, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

struct MfObs {  // one lane's observation
    double r00, r01, r02, t0, r10, r11, r12, t1, r20, r21, r22, t2;  // rows 0..2 of T_c_w of its frame
    double u, v;                                                     // (double) of the f32 pixel
};
struct MfSums {
    double h00, h01, h02, h11, h12, h22, b0, b1, b2, chi2;
};

// The m observations at (px, py, pz) -> the sums (wave-uniform), this lane's e2, and whether every observation has q_z > 0.
__device__ __forceinline__ bool mf_eval(double px, double py, double pz, const MfObs& o, const MapRefineArgs& a, int m, int lane,
                                        MfSums& S, double& e2) {
    const double qx = ((o.r00 * px + o.r01 * py) + o.r02 * pz) + o.t0;
    const double qy = ((o.r10 * px + o.r11 * py) + o.r12 * pz) + o.t1;
    const double qz = ((o.r20 * px + o.r21 * py) + o.r22 * pz) + o.t2;
    const double ax = a.fx * qx, ay = a.fy * qy;
    const double ex = (ax / qz + a.cx) - o.u;
    const double ey = (ay / qz + a.cy) - o.v;
    e2 = ex * ex + ey * ey;
    const double d2 = a.delta * a.delta;
    const double s = sqrt(e2);
    const bool inl = e2 <= d2;
    const double rho = inl ? e2 : (2.0 * a.delta) * s - d2;
    const double w = inl ? 1.0 : a.delta / s;
    const double zz = qz * qz;
    const double a0 = a.fx / qz, a2 = -(ax / zz);
    const double b1 = a.fy / qz, b2 = -(ay / zz);
    const double j00 = a0 * o.r00 + a2 * o.r20, j01 = a0 * o.r01 + a2 * o.r21, j02 = a0 * o.r02 + a2 * o.r22;
    const double j10 = b1 * o.r10 + b2 * o.r20, j11 = b1 * o.r11 + b2 * o.r21, j12 = b1 * o.r12 + b2 * o.r22;
    const double t00 = w * (j00 * j00 + j10 * j10), t01 = w * (j00 * j01 + j10 * j11), t02 = w * (j00 * j02 + j10 * j12);
    const double t11 = w * (j01 * j01 + j11 * j11), t12 = w * (j01 * j02 + j11 * j12), t22 = w * (j02 * j02 + j12 * j12);
    const double g0 = w * (j00 * ex + j10 * ey), g1 = w * (j01 * ex + j11 * ey), g2 = w * (j02 * ex + j12 * ey);
    S.h00 = S.h01 = S.h02 = S.h11 = S.h12 = S.h22 = S.b0 = S.b1 = S.b2 = S.chi2 = 0.0;
    for (int k = 0; k < m; ++k) {  // observation order
        S.h00 = S.h00 + mf_rl(t00, k);
        S.h01 = S.h01 + mf_rl(t01, k);
        S.h02 = S.h02 + mf_rl(t02, k);
        S.h11 = S.h11 + mf_rl(t11, k);
        S.h12 = S.h12 + mf_rl(t12, k);
        S.h22 = S.h22 + mf_rl(t22, k);
        S.b0 = S.b0 + mf_rl(g0, k);
        S.b1 = S.b1 + mf_rl(g1, k);
        S.b2 = S.b2 + mf_rl(g2, k);
        S.chi2 = S.chi2 + mf_rl(rho, k);
    }
    return __ballot(lane < m && !(qz > 0.0)) == 0ull;
}

// obs_start: n + 1 entries, ascending, every difference in [0, MR_MAX_OBS], the last one the number of observation rows;
// frame: every entry in [0, a.n_frames), a.n_frames <= MF_MAX_FRAMES (the host's checks).  out_*: pinned host memory.
__global__ __launch_bounds__(256) void k_map_refine(float* pos, int n, MapRefineArgs a, const double* __restrict__ Tcw,
                                                    const float* __restrict__ uv, const int32_t* __restrict__ frame,
                                                    const int32_t* __restrict__ obs_start, float* __restrict__ out_pos,
                                                    double* __restrict__ out_chi2, int32_t* __restrict__ out_info,
                                                    uint8_t* __restrict__ out_outlier) {
    __shared__ double s_T[MF_MAX_FRAMES * 12];
    for (int k = threadIdx.x; k < a.n_frames * 12; k += 256) s_T[k] = Tcw[k];
    __syncthreads();  // (every wave of the workgroup arrives: the waves past the last point leave only after it)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x * 4 + wave;  // wave-uniform
    if (i >= n) return;
    const int o0 = __builtin_amdgcn_readfirstlane(obs_start[i]);
    const int m = __builtin_amdgcn_readfirstlane(obs_start[i + 1]) - o0;
    const float fpx = pos[3 * (size_t)i], fpy = pos[3 * (size_t)i + 1], fpz = pos[3 * (size_t)i + 2];
    int status = 0, steps = 0, trials = 0;
    double px = (double)fpx, py = (double)fpy, pz = (double)fpz;
    double chi2_0 = 0.0, chi2_1 = 0.0;
    bool outlier = false;
    if (m < a.min_obs) {
        status = 1;
    } else {
        const size_t ok = (size_t)o0 + min(lane, m - 1);  // (lanes m .. 63 carry a copy of the last observation)
        const double* T = s_T + 12 * frame[ok];
        MfObs o;
        o.r00 = T[0], o.r01 = T[1], o.r02 = T[2], o.t0 = T[3];
        o.r10 = T[4], o.r11 = T[5], o.r12 = T[6], o.t1 = T[7];
        o.r20 = T[8], o.r21 = T[9], o.r22 = T[10], o.t2 = T[11];
        o.u = (double)uv[2 * ok], o.v = (double)uv[2 * ok + 1];
        MfSums S;
        double e2;
        if (!mf_eval(px, py, pz, o, a, m, lane, S, e2)) {
            status = 2;
        } else {
            chi2_0 = S.chi2;
            double mx = S.h00;
            if (S.h11 > mx) mx = S.h11;
            if (S.h22 > mx) mx = S.h22;
            double lam = 1e-3 * mx;
            if (lam > 0.0 && lam < __builtin_inf()) {
#pragma unroll 1
                while (trials < a.max_trials) {
                    ++trials;
                    bool accepted = false;
                    MfSums N;
                    double e2n = 0.0, nx = px, ny = py, nz = pz;
                    const double a00 = S.h00 + lam;
                    if (a00 > 0.0) {
                        const double l00 = sqrt(a00);
                        const double l10 = S.h01 / l00, l20 = S.h02 / l00;
                        const double p1 = (S.h11 + lam) - l10 * l10;
                        if (p1 > 0.0) {
                            const double l11 = sqrt(p1);
                            const double l21 = (S.h12 - l20 * l10) / l11;
                            const double p2 = ((S.h22 + lam) - l20 * l20) - l21 * l21;
                            if (p2 > 0.0) {
                                const double l22 = sqrt(p2);
                                const double y0 = (-S.b0) / l00;
                                const double y1 = ((-S.b1) - l10 * y0) / l11;
                                const double y2 = (((-S.b2) - l20 * y0) - l21 * y1) / l22;
                                const double d2 = y2 / l22;
                                const double d1 = (y1 - l21 * d2) / l11;
                                const double d0 = ((y0 - l10 * d1) - l20 * d2) / l00;
                                nx = px + d0, ny = py + d1, nz = pz + d2;
                                const bool front = mf_eval(nx, ny, nz, o, a, m, lane, N, e2n);
                                accepted = front && N.chi2 < S.chi2;
                            }
                        }
                    }
                    if (accepted) {
                        const double dec = S.chi2 - N.chi2;
                        const double tol = a.rel_tol * S.chi2;
                        px = nx, py = ny, pz = nz;
                        S = N;
                        e2 = e2n;
                        ++steps;
                        lam = lam * 0.1;
                        if (dec <= tol) break;
                    } else {
                        lam = lam * 10.0;
                    }
                }
            }
            status = steps > 0 ? 0 : 3;
            chi2_1 = S.chi2;
            outlier = e2 > a.delta * a.delta;
        }
    }
    if (lane < m) out_outlier[(size_t)o0 + lane] = outlier ? 1 : 0;
    if (lane == 0) {
        const float wx = status == 0 ? (float)px : fpx, wy = status == 0 ? (float)py : fpy, wz = status == 0 ? (float)pz : fpz;
        if (status == 0) pos[3 * (size_t)i] = wx, pos[3 * (size_t)i + 1] = wy, pos[3 * (size_t)i + 2] = wz;
        out_pos[3 * (size_t)i] = wx, out_pos[3 * (size_t)i + 1] = wy, out_pos[3 * (size_t)i + 2] = wz;
        out_chi2[2 * (size_t)i] = chi2_0, out_chi2[2 * (size_t)i + 1] = chi2_1;
        out_info[3 * (size_t)i] = status, out_info[3 * (size_t)i + 1] = steps, out_info[3 * (size_t)i + 2] = trials;
    }
}

// n >= 1; the inverted poses, pixels, frame indices and the n + 1 starts are on the device, the four outputs in pinned host memory
int map_refine_launch(mvo_ctx* ctx, float* d_pos, int n, const MapRefineArgs& a, const double* d_Tcw, const float* d_uv,
                      const int32_t* d_frame, const int32_t* d_obs_start, float* out_pos, double* out_chi2, int32_t* out_info,
                      uint8_t* out_outlier) {
    ProfScope ps(ctx, "k_map_refine");
    hipLaunchKernelGGL(k_map_refine, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, d_pos, n, a, d_Tcw, d_uv, d_frame, d_obs_start,
                       out_pos, out_chi2, out_info, out_outlier);
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}
