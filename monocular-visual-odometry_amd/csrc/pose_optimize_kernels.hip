// csrc/pose_optimize_kernels.hip -- the per-frame pose from a robust motion-only optimisation over all matches
// (include/mvo_hip.h: mvo_optimize_pose): ORB-SLAM's Optimizer::PoseOptimization in place of the reference's
// cv::solvePnPRansac (poseEstimationPnP_, vo.cpp:291-347) when the matches come from a predicted pose.  The arithmetic is
// declared in DESIGN.md section 21; tests/pose_optimize_numpy.py restates it.
//   k_pose_optimize   one launch per call, ONE workgroup of 256 threads (four waves): every round, trial and classification runs
//                     inside it.  The observations are read once into LDS (six f32 planes of 4096: 96 KiB, a lane reads
//                     consecutive words, no bank conflict); thread s owns the slot s = k mod 256, i.e. observations s, s + 256,
//                     ... (at most 16): their participation and outlier flags are bits of two registers.  An evaluation adds a
//                     slot's 28 terms in ascending k, then reduces the 256 slots by the adjacent pairwise tree: six levels of
//                     __shfl_xor inside a wave (lane i adds lane i ^ 2^l: both members of a pair hold the pair's sum, IEEE
//                     addition commutes), the last two levels through LDS, (w0 + w1) + (w2 + w3).  The sums of the current state
//                     and of the trial state live in two LDS rows; the state (R, t), lambda and the counters are carried
//                     redundantly by every thread, the 6 x 6 Cholesky and the Rodrigues product run redundantly per lane from
//                     LDS broadcasts.  Every branch is taken by the whole workgroup: the decisions read LDS values that all
//                     threads see alike, a lane without an observation computes on a copy of observation n - 1 and adds 0.0.
//                     Thread 0 writes the pose, chi2, info and the per-round rows, thread s the flags of its slot, straight into
//                     the ctx's pinned staging.
// Every f64 operation below is one IEEE operation in the written order (the build has -ffp-contract=off).
#include "mvo_internal.h"

#define PW_FN __device__ __forceinline__
#define PW_LANES(l, NL) for (int l = (int)threadIdx.x, pw_once_ = 1; pw_once_; pw_once_ = 0)
#define PW_WAVES(w, NW) for (int w = (int)(threadIdx.x >> 6), pw_once_ = 1; pw_once_; pw_once_ = 0)
#define PW_SYNC() __syncthreads()
#define PW_UNROLL _Pragma("unroll")
#include "pnp_wave.h"  // pw::rodrigues_fwd, the function tests/test_wave_linalg.py holds to mpmath

namespace {

struct PoState {
    double R[9], t[3];
};

struct PoLds {
    float px[PO_MAX_OBS], py[PO_MAX_OBS], pz[PO_MAX_OBS], u[PO_MAX_OBS], v[PO_MAX_OBS], s[PO_MAX_OBS];
    double part[4][28];  // the four waves' sums of the evaluation in flight
    double S[2][28];     // reduced sums: H (21, upper, row by row), b (6), chi2; row `cur` = the state, the other = the trial
    int bad[4];          // per wave: participating observations with !(q_z > 0) in the evaluation in flight
    int cnt[4];          // per wave: inliers of the classification in flight
};

// observation k at (R, t): q, the error and c (without the kernel)
struct PoProj {
    double qx, qy, qz, ax, ay, ex, ey, sk, c;
};
__device__ __forceinline__ PoProj po_project(const PoLds& L, int k, const PoState& X, const PoseOptArgs& a) {
    const double Px = (double)L.px[k], Py = (double)L.py[k], Pz = (double)L.pz[k];
    PoProj p;
    p.qx = ((X.R[0] * Px + X.R[1] * Py) + X.R[2] * Pz) + X.t[0];
    p.qy = ((X.R[3] * Px + X.R[4] * Py) + X.R[5] * Pz) + X.t[1];
    p.qz = ((X.R[6] * Px + X.R[7] * Py) + X.R[8] * Pz) + X.t[2];
    p.ax = a.fx * p.qx, p.ay = a.fy * p.qy;
    p.ex = (p.ax / p.qz + a.cx) - (double)L.u[k];
    p.ey = (p.ay / p.qz + a.cy) - (double)L.v[k];
    p.sk = a.has_sigma ? (double)L.s[k] : 1.0;
    p.c = (p.ex * p.ex + p.ey * p.ey) * p.sk;
    return p;
}

// The 28 sums over the participating observations at X into L.S[dst]; returns whether all of them have q_z > 0.  Called by all
// 256 threads; two barriers inside, the second one after the last read of part / bad: the caller may read L.S[dst] on return.
__device__ __forceinline__ bool po_eval(PoLds& L, int n, int nj, unsigned active, const PoState& X, const PoseOptArgs& a, bool robust,
                                        int dst) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double d2 = a.delta * a.delta, two_d = 2.0 * a.delta;
    double acc[28];
#pragma unroll
    for (int i = 0; i < 28; ++i) acc[i] = 0.0;
    int bad = 0;
#pragma unroll 1
    for (int j = 0; j < nj; ++j) {
        const int k = tid + 256 * j;
        const bool part = k < n && ((active >> j) & 1u);
        const PoProj p = po_project(L, min(k, n - 1), X, a);
        const double sq = sqrt(p.c);
        const bool quad = !robust || p.c <= d2;
        const double rho = quad ? p.c : two_d * sq - d2;
        const double w = quad ? 1.0 : a.delta / sq;
        const double ws = w * p.sk;
        const double zz = p.qz * p.qz;
        const double a0 = a.fx / p.qz, a2 = -(p.ax / zz);
        const double b1 = a.fy / p.qz, b2 = -(p.ay / zz);
        const double J0[6] = {a2 * p.qy, a0 * p.qz - a2 * p.qx, -(a0 * p.qy), a0, 0.0, a2};
        const double J1[6] = {b2 * p.qy - b1 * p.qz, -(b2 * p.qx), b1 * p.qx, 0.0, b1, b2};
        int i = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c, ++i) {
                const double term = ws * (J0[r] * J0[c] + J1[r] * J1[c]);
                acc[i] = acc[i] + (part ? term : 0.0);
            }
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const double term = ws * (J0[r] * p.ex + J1[r] * p.ey);
            acc[21 + r] = acc[21 + r] + (part ? term : 0.0);
        }
        acc[27] = acc[27] + (part ? rho : 0.0);
        bad += (part && !(p.qz > 0.0)) ? 1 : 0;
    }
#pragma unroll
    for (int i = 0; i < 28; ++i) {
        double x = acc[i];
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) x = x + __shfl_xor(x, m);
        acc[i] = x;
    }
    const int wave_bad = __popcll(__ballot(bad != 0));
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 28; ++i) L.part[wave][i] = acc[i];
        L.bad[wave] = wave_bad;
    }
    __syncthreads();
    if (tid < 28) L.S[dst][tid] = (L.part[0][tid] + L.part[1][tid]) + (L.part[2][tid] + L.part[3][tid]);
    const bool front = (L.bad[0] | L.bad[1] | L.bad[2] | L.bad[3]) == 0;
    __syncthreads();
    return front;
}

// outlier = !(q_z > 0) || c > chi2_threshold of every observation at X, as bits of `out` (bit j: observation tid + 256 j; the
// bits past n are 0); an observation outside `front0` is an outlier.  Returns the number of inliers.  One barrier pair inside.
__device__ __forceinline__ int po_classify(PoLds& L, int n, int nj, unsigned front0, const PoState& X, const PoseOptArgs& a, unsigned& out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned o = 0;
    int inl = 0;
#pragma unroll 1
    for (int j = 0; j < nj; ++j) {
        const int k = tid + 256 * j;
        const PoProj p = po_project(L, min(k, n - 1), X, a);
        const bool outl = !((front0 >> j) & 1u) || !(p.qz > 0.0) || p.c > a.chi2_thr;
        if (k < n) {
            o |= (outl ? 1u : 0u) << j;
            inl += outl ? 0 : 1;
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) inl += __shfl_xor(inl, m);
    __syncthreads();
    if (lane == 0) L.cnt[wave] = inl;
    __syncthreads();
    out = o;
    return L.cnt[0] + L.cnt[1] + L.cnt[2] + L.cnt[3];
}

// (H + lam I) delta = -b by Cholesky, H and b = L.S[cur]; false if a pivot is not positive and finite
__device__ __forceinline__ bool po_solve(const double* S, double lam, double (&x)[6]) {
    double A[6][6], Lc[6][6], y[6];
    int i = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c, ++i) A[c][r] = S[i];  // the lower triangle
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = A[j][j] + lam;
#pragma unroll
        for (int k = 0; k < j; ++k) d = d - Lc[j][k] * Lc[j][k];
        ok = ok && d > 0.0 && d < __builtin_inf();
        Lc[j][j] = sqrt(d);
#pragma unroll
        for (int r = j + 1; r < 6; ++r) {
            double s = A[r][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s = s - Lc[r][k] * Lc[j][k];
            Lc[r][j] = s / Lc[j][j];
        }
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double s = -S[21 + r];
#pragma unroll
        for (int k = 0; k < r; ++k) s = s - Lc[r][k] * y[k];
        y[r] = s / Lc[r][r];
    }
#pragma unroll
    for (int r = 5; r >= 0; --r) {
        double s = y[r];
#pragma unroll
        for (int k = r + 1; k < 6; ++k) s = s - Lc[k][r] * x[k];
        x[r] = s / Lc[r][r];
    }
    return ok;
}

}  // namespace

// n in [1, PO_MAX_OBS]; p3 / p2 / sg (sg only if a.has_sigma) on the device, out / out_outlier in pinned host memory.
__global__ __launch_bounds__(256) void k_pose_optimize(const float* __restrict__ p3, const float* __restrict__ p2,
                                                       const float* __restrict__ sg, int n, PoseOptArgs a, PoseOptOut* __restrict__ out,
                                                       uint8_t* __restrict__ out_outlier) {
    __shared__ PoLds L;
    const int tid = threadIdx.x;
    const int nj = (n + 255) >> 8;  // observations per slot, at most 16
    for (int k = tid; k < n; k += 256) {
        L.px[k] = p3[3 * k], L.py[k] = p3[3 * k + 1], L.pz[k] = p3[3 * k + 2];
        L.u[k] = p2[2 * k], L.v[k] = p2[2 * k + 1];
        L.s[k] = a.has_sigma ? sg[k] : 1.0f;
    }
    __syncthreads();
    PoState X0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        X0.R[3 * r] = a.T0[4 * r], X0.R[3 * r + 1] = a.T0[4 * r + 1], X0.R[3 * r + 2] = a.T0[4 * r + 2];
        X0.t[r] = a.T0[4 * r + 3];
    }
    // in front at the initial pose: the only observations that ever take part
    unsigned front0 = 0;
#pragma unroll 1
    for (int j = 0; j < nj; ++j) {
        const int k = tid + 256 * j;
        const PoProj p = po_project(L, min(k, n - 1), X0, a);
        if (k < n && p.qz > 0.0) front0 |= 1u << j;
    }
    int n_front = __popc(front0);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) n_front += __shfl_xor(n_front, m);
    if ((tid & 63) == 0) L.cnt[tid >> 6] = n_front;
    __syncthreads();
    n_front = L.cnt[0] + L.cnt[1] + L.cnt[2] + L.cnt[3];

    int status = 0, rounds_run = 0, trials_all = 0, steps_all = 0, inliers = n_front;
    double chi2_first = 0.0, chi2_last = 0.0;
    unsigned outl = ~0u;
    PoState X = X0;
    if (n_front < a.min_inliers) {
        status = 2;
    } else {
        unsigned active = front0;
#pragma unroll 1
        for (int round = 0; round < a.rounds; ++round) {
            const bool robust = a.rounds == 1 || round + 1 < a.rounds;
            X = X0;
            int cur = 0, trials = 0, steps = 0;
            po_eval(L, n, nj, active, X, a, robust, cur);
            const double chi2_start = L.S[cur][27];
            double mx = L.S[cur][0];
            {
                const int diag[5] = {6, 11, 15, 18, 20};
#pragma unroll
                for (int i = 0; i < 5; ++i)
                    if (L.S[cur][diag[i]] > mx) mx = L.S[cur][diag[i]];
            }
            double lam = 1e-3 * mx;
#pragma unroll 1
            while (trials < a.iterations) {
                ++trials;
                double d[6];
                bool accepted = false;
                PoState N = X;
                if (po_solve(L.S[cur], lam, d)) {
                    double W[9], unused[27];
                    const double om[3] = {d[0], d[1], d[2]};
                    pw::rodrigues_fwd(om, W, unused, false);
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) N.R[3 * r + c] = (W[3 * r] * X.R[c] + W[3 * r + 1] * X.R[3 + c]) + W[3 * r + 2] * X.R[6 + c];
                        N.t[r] = ((W[3 * r] * X.t[0] + W[3 * r + 1] * X.t[1]) + W[3 * r + 2] * X.t[2]) + d[3 + r];
                    }
                    const bool front = po_eval(L, n, nj, active, N, a, robust, cur ^ 1);
                    accepted = front && L.S[cur ^ 1][27] < L.S[cur][27];
                }
                if (accepted) {
                    const double before = L.S[cur][27];
                    const double dec = before - L.S[cur ^ 1][27];
                    const double tol = a.rel_tol * before;
                    X = N;
                    cur ^= 1;
                    ++steps;
                    lam = lam * 0.1;
                    if (dec <= tol) break;
                } else {
                    lam = lam * 10.0;
                }
            }
            const double chi2_end = L.S[cur][27];
            const int in_before = inliers;
            inliers = po_classify(L, n, nj, front0, X, a, outl);
            active = ~outl;  // (the bits past n are masked by k < n wherever `active` is read)
            if (round == 0) chi2_first = chi2_start;
            chi2_last = chi2_end;
            trials_all += trials, steps_all += steps;
            if (tid == 0) {
                double* row = out->rows + 6 * round;
                row[0] = (double)in_before, row[1] = chi2_start, row[2] = chi2_end;
                row[3] = (double)trials, row[4] = (double)steps, row[5] = (double)inliers;
            }
            ++rounds_run;
            if (inliers < a.min_inliers) {
                status = 1;
                break;
            }
        }
        if (status == 0 && steps_all == 0) status = 3;
    }
#pragma unroll 1
    for (int j = 0; j < nj; ++j) {
        const int k = tid + 256 * j;
        if (k < n) out_outlier[k] = (uint8_t)((outl >> j) & 1u);
    }
    if (tid == 0) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            out->Tcw[4 * r] = X.R[3 * r], out->Tcw[4 * r + 1] = X.R[3 * r + 1], out->Tcw[4 * r + 2] = X.R[3 * r + 2];
            out->Tcw[4 * r + 3] = X.t[r];
        }
        out->chi2[0] = chi2_first, out->chi2[1] = chi2_last;
        out->info[0] = status, out->info[1] = rounds_run, out->info[2] = trials_all, out->info[3] = steps_all;
        out->info[4] = status == 2 ? 0 : inliers, out->info[5] = n_front;
    }
}

int pose_optimize_launch(mvo_ctx* ctx, const float* d_p3, const float* d_p2, const float* d_s, int n, const PoseOptArgs& a, PoseOptOut* out,
                         uint8_t* out_outlier) {
    ProfScope ps(ctx, "k_pose_optimize");
    hipLaunchKernelGGL(k_pose_optimize, dim3(1), dim3(256), 0, ctx->stream, d_p3, d_p2, d_s, n, a, out, out_outlier);
    MVO_HIP(hipGetLastError());
    return MVO_OK;
}
