// csrc/h_wave.h -- cv::findHomography(RANSAC) on single waves (track_kernels.hip: k_h_hypotheses, k_h_mask,
// k_h_refine).  Reference call site: estiMotionByHomography (src/geometry/motion_estimation.cpp), run on every
// frame of the monocular initialisation (src/vo/vo_addFrame.cpp:36-69).
//
// Structure of OpenCV's calib3d fundam.cpp:
//   HomographyEstimatorCallback::runKernel  normalised DLT: centroids, mean-absolute-deviation scales, the 9 x 9 L^T L
//                                           summed point by point, the eigenvector of its smallest eigenvalue,
//                                           de-normalisation, scaling by 1 / H(2,2)
//   HomographyEstimatorCallback::computeError  squared reprojection error in image 2, in float from a float copy of H
//   HomographyRefineCallback + LMSolver    10 Levenberg-Marquardt iterations on the 8 free entries, on the inliers
// Same SPMD style as pnp_wave.h (PW_LANES / PW_SYNC / uniform code outside the lane loops); canonical arithmetic:
// DESIGN.md section 9.  The eigen decompositions are the one-sided Jacobi of pnp_wave.h (jacobi_rr): L^T L padded
// with a zero row and column to 10 x 10 (the round-robin schedule needs an even size; the zero row never rotates),
// the LM's 8 x 8 systems as they are; eigenvalues = row norms of the rotated matrix, eigenvectors = the rows of the
// accumulated rotations, order = descending norm, ties by index.
//
// Declared summation order of every sum over the inliers of the refinement (centroids, scales, L^T L, J^T J,
// J^T r, |r|^2): lane l of the wave accumulates the inliers i = l, l + 64, l + 128, ... in increasing i, starting
// from 0.0; the 64 lane partials are then added in lane order 0..63, again starting from 0.0.  Per match the terms
// are added in the order the OpenCV loop adds them (x before y, L_x before L_y).  The 4-point DLT of a hypothesis
// sums its 4 points in subset order.
#ifndef MVO_H_WAVE_H
#define MVO_H_WAVE_H
#include "pnp_wave.h"

namespace pw {

constexpr int kHLanes = 64;         // one hypothesis / the whole refinement per wave
constexpr int kHPad = 10;           // L^T L padded to 10 x 10
constexpr int kHPart = 47;          // per-lane partials: 45 (L^T L or J^T J + J^T r) + |r|^2 + max|r|, odd stride
constexpr int kHLmIters = 10;       // LMSolver::create(callback, 10)

struct HDltLds {
    double At[kHPad * kHPad];
    double Vt[kHPad * kHPad];
    JacobiLds js;
    int cnt[kHLanes];
};

struct HRefLds {
    HDltLds d;
    double part[kHLanes * kHPart];
    double tot[kHPart];
};

// DLT scaffolding of runKernel: nrm = {cm.x, cm.y, cM.x, cM.y, sm.x, sm.y, sM.x, sM.y} after `s = count / s`.
// Lx / Ly of one correspondence (M in image 1, m in image 2).
PW_FN void h_dlt_rows(const double* nrm, float Mx, float My, float mx, float my, double* Lx, double* Ly) {
    const double x = (mx - nrm[0]) * nrm[4], y = (my - nrm[1]) * nrm[5];
    const double X = (Mx - nrm[2]) * nrm[6], Y = (My - nrm[3]) * nrm[7];
    Lx[0] = X;
    Lx[1] = Y;
    Lx[2] = 1;
    Lx[3] = 0;
    Lx[4] = 0;
    Lx[5] = 0;
    Lx[6] = -x * X;
    Lx[7] = -x * Y;
    Lx[8] = -x;
    Ly[0] = 0;
    Ly[1] = 0;
    Ly[2] = 0;
    Ly[3] = X;
    Ly[4] = Y;
    Ly[5] = 1;
    Ly[6] = -y * X;
    Ly[7] = -y * Y;
    Ly[8] = -y;
}

// s.At holds L^T L (both halves, padded to 10 x 10):
// eigenvector of the smallest eigenvalue -> H0; H = invHnorm * H0 * Hnorm2, scaled by 1 / H(2,2).
PW_FN void h_dlt_finish(HDltLds& s, const double* nrm, double* H) {
    jacobi_rr<kHPad, kHPad, kHLanes>(s.At, s.Vt, s.js);
    const double* v = s.Vt + kHPad * s.js.perm[kHPad - 2];  // row 9 of the padding stays zero and ranks last
    const double invHnorm[9] = {1. / nrm[4], 0, nrm[0], 0, 1. / nrm[5], nrm[1], 0, 0, 1};
    const double Hnorm2[9] = {nrm[6], 0, -nrm[2] * nrm[6], 0, nrm[7], -nrm[3] * nrm[7], 0, 0, 1};
    double T[9], H0[9];
    PW_UNROLL
    for (int k = 0; k < 9; k++) H0[k] = v[k];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            double acc = 0;
            for (int k = 0; k < 3; k++) acc += invHnorm[3 * r + k] * H0[3 * k + c];
            T[3 * r + c] = acc;
        }
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            double acc = 0;
            for (int k = 0; k < 3; k++) acc += T[3 * r + k] * Hnorm2[3 * k + c];
            H0[3 * r + c] = acc;
        }
    const double sc = 1. / H0[8];
    PW_UNROLL
    for (int k = 0; k < 9; k++) H[k] = H0[k] * sc;
}

// runKernel's degenerate-scale rule, then count / s
PW_FN bool h_scales_ok(double* nrm, int count) {
    if (fabs(nrm[4]) < DBL_EPSILON || fabs(nrm[5]) < DBL_EPSILON || fabs(nrm[6]) < DBL_EPSILON || fabs(nrm[7]) < DBL_EPSILON)
        return false;
    for (int k = 4; k < 8; k++) nrm[k] = count / nrm[k];
    return true;
}

// fills the padded 10 x 10 matrix from the 45 upper-triangle sums
PW_FN void h_spread_ltl(HDltLds& s, const double* ltl) {
    PW_LANES(l, kHLanes) {
        for (int e = l; e < kHPad * kHPad; e += kHLanes) {
            const int r = e / kHPad, c = e % kHPad;
            double v = 0;
            if (r < 9 && c < 9) {
                const int j = r < c ? r : c, k = r < c ? c : r;
                v = ltl[j * 9 - j * (j - 1) / 2 + (k - j)];
            }
            s.At[e] = v;
        }
    }
    PW_SYNC();
}

// runKernel on the 4 matches of a hypothesis (subset order).  false: degenerate scales (no model).
PW_FN bool h_hypothesis(HDltLds& s, const float* src, const float* dst, const int32_t* idx, double* H) {
    float M[4][2], m[4][2];
    for (int i = 0; i < 4; i++) {
        const int q = idx[i];
        M[i][0] = src[2 * q];
        M[i][1] = src[2 * q + 1];
        m[i][0] = dst[2 * q];
        m[i][1] = dst[2 * q + 1];
    }
    double nrm[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
        nrm[0] += m[i][0];
        nrm[1] += m[i][1];
        nrm[2] += M[i][0];
        nrm[3] += M[i][1];
    }
    for (int k = 0; k < 4; k++) nrm[k] /= 4;
    for (int i = 0; i < 4; i++) {
        nrm[4] += fabs(m[i][0] - nrm[0]);
        nrm[5] += fabs(m[i][1] - nrm[1]);
        nrm[6] += fabs(M[i][0] - nrm[2]);
        nrm[7] += fabs(M[i][1] - nrm[3]);
    }
    if (!h_scales_ok(nrm, 4)) return false;
    PW_LANES(l, kHLanes) {
        for (int e = l; e < kHPad * kHPad; e += kHLanes) {
            const int r = e / kHPad, c = e % kHPad;
            double acc = 0;
            if (r < 9 && c < 9) {
                const int j = r < c ? r : c, k = r < c ? c : r;
                for (int i = 0; i < 4; i++) {
                    double Lx[9], Ly[9];
                    h_dlt_rows(nrm, M[i][0], M[i][1], m[i][0], m[i][1], Lx, Ly);
                    acc += Lx[j] * Lx[k] + Ly[j] * Ly[k];
                }
            }
            s.At[e] = acc;
        }
    }
    PW_SYNC();
    h_dlt_finish(s, nrm, H);
    return true;
}

// HomographyEstimatorCallback::computeError for one match, float arithmetic on the float copy of H
PW_FN float h_error(const float* Hf, float Mx, float My, float mx, float my) {
    const float ww = 1.f / (Hf[6] * Mx + Hf[7] * My + 1.f);
    const float dx = (Hf[0] * Mx + Hf[1] * My + Hf[2]) * ww - mx;
    const float dy = (Hf[3] * Mx + Hf[4] * My + Hf[5]) * ww - my;
    return dx * dx + dy * dy;
}

PW_FN void h_to_float(const double* H, float* Hf) {
    PW_UNROLL
    for (int k = 0; k < 9; k++) Hf[k] = (float)H[k];
}

// inliers of H over all n matches (findInliers: err <= (float)(thr * thr))
PW_FN int h_count(HDltLds& s, const float* src, const float* dst, int n, const double* H, float thr2) {
    float Hf[9];
    h_to_float(H, Hf);
    PW_LANES(l, kHLanes) {
        int good = 0;
        for (int i = l; i < n; i += kHLanes)
            good += h_error(Hf, src[2 * i], src[2 * i + 1], dst[2 * i], dst[2 * i + 1]) <= thr2 ? 1 : 0;
        s.cnt[l] = good;
    }
    PW_SYNC();
    int total = 0;
    for (int q = 0; q < kHLanes; q++) total += s.cnt[q];
    PW_SYNC();
    return total;
}

// ------------------------------------------------------------------------------------------------ refinement
// The 64 lane partials p[l * kHPart + e] of entries e < ne -> s.tot[e] (lane order)
PW_FN void h_reduce(HRefLds& s, int ne) {
    PW_SYNC();
    PW_LANES(l, kHLanes) {
        if (l < ne) {
            double acc = 0;
            for (int q = 0; q < kHLanes; q++) acc += s.part[q * kHPart + l];
            s.tot[l] = acc;
        }
    }
    PW_SYNC();
}

// runKernel on the inliers (mask) in the declared block order.  false: fewer than one inlier or degenerate scales.
PW_FN bool h_dlt_inliers(HRefLds& s, const float* src, const float* dst, const uint8_t* mask, int n, double* H) {
    PW_LANES(l, kHLanes) {
        double a[5] = {0, 0, 0, 0, 0};
        for (int i = l; i < n; i += kHLanes)
            if (mask[i]) {
                a[0] += dst[2 * i];
                a[1] += dst[2 * i + 1];
                a[2] += src[2 * i];
                a[3] += src[2 * i + 1];
                a[4] += 1;
            }
        for (int e = 0; e < 5; e++) s.part[l * kHPart + e] = a[e];
    }
    h_reduce(s, 5);
    const int count = (int)s.tot[4];
    if (count < 1) return false;
    double nrm[8];
    for (int k = 0; k < 4; k++) nrm[k] = s.tot[k] / count;
    PW_SYNC();
    PW_LANES(l, kHLanes) {
        double a[4] = {0, 0, 0, 0};
        for (int i = l; i < n; i += kHLanes)
            if (mask[i]) {
                a[0] += fabs(dst[2 * i] - nrm[0]);
                a[1] += fabs(dst[2 * i + 1] - nrm[1]);
                a[2] += fabs(src[2 * i] - nrm[2]);
                a[3] += fabs(src[2 * i + 1] - nrm[3]);
            }
        for (int e = 0; e < 4; e++) s.part[l * kHPart + e] = a[e];
    }
    h_reduce(s, 4);
    for (int k = 0; k < 4; k++) nrm[4 + k] = s.tot[k];
    if (!h_scales_ok(nrm, count)) return false;
    PW_SYNC();
    PW_LANES(l, kHLanes) {
        double a[45];
        for (int e = 0; e < 45; e++) a[e] = 0;
        for (int i = l; i < n; i += kHLanes)
            if (mask[i]) {
                double Lx[9], Ly[9];
                h_dlt_rows(nrm, src[2 * i], src[2 * i + 1], dst[2 * i], dst[2 * i + 1], Lx, Ly);
                int e = 0;
                for (int j = 0; j < 9; j++)
                    for (int k = j; k < 9; k++, e++) a[e] += Lx[j] * Lx[k] + Ly[j] * Ly[k];
            }
        for (int e = 0; e < 45; e++) s.part[l * kHPart + e] = a[e];
    }
    h_reduce(s, 45);
    double ltl[45];
    for (int e = 0; e < 45; e++) ltl[e] = s.tot[e];
    h_spread_ltl(s.d, ltl);
    h_dlt_finish(s.d, nrm, H);
    return true;
}

// HomographyRefineCallback::compute over the inliers: S = |r|^2, rinf = max |r_i|; with `jac` also J^T J (upper
// triangle, 36) and J^T r (8).
PW_FN void h_lm_compute(HRefLds& s, const float* src, const float* dst, const uint8_t* mask, int n, const double* h,
                        bool jac, double* S, double* rinf, double* JtJ, double* Jtr) {
    PW_LANES(l, kHLanes) {
        double a[46], mx = 0;
        for (int e = 0; e < 46; e++) a[e] = 0;
        for (int i = l; i < n; i += kHLanes)
            if (mask[i]) {
                const float Mx = src[2 * i], My = src[2 * i + 1];
                double ww = h[6] * Mx + h[7] * My + 1.;
                ww = fabs(ww) > DBL_EPSILON ? 1. / ww : 0;
                const double xi = (h[0] * Mx + h[1] * My + h[2]) * ww;
                const double yi = (h[3] * Mx + h[4] * My + h[5]) * ww;
                const double ex = xi - dst[2 * i], ey = yi - dst[2 * i + 1];
                a[45] += ex * ex;
                a[45] += ey * ey;
                const double ax = fabs(ex), ay = fabs(ey);
                mx = ax > mx ? ax : mx;
                mx = ay > mx ? ay : mx;
                if (jac) {
                    const double Jx[8] = {Mx * ww, My * ww, ww, 0, 0, 0, -Mx * ww * xi, -My * ww * xi};
                    const double Jy[8] = {0, 0, 0, Mx * ww, My * ww, ww, -Mx * ww * yi, -My * ww * yi};
                    int e = 0;
                    for (int j = 0; j < 8; j++)
                        for (int k = j; k < 8; k++, e++) {
                            a[e] += Jx[j] * Jx[k];
                            a[e] += Jy[j] * Jy[k];
                        }
                    for (int j = 0; j < 8; j++) {
                        a[36 + j] += Jx[j] * ex;
                        a[36 + j] += Jy[j] * ey;
                    }
                }
            }
        for (int e = 0; e < 46; e++) s.part[l * kHPart + e] = a[e];
        s.part[l * kHPart + 46] = mx;
    }
    PW_SYNC();
    PW_LANES(l, kHLanes) {
        if (l < kHPart) {
            double acc = 0;
            for (int q = 0; q < kHLanes; q++) {
                const double v = s.part[q * kHPart + l];
                acc = l == 46 ? (v > acc ? v : acc) : acc + v;
            }
            s.tot[l] = acc;
        }
    }
    PW_SYNC();
    *S = s.tot[45];
    *rinf = s.tot[46];
    if (jac) {
        for (int e = 0; e < 36; e++) JtJ[e] = s.tot[e];
        for (int j = 0; j < 8; j++) Jtr[j] = s.tot[36 + j];
    }
    PW_SYNC();
}

// Symmetric 8 x 8 eigen decomposition (DECOMP_EIG) by jacobi_rr: w[i] descending, E rows = eigenvectors.
PW_FN void h_eig8(HDltLds& s, const double* A, double* w, double* E) {
    PW_LANES(l, kHLanes) { s.At[l] = A[l]; }
    PW_SYNC();
    jacobi_rr<8, 8, kHLanes>(s.At, s.Vt, s.js);
    for (int i = 0; i < 8; i++) {
        const int src = s.js.perm[i];
        w[i] = s.js.W[src];
        for (int k = 0; k < 8; k++) E[8 * i + k] = s.Vt[8 * src + k];
    }
    PW_SYNC();
}

// SVBkSb's threshold: sum of the eigenvalues (descending order) times 2 DBL_EPSILON
PW_FN double h_eig_thr(const double* w) {
    double thr = 0;
    for (int i = 0; i < 8; i++) thr += w[i];
    return thr * (DBL_EPSILON * 2);
}

PW_FN void h_unpack8(const double* up, double* A) {
    int e = 0;
    for (int j = 0; j < 8; j++)
        for (int k = j; k < 8; k++, e++) {
            A[8 * j + k] = up[e];
            A[8 * k + j] = up[e];
        }
}

// LMSolverImpl::run (OpenCV 4.x calib3d levmarq.cpp) on x[8], HomographyRefineCallback, maxIters 10,
// eps = FLT_EPSILON.  Returns the iteration count.
PW_FN int h_refine_lm(HRefLds& s, const float* src, const float* dst, const uint8_t* mask, int n, double* x) {
    double S, rinf, JtJu[36], v[8], A[64], D[8];
    h_lm_compute(s, src, dst, mask, n, x, true, &S, &rinf, JtJu, v);
    h_unpack8(JtJu, A);
    for (int i = 0; i < 8; i++) D[i] = A[9 * i];
    const double Rlo = 0.25, Rhi = 0.75;
    double lambda = 1, lc = 0.75;
    int iter = 0;
    for (;;) {
        double Ap[64], w[8], E[64], d[8], xd[8];
        for (int k = 0; k < 64; k++) Ap[k] = A[k];
        for (int i = 0; i < 8; i++) Ap[9 * i] += lambda * D[i];
        // solve(Ap, v, d, DECOMP_EIG)
        h_eig8(s.d, Ap, w, E);
        const double thr = h_eig_thr(w);
        for (int k = 0; k < 8; k++) d[k] = 0;
        for (int i = 0; i < 8; i++) {
            if (fabs(w[i]) <= thr) continue;
            const double wi = 1 / w[i];
            double sd = 0;
            for (int j = 0; j < 8; j++) sd += E[8 * i + j] * v[j];
            sd *= wi;
            for (int k = 0; k < 8; k++) d[k] += sd * E[8 * i + k];
        }
        for (int k = 0; k < 8; k++) xd[k] = x[k] - d[k];
        double Sd, rdinf;
        h_lm_compute(s, src, dst, mask, n, xd, false, &Sd, &rdinf, nullptr, nullptr);
        // dS = d . (2 v - A d)
        double dS = 0;
        for (int i = 0; i < 8; i++) {
            double Ad = 0;
            for (int k = 0; k < 8; k++) Ad += A[8 * i + k] * d[k];
            const double td = -Ad + 2 * v[i];
            dS += d[i] * td;
        }
        const double R = (S - Sd) / (fabs(dS) > DBL_EPSILON ? dS : 1);
        if (R > Rhi) {
            lambda *= 0.5;
            if (lambda < lc) lambda = 0;
        } else if (R < Rlo) {
            double t = 0;
            for (int k = 0; k < 8; k++) t += d[k] * v[k];
            double nu = (Sd - S) / (fabs(t) > DBL_EPSILON ? t : 1) + 2;
            nu = nu < 2. ? 2. : nu > 10. ? 10. : nu;
            if (lambda == 0) {
                // invert(A, Ap, DECOMP_EIG): only the diagonal is read
                h_eig8(s.d, A, w, E);
                const double ithr = h_eig_thr(w);
                double maxval = DBL_EPSILON;
                for (int k = 0; k < 8; k++) {
                    double dk = 0;
                    for (int i = 0; i < 8; i++) {
                        if (fabs(w[i]) <= ithr) continue;
                        dk += E[8 * i + k] * (E[8 * i + k] * (1 / w[i]));
                    }
                    maxval = fabs(dk) > maxval ? fabs(dk) : maxval;
                }
                lambda = lc = 1. / maxval;
                nu *= 0.5;
            }
            lambda *= nu;
        }
        if (Sd < S) {
            S = Sd;
            for (int k = 0; k < 8; k++) x[k] = xd[k];
            h_lm_compute(s, src, dst, mask, n, x, true, &S, &rinf, JtJu, v);
            h_unpack8(JtJu, A);
        }
        iter++;
        double dinf = 0;
        for (int k = 0; k < 8; k++) dinf = fabs(d[k]) > dinf ? fabs(d[k]) : dinf;
        const bool proceed = iter < kHLmIters && dinf >= FLT_EPSILON && rinf >= FLT_EPSILON;
        if (!proceed) break;
    }
    return iter;
}

}  // namespace pw
#endif
