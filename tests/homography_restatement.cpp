// tests/homography_restatement.cpp -- TEST INFRASTRUCTURE: cv::findHomography(RANSAC) restated sequentially, in
// the canonical arithmetic the device declares in csrc/h_wave.h (compiled by tests/h_restate.py with
// g++ -ffp-contract=off).  OpenCV 4.x calib3d (fundam.cpp, ptsetreg.cpp, levmarq.cpp) is the model:
//   getSubset / checkSubset      cv::RNG((uint64)-1), distinct indices, haveCollinearPoints on the triples with the
//                                last point, triangle orientations all or none, maxAttempts 1000
//   runKernel                    normalised DLT, eigenvector of the smallest eigenvalue of L^T L, / H(2,2)
//   computeError / findInliers   float, err <= (float)(thr * thr)
//   RANSACPointSetRegistrator::run with RANSACUpdateNumIters, then the DLT re-fit on the inliers and LMSolverImpl
// Sums over the inliers of the refinement run in the declared block order: partial l takes i = l, l + 64, ... in
// increasing i, the 64 partials are added in order.  Eigen decompositions: one-sided Jacobi, round-robin pairs.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../oracle/linalg_oracle.h"

using orc_linalg::CvRng;
using orc_linalg::jacobi_pair;
using orc_linalg::rr_pair;

namespace {

constexpr int kLanes = 64;

// jacobi_rr of csrc/pnp_wave.h, sequentially: round-robin rounds, stop after a sweep without rotation; W = row norms,
// perm = stable descending order
void jacobi_rr(double* At, int n, int m, double* Vt, double* W, int* perm) {
    for (int i = 0; i < n; i++)
        for (int k = 0; k < n; k++) Vt[i * n + k] = i == k ? 1.0 : 0.0;
    const int max_iter = m > 30 ? m : 30;
    for (int it = 0; it < max_iter; it++) {
        bool changed = false;
        for (int r = 0; r < n - 1; r++)
            for (int k = 0; k < n / 2; k++) {
                int i, j;
                rr_pair(n, r, k, &i, &j);
                changed |= jacobi_pair(At, m, Vt, n, i, j);
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) sd += At[i * m + k] * At[i * m + k];
        W[i] = sqrt(sd);
    }
    for (int i = 0; i < n; i++) {
        int rank = 0;
        for (int j = 0; j < n; j++) rank += (W[j] > W[i]) || (W[j] == W[i] && j < i);
        perm[rank] = i;
    }
}

void dlt_rows(const double* nrm, float Mx, float My, float mx, float my, double* Lx, double* Ly) {
    const double x = (mx - nrm[0]) * nrm[4], y = (my - nrm[1]) * nrm[5];
    const double X = (Mx - nrm[2]) * nrm[6], Y = (My - nrm[3]) * nrm[7];
    const double lx[9] = {X, Y, 1, 0, 0, 0, -x * X, -x * Y, -x};
    const double ly[9] = {0, 0, 0, X, Y, 1, -y * X, -y * Y, -y};
    memcpy(Lx, lx, sizeof(lx));
    memcpy(Ly, ly, sizeof(ly));
}

bool scales_ok(double* nrm, int count) {
    if (fabs(nrm[4]) < DBL_EPSILON || fabs(nrm[5]) < DBL_EPSILON || fabs(nrm[6]) < DBL_EPSILON || fabs(nrm[7]) < DBL_EPSILON)
        return false;
    for (int k = 4; k < 8; k++) nrm[k] = count / nrm[k];
    return true;
}

// ltl: 45 upper-triangle sums -> H
void dlt_finish(const double* ltl, const double* nrm, double* H) {
    double At[100], Vt[100], W[10];
    int perm[10];
    for (int r = 0; r < 10; r++)
        for (int c = 0; c < 10; c++) {
            double v = 0;
            if (r < 9 && c < 9) {
                const int j = std::min(r, c), k = std::max(r, c);
                v = ltl[j * 9 - j * (j - 1) / 2 + (k - j)];
            }
            At[10 * r + c] = v;
        }
    jacobi_rr(At, 10, 10, Vt, W, perm);
    const double* v = Vt + 10 * perm[8];
    const double invHnorm[9] = {1. / nrm[4], 0, nrm[0], 0, 1. / nrm[5], nrm[1], 0, 0, 1};
    const double Hnorm2[9] = {nrm[6], 0, -nrm[2] * nrm[6], 0, nrm[7], -nrm[3] * nrm[7], 0, 0, 1};
    double T[9], H0[9];
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
    for (int k = 0; k < 9; k++) H[k] = H0[k] * sc;
}

// runKernel on 4 matches in subset order
bool run_kernel4(const float* src, const float* dst, const int32_t* idx, double* H) {
    double nrm[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
        const int q = idx[i];
        nrm[0] += dst[2 * q];
        nrm[1] += dst[2 * q + 1];
        nrm[2] += src[2 * q];
        nrm[3] += src[2 * q + 1];
    }
    for (int k = 0; k < 4; k++) nrm[k] /= 4;
    for (int i = 0; i < 4; i++) {
        const int q = idx[i];
        nrm[4] += fabs(dst[2 * q] - nrm[0]);
        nrm[5] += fabs(dst[2 * q + 1] - nrm[1]);
        nrm[6] += fabs(src[2 * q] - nrm[2]);
        nrm[7] += fabs(src[2 * q + 1] - nrm[3]);
    }
    if (!scales_ok(nrm, 4)) return false;
    double ltl[45] = {0};
    for (int i = 0; i < 4; i++) {
        const int q = idx[i];
        double Lx[9], Ly[9];
        dlt_rows(nrm, src[2 * q], src[2 * q + 1], dst[2 * q], dst[2 * q + 1], Lx, Ly);
        int e = 0;
        for (int j = 0; j < 9; j++)
            for (int k = j; k < 9; k++, e++) ltl[e] += Lx[j] * Lx[k] + Ly[j] * Ly[k];
    }
    dlt_finish(ltl, nrm, H);
    return true;
}

// block-ordered sums: part[l][e], lane l = i % 64, then the lanes in order
struct Blocks {
    int ne;
    std::vector<double> part;
    explicit Blocks(int ne_) : ne(ne_), part((size_t)kLanes * ne_, 0.0) {}
    double* lane(int i) { return part.data() + (size_t)(i % kLanes) * ne; }
    double total(int e) const {
        double acc = 0;
        for (int l = 0; l < kLanes; l++) acc += part[(size_t)l * ne + e];
        return acc;
    }
};

bool dlt_inliers(const float* src, const float* dst, const uint8_t* mask, int n, double* H) {
    Blocks c(5);
    for (int i = 0; i < n; i++)
        if (mask[i]) {
            double* a = c.lane(i);
            a[0] += dst[2 * i];
            a[1] += dst[2 * i + 1];
            a[2] += src[2 * i];
            a[3] += src[2 * i + 1];
            a[4] += 1;
        }
    const int count = (int)c.total(4);
    if (count < 1) return false;
    double nrm[8];
    for (int k = 0; k < 4; k++) nrm[k] = c.total(k) / count;
    Blocks sc(4);
    for (int i = 0; i < n; i++)
        if (mask[i]) {
            double* a = sc.lane(i);
            a[0] += fabs(dst[2 * i] - nrm[0]);
            a[1] += fabs(dst[2 * i + 1] - nrm[1]);
            a[2] += fabs(src[2 * i] - nrm[2]);
            a[3] += fabs(src[2 * i + 1] - nrm[3]);
        }
    for (int k = 0; k < 4; k++) nrm[4 + k] = sc.total(k);
    if (!scales_ok(nrm, count)) return false;
    Blocks L(45);
    for (int i = 0; i < n; i++)
        if (mask[i]) {
            double* a = L.lane(i);
            double Lx[9], Ly[9];
            dlt_rows(nrm, src[2 * i], src[2 * i + 1], dst[2 * i], dst[2 * i + 1], Lx, Ly);
            int e = 0;
            for (int j = 0; j < 9; j++)
                for (int k = j; k < 9; k++, e++) a[e] += Lx[j] * Lx[k] + Ly[j] * Ly[k];
        }
    double ltl[45];
    for (int e = 0; e < 45; e++) ltl[e] = L.total(e);
    dlt_finish(ltl, nrm, H);
    return true;
}

float h_error(const float* Hf, float Mx, float My, float mx, float my) {
    const float ww = 1.f / (Hf[6] * Mx + Hf[7] * My + 1.f);
    const float dx = (Hf[0] * Mx + Hf[1] * My + Hf[2]) * ww - mx;
    const float dy = (Hf[3] * Mx + Hf[4] * My + Hf[5]) * ww - my;
    return dx * dx + dy * dy;
}

int find_inliers(const float* src, const float* dst, int n, const double* H, float thr2, uint8_t* mask) {
    float Hf[9];
    for (int k = 0; k < 9; k++) Hf[k] = (float)H[k];
    int good = 0;
    for (int i = 0; i < n; i++) {
        const bool in = h_error(Hf, src[2 * i], src[2 * i + 1], dst[2 * i], dst[2 * i + 1]) <= thr2;
        if (mask) mask[i] = in;
        good += in;
    }
    return good;
}

// HomographyRefineCallback::compute in the block order: S, max |r|, J^T J (36, upper), J^T r (8)
void lm_compute(const float* src, const float* dst, const uint8_t* mask, int n, const double* h, bool jac, double* S,
                double* rinf, double* JtJ, double* Jtr) {
    Blocks b(46);
    double mx = 0;
    for (int i = 0; i < n; i++)
        if (mask[i]) {
            double* a = b.lane(i);
            const float Mx = src[2 * i], My = src[2 * i + 1];
            double ww = h[6] * Mx + h[7] * My + 1.;
            ww = fabs(ww) > DBL_EPSILON ? 1. / ww : 0;
            const double xi = (h[0] * Mx + h[1] * My + h[2]) * ww;
            const double yi = (h[3] * Mx + h[4] * My + h[5]) * ww;
            const double ex = xi - dst[2 * i], ey = yi - dst[2 * i + 1];
            a[45] += ex * ex;
            a[45] += ey * ey;
            mx = std::max(mx, std::max(fabs(ex), fabs(ey)));
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
    *S = b.total(45);
    *rinf = mx;
    if (jac) {
        for (int e = 0; e < 36; e++) JtJ[e] = b.total(e);
        for (int j = 0; j < 8; j++) Jtr[j] = b.total(36 + j);
    }
}

void eig8(const double* A, double* w, double* E) {
    double At[64], Vt[64], W[8];
    int perm[8];
    memcpy(At, A, sizeof(At));
    jacobi_rr(At, 8, 8, Vt, W, perm);
    for (int i = 0; i < 8; i++) {
        w[i] = W[perm[i]];
        for (int k = 0; k < 8; k++) E[8 * i + k] = Vt[8 * perm[i] + k];
    }
}

double eig_thr(const double* w) {
    double thr = 0;
    for (int i = 0; i < 8; i++) thr += w[i];
    return thr * (DBL_EPSILON * 2);
}

void unpack8(const double* up, double* A) {
    int e = 0;
    for (int j = 0; j < 8; j++)
        for (int k = j; k < 8; k++, e++) A[8 * j + k] = A[8 * k + j] = up[e];
}

// LMSolverImpl::run, maxIters 10, eps FLT_EPSILON
int refine_lm(const float* src, const float* dst, const uint8_t* mask, int n, double* x) {
    double S, rinf, JtJu[36], v[8], A[64], D[8];
    lm_compute(src, dst, mask, n, x, true, &S, &rinf, JtJu, v);
    unpack8(JtJu, A);
    for (int i = 0; i < 8; i++) D[i] = A[9 * i];
    const double Rlo = 0.25, Rhi = 0.75;
    double lambda = 1, lc = 0.75;
    int iter = 0;
    for (;;) {
        double Ap[64], w[8], E[64], d[8] = {0}, xd[8];
        memcpy(Ap, A, sizeof(Ap));
        for (int i = 0; i < 8; i++) Ap[9 * i] += lambda * D[i];
        eig8(Ap, w, E);
        const double thr = eig_thr(w);
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
        lm_compute(src, dst, mask, n, xd, false, &Sd, &rdinf, nullptr, nullptr);
        double dS = 0;
        for (int i = 0; i < 8; i++) {
            double Ad = 0;
            for (int k = 0; k < 8; k++) Ad += A[8 * i + k] * d[k];
            dS += d[i] * (-Ad + 2 * v[i]);
        }
        const double R = (S - Sd) / (fabs(dS) > DBL_EPSILON ? dS : 1);
        if (R > Rhi) {
            lambda *= 0.5;
            if (lambda < lc) lambda = 0;
        } else if (R < Rlo) {
            double t = 0;
            for (int k = 0; k < 8; k++) t += d[k] * v[k];
            double nu = (Sd - S) / (fabs(t) > DBL_EPSILON ? t : 1) + 2;
            nu = std::min(std::max(nu, 2.), 10.);
            if (lambda == 0) {
                eig8(A, w, E);
                const double ithr = eig_thr(w);
                double maxval = DBL_EPSILON;
                for (int k = 0; k < 8; k++) {
                    double dk = 0;
                    for (int i = 0; i < 8; i++) {
                        if (fabs(w[i]) <= ithr) continue;
                        dk += E[8 * i + k] * (E[8 * i + k] * (1 / w[i]));
                    }
                    maxval = std::max(maxval, fabs(dk));
                }
                lambda = lc = 1. / maxval;
                nu *= 0.5;
            }
            lambda *= nu;
        }
        if (Sd < S) {
            memcpy(x, xd, sizeof(xd));
            lm_compute(src, dst, mask, n, x, true, &S, &rinf, JtJu, v);
            unpack8(JtJu, A);
        }
        iter++;
        double dinf = 0;
        for (int k = 0; k < 8; k++) dinf = std::max(dinf, fabs(d[k]));
        if (!(iter < 10 && dinf >= FLT_EPSILON && rinf >= FLT_EPSILON)) break;
    }
    return iter;
}

bool collinear(const float* p, const int32_t* idx) {
    const int i = 3;
    for (int j = 0; j < i; ++j) {
        const double dx1 = p[2 * idx[j]] - p[2 * idx[i]];
        const double dy1 = p[2 * idx[j] + 1] - p[2 * idx[i] + 1];
        for (int k = 0; k < j; ++k) {
            const double dx2 = p[2 * idx[k]] - p[2 * idx[i]];
            const double dy2 = p[2 * idx[k] + 1] - p[2 * idx[i] + 1];
            if (fabs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2))) return true;
        }
    }
    return false;
}

double det3(const float* p, int a, int b, int c) {
    const double m[9] = {p[2 * a], p[2 * a + 1], 1., p[2 * b], p[2 * b + 1], 1., p[2 * c], p[2 * c + 1], 1.};
    return m[0] * (m[4] * m[8] - m[7] * m[5]) - m[1] * (m[3] * m[8] - m[6] * m[5]) + m[2] * (m[3] * m[7] - m[6] * m[4]);
}

int rans_update(double p, double ep, int model_points, int max_iters) {
    p = std::min(std::max(p, 0.), 1.);
    ep = std::min(std::max(ep, 0.), 1.);
    double num = std::max(1. - p, DBL_MIN);
    double denom = 1. - std::pow(1. - ep, model_points);
    if (denom < DBL_MIN) return 0;
    num = std::log(num);
    denom = std::log(denom);
    return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)std::lrint(num / denom);
}

}  // namespace

extern "C" {

int hr_check_subset(const float* src, const float* dst, const int32_t* idx) {
    if (collinear(src, idx) || collinear(dst, idx)) return 0;
    static const int tt[4][3] = {{0, 1, 2}, {1, 2, 3}, {0, 2, 3}, {0, 1, 3}};
    int negative = 0;
    for (int i = 0; i < 4; ++i)
        negative += det3(src, idx[tt[i][0]], idx[tt[i][1]], idx[tt[i][2]]) * det3(dst, idx[tt[i][0]], idx[tt[i][1]], idx[tt[i][2]]) < 0;
    return negative == 0 || negative == 4;
}

// subsets (max_iters x 4) as getSubset draws them; returns how many were drawn before it gave up
int hr_subsets(const float* src, const float* dst, int n, int max_iters, int32_t* out) {
    CvRng rng(~0ULL);
    for (int it = 0; it < max_iters; ++it) {
        int32_t* s = out + 4 * it;
        bool found = false;
        for (int attempt = 0; attempt < 1000 && !found; ++attempt) {
            for (int i = 0; i < 4; ++i) {
                int v;
                do {
                    v = rng.uniform(0, n);
                } while (std::find(s, s + i, v) != s + i);
                s[i] = v;
            }
            found = hr_check_subset(src, dst, s);
        }
        if (!found) return it;
    }
    return max_iters;
}

int hr_run_kernel4(const float* src, const float* dst, const int32_t* idx, double* H) { return run_kernel4(src, dst, idx, H); }

int hr_dlt_inliers(const float* src, const float* dst, const uint8_t* mask, int n, double* H) {
    return dlt_inliers(src, dst, mask, n, H);
}

int hr_refine_lm(const float* src, const float* dst, const uint8_t* mask, int n, double* x) {
    return refine_lm(src, dst, mask, n, x);
}

// findHomography(src, dst, RANSAC, thr, noArray(), 2000, conf).  counts: every hypothesis the sequential loop ran
// (-1: no model); info = {selected iteration, iterations run, 0, subsets drawn, LM iterations, DLT re-fit used}.
// Returns 1 when a model was found.
int hr_find_homography(const float* src, const float* dst, int n, double thr, double conf, double* H, uint8_t* mask,
                       int32_t* counts, int32_t* info) {
    for (int k = 0; k < 6; k++) info[k] = 0;
    info[0] = -1;
    for (int k = 0; k < 9; k++) H[k] = 0;
    if (n < 4) return 0;
    if (thr <= 0) thr = 3;
    const float thr2 = (float)(thr * thr);
    if (n == 4) {
        const int32_t idx[4] = {0, 1, 2, 3};
        info[3] = 1;
        info[1] = 1;
        counts[0] = -1;
        if (!run_kernel4(src, dst, idx, H)) return 0;
        counts[0] = find_inliers(src, dst, n, H, thr2, nullptr);
        info[0] = 0;
        for (int i = 0; i < 4; i++) mask[i] = 1;
        return 1;
    }
    std::vector<int32_t> sub((size_t)2000 * 4);
    const int total = hr_subsets(src, dst, n, 2000, sub.data());
    info[3] = total;
    if (total == 0) return 0;
    int niters = 2000, max_good = 0, best = -1, it = 0;
    double bestH[9] = {0};
    for (; it < niters; it++) {
        if (it >= total) break;
        double Hh[9];
        if (!run_kernel4(src, dst, sub.data() + 4 * it, Hh)) {
            counts[it] = -1;
            continue;
        }
        const int good = find_inliers(src, dst, n, Hh, thr2, nullptr);
        counts[it] = good;
        if (good > std::max(max_good, 3)) {
            max_good = good;
            best = it;
            memcpy(bestH, Hh, sizeof(bestH));
            niters = rans_update(conf, (double)(n - good) / n, 4, niters);
        }
    }
    info[1] = it;
    if (best < 0) return 0;
    info[0] = best;
    find_inliers(src, dst, n, bestH, thr2, mask);
    double Hn[9];
    memcpy(H, bestH, sizeof(bestH));
    if (dlt_inliers(src, dst, mask, n, Hn)) {
        memcpy(H, Hn, sizeof(Hn));
        info[5] = 1;
    }
    info[4] = refine_lm(src, dst, mask, n, H);
    return 1;
}

}  // extern "C"
