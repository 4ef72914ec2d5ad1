// tests/init_pose_restatement.cpp -- TEST INFRASTRUCTURE: the homography branch of the monocular initialisation after
// its RANSAC (estiMotionByHomography: decomposeHomographyMat, t / |t|; removeWrongRtOfHomography) and the rest of
// helperEstimatePossibleRelativePosesByEpipolarGeometry (the choice, invRt), restated sequentially in the arithmetic
// csrc/hd_wave.h declares (compiled by tests/pose_restate.py with g++ -ffp-contract=off).  The RANSACs, the E branch,
// the triangulation and the scores come from the existing restatements and the CPU oracle.
//   normalisation  Hn = (K^-1 H) K with the closed-form 3 x 3 inverse; Hn * (1.0 / w[1]), w from the oracle's svd3
//   decomposition  HomographyDecompInria in OpenCV's order of operations, v with a float sqrt
//   filter         every H inlier tested against every candidate; a candidate survives when no inlier rejects it
//   choice         ratio = score_h / (score_e + score_h); ratio > 0.5: the H slot with the strictly largest |n_z|
//   invRt          [R t; 0 1] inverted by the oracle's partial-pivoting LU
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../oracle/linalg_oracle.h"

namespace {

double det3(const double* m) {
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// Matx33d * Matx33d: s = a(i,0) b(0,j), then + a(i,1) b(1,j), then + a(i,2) b(2,j)
void mul3(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double v = A[3 * i] * B[j];
            v = v + A[3 * i + 1] * B[3 + j];
            C[3 * i + j] = v + A[3 * i + 2] * B[6 + j];
        }
}

void mulv(const double* A, const double* x, double* y) {
    for (int i = 0; i < 3; i++) {
        double v = A[3 * i] * x[0];
        v = v + A[3 * i + 1] * x[1];
        y[i] = v + A[3 * i + 2] * x[2];
    }
}

// Matx33d::inv: adjugate times 1 / det, zeros when det == 0
void invert3(const double* M, double* out) {
    auto m = [&](int r, int c) { return M[3 * r + c]; };
    double d = det3(M);
    if (d == 0.) {
        for (int k = 0; k < 9; k++) out[k] = 0;
        return;
    }
    d = 1. / d;
    out[0] = (m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1)) * d;
    out[1] = (m(0, 2) * m(2, 1) - m(0, 1) * m(2, 2)) * d;
    out[2] = (m(0, 1) * m(1, 2) - m(0, 2) * m(1, 1)) * d;
    out[3] = (m(1, 2) * m(2, 0) - m(1, 0) * m(2, 2)) * d;
    out[4] = (m(0, 0) * m(2, 2) - m(0, 2) * m(2, 0)) * d;
    out[5] = (m(0, 2) * m(1, 0) - m(0, 0) * m(1, 2)) * d;
    out[6] = (m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0)) * d;
    out[7] = (m(0, 1) * m(2, 0) - m(0, 0) * m(2, 1)) * d;
    out[8] = (m(0, 0) * m(1, 1) - m(0, 1) * m(1, 0)) * d;
}

int signd(double x) { return x >= 0 ? 1 : -1; }

double opposite_of_minor(const double* M, int row, int col) {
    const int x1 = col == 0 ? 1 : 0, x2 = col == 2 ? 1 : 2;
    const int y1 = row == 0 ? 1 : 0, y2 = row == 2 ? 1 : 2;
    return M[3 * y1 + x2] * M[3 * y2 + x1] - M[3 * y1 + x1] * M[3 * y2 + x2];
}

double norm3(const double* v) {
    double s = v[0] * v[0] + v[1] * v[1];
    s = s + v[2] * v[2];
    return sqrt(s);
}

// findRmatFrom_tstar_n: R = Hn (I - ((2 / v) t*) n^T), negated when det(R) < 0
void rmat_from_tstar_n(const double* Hn, const double* ts, const double* n, double v, double* R) {
    double M[9];
    const double c = 2 / v;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) M[3 * i + j] = (i == j ? 1.0 : 0.0) - (ts[i] * c) * n[j];
    mul3(Hn, M, R);
    if (det3(R) < 0)
        for (int k = 0; k < 9; k++) R[k] = -R[k];
}

}  // namespace

extern "C" {

// decomposeHomographyMat(Hs, K).  Outputs Hn (after 1 / w[1]), w, branch = {rotation-only, index of the largest
// |S_ii| or -1}, the raw candidates Rs (4 x 9), ts (4 x 3), ns (4 x 3; unused rows zero).  Returns the count (1 or 4).
int pr_decompose(const double* Hs, const double* K4, double* Hn_out, double* w, int32_t* branch, double* Rs, double* ts,
                 double* ns) {
    const double K[9] = {K4[0], 0, K4[2], 0, K4[1], K4[3], 0, 0, 1};
    double Ki[9], T[9], Hn[9], U[9], V[9];
    invert3(K, Ki);
    mul3(Ki, Hs, T);
    mul3(T, K, Hn);
    orc_linalg::svd3(Hn, U, w, V);
    const double a = 1.0 / w[1];
    for (int k = 0; k < 9; k++) Hn[k] = Hn[k] * a;
    std::memcpy(Hn_out, Hn, sizeof(Hn));
    for (int k = 0; k < 36; k++) Rs[k] = 0;
    for (int k = 0; k < 12; k++) ts[k] = ns[k] = 0;
    double HnT[9], S[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) HnT[3 * i + j] = Hn[3 * j + i];
    mul3(HnT, Hn, S);
    S[0] -= 1.0;
    S[4] -= 1.0;
    S[8] -= 1.0;
    double norm_inf = 0;  // cv::norm(NORM_INF): s = std::max(s, |S_ij|)
    for (int k = 0; k < 9; k++) norm_inf = norm_inf < std::fabs(S[k]) ? std::fabs(S[k]) : norm_inf;
    if (norm_inf < 0.001) {
        std::memcpy(Rs, Hn, sizeof(Hn));
        branch[0] = 1;
        branch[1] = -1;
        return 1;
    }
    auto s = [&](int r, int c) { return S[3 * r + c]; };
    const double M00 = opposite_of_minor(S, 0, 0), M11 = opposite_of_minor(S, 1, 1), M22 = opposite_of_minor(S, 2, 2);
    const double rtM00 = sqrt(M00), rtM11 = sqrt(M11), rtM22 = sqrt(M22);
    const double M01 = opposite_of_minor(S, 0, 1), M12 = opposite_of_minor(S, 1, 2), M02 = opposite_of_minor(S, 0, 2);
    const int e12 = signd(M12), e02 = signd(M02), e01 = signd(M01);
    const double nS00 = std::fabs(s(0, 0)), nS11 = std::fabs(s(1, 1)), nS22 = std::fabs(s(2, 2));
    int indx = 0;
    if (nS00 < nS11) {
        indx = 1;
        if (nS11 < nS22) indx = 2;
    } else {
        if (nS00 < nS22) indx = 2;
    }
    double npa[3], npb[3];
    switch (indx) {
        case 0:
            npa[0] = s(0, 0), npb[0] = s(0, 0);
            npa[1] = s(0, 1) + rtM22, npb[1] = s(0, 1) - rtM22;
            npa[2] = s(0, 2) + e12 * rtM11, npb[2] = s(0, 2) - e12 * rtM11;
            break;
        case 1:
            npa[0] = s(0, 1) + rtM22, npb[0] = s(0, 1) - rtM22;
            npa[1] = s(1, 1), npb[1] = s(1, 1);
            npa[2] = s(1, 2) - e02 * rtM00, npb[2] = s(1, 2) + e02 * rtM00;
            break;
        default:
            npa[0] = s(0, 2) + e01 * rtM11, npb[0] = s(0, 2) - e01 * rtM11;
            npa[1] = s(1, 2) + rtM00, npb[1] = s(1, 2) - rtM00;
            npa[2] = s(2, 2), npb[2] = s(2, 2);
            break;
    }
    const double traceS = s(0, 0) + s(1, 1) + s(2, 2);
    const double v = 2.0 * sqrtf((float)(1 + traceS - M00 - M11 - M22));
    const double ESii = signd(s(indx, indx));
    const double r_2 = 2 + traceS + v, nt_2 = 2 + traceS - v;
    const double r = sqrt(r_2), n_t = sqrt(nt_2);
    double na[3], nb[3];
    const double ia = 1.0 / norm3(npa), ib = 1.0 / norm3(npb);
    for (int k = 0; k < 3; k++) {
        na[k] = npa[k] * ia;
        nb[k] = npb[k] * ib;
    }
    const double half_nt = 0.5 * n_t, esii_t_r = ESii * r;
    double ta_star[3], tb_star[3];
    for (int k = 0; k < 3; k++) {
        ta_star[k] = (esii_t_r * nb[k] - n_t * na[k]) * half_nt;
        tb_star[k] = (esii_t_r * na[k] - n_t * nb[k]) * half_nt;
    }
    double Ra[9], Rb[9], ta[3], tb[3];
    rmat_from_tstar_n(Hn, ta_star, na, v, Ra);
    mulv(Ra, ta_star, ta);
    rmat_from_tstar_n(Hn, tb_star, nb, v, Rb);
    mulv(Rb, tb_star, tb);
    const double* Rc[4] = {Ra, Ra, Rb, Rb};
    for (int c = 0; c < 4; c++) {
        std::memcpy(Rs + 9 * c, Rc[c], 9 * sizeof(double));
        for (int k = 0; k < 3; k++) {
            const double* tc = c < 2 ? ta : tb;
            const double* nc = c < 2 ? na : nb;
            ts[3 * c + k] = (c & 1) ? -tc[k] : tc[k];
            ns[3 * c + k] = (c & 1) ? -nc[k] : nc[k];
        }
    }
    branch[0] = 0;
    branch[1] = indx;
    return 4;
}

// t * (1.0 / sqrt((t1^2 + t2^2) + t0^2))
void pr_normalise_t(const double* t, double* out) {
    double s = t[1] * t[1] + t[2] * t[2];
    s = s + t[0] * t[0];
    const double a = 1.0 / sqrt(s);
    for (int k = 0; k < 3; k++) out[k] = t[k] * a;
}

// filterHomographyDecompByVisibleRefpoints over the listed matches (pixels, normalised by pixel2CamNormPlane and
// rounded to float): rejected[c] = how many listed matches see candidate c's plane behind a camera.
void pr_filter(const float* kp1, const float* kp2, const int32_t* list, int m, const double* K4, const double* Rs,
               const double* ns, int count, int32_t* rejected) {
    for (int c = 0; c < 4; c++) rejected[c] = 0;
    for (int c = 0; c < count; c++) {
        const double* R = Rs + 9 * c;
        const double* n = ns + 3 * c;
        double Rn[3];
        mulv(R, n, Rn);
        for (int j = 0; j < m; j++) {
            const int i = list[j];
            const double prev[3] = {(float)((kp1[2 * i] - K4[2]) / K4[0]), (float)((kp1[2 * i + 1] - K4[3]) / K4[1]), 1.0};
            const double curr[3] = {(float)((kp2[2 * i] - K4[2]) / K4[0]), (float)((kp2[2 * i + 1] - K4[3]) / K4[1]), 1.0};
            double d1 = 0, d2 = 0;  // Vec3d::dot
            for (int k = 0; k < 3; k++) d1 += prev[k] * n[k];
            for (int k = 0; k < 3; k++) d2 += curr[k] * Rn[k];
            if (d1 <= 0 || d2 <= 0) rejected[c]++;
        }
    }
}

// the choice of motion_estimation.cpp:139-155 over the table: nz[s] = |normal_z| of H slot s (1..k); -1 when the rule
// picks a slot that does not exist
int pr_choose(double score_e, double score_h, int has_e, const double* nz, int k, double* ratio) {
    *ratio = score_h / (score_e + score_h);
    if (*ratio > 0.5) {
        if (k < 1) return -1;
        int best = 1;
        double largest = nz[1];
        for (int i = 2; i <= k; i++)
            if (nz[i] > largest) {
                largest = nz[i];
                best = i;
            }
        return best;
    }
    return has_e ? 0 : -1;
}

// basics::invRt
void pr_inv_rt(double* R, double* t) {
    const double T[16] = {R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2], 0, 0, 0, 1};
    double Ti[16];
    if (!orc_linalg::invert4x4_lu(T, Ti))
        for (int k = 0; k < 16; k++) Ti[k] = 0;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R[3 * i + j] = Ti[4 * i + j];
        t[i] = Ti[4 * i + 3];
    }
}
}
