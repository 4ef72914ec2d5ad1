// csrc/hd_wave.h -- the homography branch of the monocular initialisation after its RANSAC (track_kernels.hip:
// k_h_decompose, k_init_triangulate).  Reference: estiMotionByHomography + removeWrongRtOfHomography
// (src/geometry/epipolar_geometry.cpp:59-128), called by helperEstimatePossibleRelativePosesByEpipolarGeometry
// (src/geometry/motion_estimation.cpp:10-157).
//
// decomposeHomographyMat(H, K) is OpenCV's HomographyDecompInria (Malis & Vargas).  Uniform code: every lane that
// needs the decomposition computes it.  Declared arithmetic:
//   scaling        H /= H(2,2) and t /= |t| are cv::Mat::convertTo with alpha = 1 / s: every entry times (1.0 / s);
//                  |t| = sqrt((t1^2 + t2^2) + t0^2) in the reference's order
//   normalisation  Hn = (K^-1 H) K, K^-1 by the 3 x 3 closed form of Matx33d::inv (zeros when det == 0), every
//                  product entry summed k = 0..2 in order; Hn *= 1.0 / w[1], w the singular values of svd3
//                  (the canonical Jacobi) in descending order
//   S              Hn^T Hn - I; rotation-only when max |S_ij| < 0.001 (NaN entries never raise the maximum)
//   general        oppositeOfMinor, signd(x) = x >= 0 ? 1 : -1, the index of the largest |S_ii| by OpenCV's
//                  comparison chain, npa / npb, v = 2 sqrtf(((1 + tr S) - M00 - M11) - M22) (OpenCV takes a FLOAT
//                  sqrt here), r = sqrt((2 + tr S) + v), n_t = sqrt((2 + tr S) - v), n = np * (1.0 / |np|) with
//                  |np| = sqrt((np0^2 + np1^2) + np2^2), t* = half_nt * (esii_t_r * n' - n_t * n)
//   R              Hn (I - ((2 / v) t*) n^T), negated when cv::determinant(R) < 0 (cofactor expansion along row 0);
//                  t = R t*; the four motions (Ra, ta, na), (Ra, -ta, -na), (Rb, tb, nb), (Rb, -tb, -nb)
//   visibility     filterHomographyDecompByVisibleRefpoints on pixel2CamNormPlane rounded to float: a candidate is
//                  rejected by a match when (x1 n0 + y1 n1) + n2 <= 0 or (x2 m0 + y2 m1) + m2 <= 0, m = R n
#ifndef MVO_HD_WAVE_H
#define MVO_HD_WAVE_H
#include "em_wave.h"

namespace pw {

// the layouts of k_h_decompose's outputs (kHd*) are in mvo_internal.h

struct HDecomp {
    double Hn[9], w[3];
    double R[4][9], t[4][3], n[4][3];
    int count, branch;
};

PW_FN void hd_invert3(const double (&m)[3][3], double (&out)[3][3]) {
    double d = rp_det3(m);
    if (d == 0.) {
        PW_UNROLL
        for (int k = 0; k < 9; k++) out[k / 3][k % 3] = 0;
        return;
    }
    d = 1. / d;
    out[0][0] = (m[1][1] * m[2][2] - m[1][2] * m[2][1]) * d;
    out[0][1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) * d;
    out[0][2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) * d;
    out[1][0] = (m[1][2] * m[2][0] - m[1][0] * m[2][2]) * d;
    out[1][1] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) * d;
    out[1][2] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) * d;
    out[2][0] = (m[1][0] * m[2][1] - m[1][1] * m[2][0]) * d;
    out[2][1] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) * d;
    out[2][2] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) * d;
}

PW_FN double hd_signd(double x) { return x >= 0 ? 1 : -1; }

// HomographyDecompInria::oppositeOfMinor
PW_FN double hd_minor(const double (&M)[3][3], int row, int col) {
    const int x1 = col == 0 ? 1 : 0, x2 = col == 2 ? 1 : 2;
    const int y1 = row == 0 ? 1 : 0, y2 = row == 2 ? 1 : 2;
    return M[y1][x2] * M[y2][x1] - M[y1][x1] * M[y2][x2];
}

// v = (x, y, z) * (1.0 / |v|)
PW_FN void hd_unit(const double (&v)[3], double (&out)[3]) {
    double s = v[0] * v[0] + v[1] * v[1];
    s = s + v[2] * v[2];
    const double a = 1.0 / sqrt(s);
    PW_UNROLL
    for (int k = 0; k < 3; k++) out[k] = v[k] * a;
}

// findRmatFrom_tstar_n, then t = R t*
PW_FN void hd_rt(const double (&Hn)[3][3], const double (&ts)[3], const double (&n)[3], double v, double (&R)[9],
                 double (&t)[3]) {
    const double c = 2 / v;
    double M[3][3], Rm[3][3];
    PW_UNROLL
    for (int i = 0; i < 3; i++) {
        PW_UNROLL
        for (int j = 0; j < 3; j++) M[i][j] = (i == j ? 1.0 : 0.0) - (ts[i] * c) * n[j];
    }
    rp_mul3(Hn, M, Rm);
    if (rp_det3(Rm) < 0) {
        PW_UNROLL
        for (int k = 0; k < 9; k++) Rm[k / 3][k % 3] = -Rm[k / 3][k % 3];
    }
    PW_UNROLL
    for (int k = 0; k < 9; k++) R[k] = Rm[k / 3][k % 3];
    PW_UNROLL
    for (int r = 0; r < 3; r++) {
        double s = Rm[r][0] * ts[0];
        s = s + Rm[r][1] * ts[1];
        t[r] = s + Rm[r][2] * ts[2];
    }
}

// decomposeHomographyMat(Hs, K) for the scaled H (Hs, row-major) and K = [fx 0 cx; 0 fy cy; 0 0 1]
PW_FN void hd_decompose(const double (&Hs)[9], double fx, double fy, double cx, double cy, HDecomp& d) {
    const double K[3][3] = {{fx, 0, cx}, {0, fy, cy}, {0, 0, 1}};
    double Ki[3][3], H[3][3], T[3][3], Hn[3][3];
    hd_invert3(K, Ki);
    PW_UNROLL
    for (int k = 0; k < 9; k++) H[k / 3][k % 3] = Hs[k];
    rp_mul3(Ki, H, T);
    rp_mul3(T, K, Hn);
    double U[3][3], V[3][3];
    svd3(Hn, U, d.w, V);
    const double a = 1.0 / d.w[1];
    PW_UNROLL
    for (int k = 0; k < 9; k++) Hn[k / 3][k % 3] = Hn[k / 3][k % 3] * a;
    PW_UNROLL
    for (int k = 0; k < 9; k++) d.Hn[k] = Hn[k / 3][k % 3];
    double HnT[3][3], S[3][3];
    PW_UNROLL
    for (int k = 0; k < 9; k++) HnT[k / 3][k % 3] = Hn[k % 3][k / 3];
    rp_mul3(HnT, Hn, S);
    S[0][0] -= 1.0;
    S[1][1] -= 1.0;
    S[2][2] -= 1.0;
    double mx = 0;
    PW_UNROLL
    for (int k = 0; k < 9; k++) {
        const double e = fabs(S[k / 3][k % 3]);
        mx = mx < e ? e : mx;
    }
    PW_UNROLL
    for (int c = 0; c < 4; c++) {
        PW_UNROLL
        for (int k = 0; k < 9; k++) d.R[c][k] = 0;
        PW_UNROLL
        for (int k = 0; k < 3; k++) d.t[c][k] = d.n[c][k] = 0;
    }
    if (mx < 0.001) {
        PW_UNROLL
        for (int k = 0; k < 9; k++) d.R[0][k] = d.Hn[k];
        d.count = 1;
        d.branch = -1;
        return;
    }
    const double M00 = hd_minor(S, 0, 0), M11 = hd_minor(S, 1, 1), M22 = hd_minor(S, 2, 2);
    const double rtM00 = sqrt(M00), rtM11 = sqrt(M11), rtM22 = sqrt(M22);
    const double M01 = hd_minor(S, 0, 1), M12 = hd_minor(S, 1, 2), M02 = hd_minor(S, 0, 2);
    const double e12 = hd_signd(M12), e02 = hd_signd(M02), e01 = hd_signd(M01);
    const double nS00 = fabs(S[0][0]), nS11 = fabs(S[1][1]), nS22 = fabs(S[2][2]);
    int indx = 0;
    if (nS00 < nS11) {
        indx = 1;
        if (nS11 < nS22) indx = 2;
    } else {
        if (nS00 < nS22) indx = 2;
    }
    double npa[3], npb[3];
    if (indx == 0) {
        npa[0] = S[0][0], npb[0] = S[0][0];
        npa[1] = S[0][1] + rtM22, npb[1] = S[0][1] - rtM22;
        npa[2] = S[0][2] + e12 * rtM11, npb[2] = S[0][2] - e12 * rtM11;
    } else if (indx == 1) {
        npa[0] = S[0][1] + rtM22, npb[0] = S[0][1] - rtM22;
        npa[1] = S[1][1], npb[1] = S[1][1];
        npa[2] = S[1][2] - e02 * rtM00, npb[2] = S[1][2] + e02 * rtM00;
    } else {
        npa[0] = S[0][2] + e01 * rtM11, npb[0] = S[0][2] - e01 * rtM11;
        npa[1] = S[1][2] + rtM00, npb[1] = S[1][2] - rtM00;
        npa[2] = S[2][2], npb[2] = S[2][2];
    }
    const double traceS = (S[0][0] + S[1][1]) + S[2][2];
    const double v = 2.0 * (double)sqrtf((float)(1 + traceS - M00 - M11 - M22));
    const double ESii = hd_signd(indx == 0 ? S[0][0] : indx == 1 ? S[1][1] : S[2][2]);
    const double r = sqrt((2 + traceS) + v), n_t = sqrt((2 + traceS) - v);
    double na[3], nb[3];
    hd_unit(npa, na);
    hd_unit(npb, nb);
    const double half_nt = 0.5 * n_t, esii_t_r = ESii * r;
    double ta_star[3], tb_star[3];
    PW_UNROLL
    for (int k = 0; k < 3; k++) {
        ta_star[k] = half_nt * (esii_t_r * nb[k] - n_t * na[k]);
        tb_star[k] = half_nt * (esii_t_r * na[k] - n_t * nb[k]);
    }
    hd_rt(Hn, ta_star, na, v, d.R[0], d.t[0]);
    hd_rt(Hn, tb_star, nb, v, d.R[2], d.t[2]);
    PW_UNROLL
    for (int k = 0; k < 9; k++) {
        d.R[1][k] = d.R[0][k];
        d.R[3][k] = d.R[2][k];
    }
    PW_UNROLL
    for (int k = 0; k < 3; k++) {
        d.n[0][k] = na[k];
        d.n[2][k] = nb[k];
        d.t[1][k] = -d.t[0][k];
        d.n[1][k] = -na[k];
        d.t[3][k] = -d.t[2][k];
        d.n[3][k] = -nb[k];
    }
    d.count = 4;
    d.branch = indx;
}

// t / sqrt((t1^2 + t2^2) + t0^2) as estiMotionByHomography normalises it (epipolar_geometry.cpp:120-125); a zero t
// gives NaN (0 * inf), as in the reference
PW_FN void hd_normalise_t(const double (&t)[3], double (&out)[3]) {
    double s = t[1] * t[1] + t[2] * t[2];
    s = s + t[0] * t[0];
    const double a = 1.0 / sqrt(s);
    PW_UNROLL
    for (int k = 0; k < 3; k++) out[k] = t[k] * a;
}

// filterHomographyDecompByVisibleRefpoints for one match (x1, y1), (x2, y2) on the normalised plane: true when the
// match rejects candidate (R, n)
PW_FN bool hd_rejects(double x1, double y1, double x2, double y2, const double (&R)[9], const double (&n)[3]) {
    double d1 = x1 * n[0] + y1 * n[1];
    d1 = d1 + 1.0 * n[2];
    double m[3];
    PW_UNROLL
    for (int r = 0; r < 3; r++) {
        double s = R[3 * r] * n[0];
        s = s + R[3 * r + 1] * n[1];
        m[r] = s + R[3 * r + 2] * n[2];
    }
    double d2 = x2 * m[0] + y2 * m[1];
    d2 = d2 + 1.0 * m[2];
    return d1 <= 0 || d2 <= 0;
}

}  // namespace pw
#endif
