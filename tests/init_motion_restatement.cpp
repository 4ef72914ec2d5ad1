// tests/init_motion_restatement.cpp -- TEST INFRASTRUCTURE: the essential-matrix branch of the monocular
// initialisation after its RANSAC (estiMotionByEssential: E /= E(2,2), recoverPose, t / |t|) and the two ORB-SLAM
// model scores (checkEssentialScore, checkHomographyScore), restated sequentially in the arithmetic csrc/em_wave.h
// declares (compiled by tests/init_restate.py with g++ -ffp-contract=off).  The RANSAC itself and its selected E come
// from the CPU oracle; the SVDs are its one-sided Jacobi (cyclic pairs for 3 x 3 and 4 x 4, as svd_small).
//   scaling        every entry times (1.0 / s)  (cv::Mat::convertTo with alpha = 1 / s)
//   decomposition  U, Vt of the scaled E, negated when det < 0; R1 = (U W) Vt, R2 = (U W^T) Vt, t = U.col(2)
//   cheirality     cvTriangulatePoints' 4 x 4 system, the last row of Vt kept in double, recoverPose's tests in order
//   scores         lane l of one wave takes list positions l, l + 64, ... from 0.0, term 1 before term 2; the 64
//                  partials are added in lane order
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../oracle/linalg_oracle.h"

namespace {

constexpr int kLanes = 64;
constexpr double kDist = 50.0;

double det3(const double* m) {
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

void mul3(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double v = A[3 * i] * B[j];
            v = v + A[3 * i + 1] * B[3 + j];
            C[3 * i + j] = v + A[3 * i + 2] * B[6 + j];
        }
}

// cv::invert(DECOMP_LU) for 3 x 3: adjugate / det3, zeros when det3 == 0
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

// decomposeEssentialMat: D = R1 (9), R2 (9), t (3)
void decompose(const double* E, double* D) {
    double U[9], W[3], V[9], Vt[9];
    orc_linalg::svd3(E, U, W, V);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Vt[3 * i + j] = V[3 * j + i];
    if (det3(U) < 0)
        for (int k = 0; k < 9; k++) U[k] = -U[k];
    if (det3(Vt) < 0)
        for (int k = 0; k < 9; k++) Vt[k] = -Vt[k];
    const double Wm[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1}, Wmt[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};
    double T[9];
    mul3(U, Wm, T);
    mul3(T, Vt, D);
    mul3(U, Wmt, T);
    mul3(T, Vt, D + 9);
    for (int r = 0; r < 3; r++) D[18 + r] = U[3 * r + 2];
}

bool cheirality(double x1, double y1, double x2, double y2, const double* P) {
    const double P0[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const double* Ps[2] = {P0, P};
    const double pt[2][2] = {{x1, y1}, {x2, y2}};
    double A[16];
    for (int j = 0; j < 2; j++)
        for (int k = 0; k < 4; k++) {
            A[(2 * j) * 4 + k] = pt[j][0] * Ps[j][8 + k] - Ps[j][k];
            A[(2 * j + 1) * 4 + k] = pt[j][1] * Ps[j][8 + k] - Ps[j][4 + k];
        }
    double At[16], Vt[16], W[4];
    for (int i = 0; i < 4; i++)
        for (int k = 0; k < 4; k++) At[i * 4 + k] = A[k * 4 + i];
    orc_linalg::jacobi_svd(At, 4, 4, Vt, W);
    double Q[4] = {Vt[12], Vt[13], Vt[14], Vt[15]};
    bool ok = Q[2] * Q[3] > 0;  // mask1 = Q.row(2).mul(Q.row(3)) > 0
    const double w = Q[3];
    for (int k = 0; k < 4; k++) Q[k] = Q[k] / w;  // Q.row(k) /= Q.row(3), k = 0..3 in order (row 3 last)
    ok = ok && Q[2] < kDist;
    double z = P[8] * Q[0] + P[9] * Q[1];  // (P Q)(2)
    z = z + P[10] * Q[2];
    z = z + P[11] * Q[3];
    ok = ok && z > 0;
    ok = ok && z < kDist;
    return ok;
}

}  // namespace

extern "C" {

// E_raw: findEssentialMat's selected candidate; mask: its RANSAC mask (NULL: every match).  Outputs the scaled E, R,
// the unit t, the four counts, the chosen combination, the decomposition and the per-match bits.
void ir_recover_pose(const float* kp1, const float* kp2, int n, const double* K4, const double* E_raw,
                     const uint8_t* mask, double* E, double* R, double* t, int32_t* good, int32_t* chosen,
                     double* R1R2t, uint8_t* masks) {
    const double focal = (K4[0] + K4[1]) / 2;
    const double pcx = (double)(float)K4[2], pcy = (double)(float)K4[3];
    const double a = 1.0 / E_raw[8];
    for (int k = 0; k < 9; k++) E[k] = E_raw[k] * a;
    decompose(E, R1R2t);
    for (int c = 0; c < 4; c++) good[c] = 0;
    for (int i = 0; i < n; i++) {
        const double x1 = ((double)kp1[2 * i] - pcx) / focal, y1 = ((double)kp1[2 * i + 1] - pcy) / focal;
        const double x2 = ((double)kp2[2 * i] - pcx) / focal, y2 = ((double)kp2[2 * i + 1] - pcy) / focal;
        uint8_t bits = 0;
        for (int c = 0; c < 4; c++) {
            const double* Rc = R1R2t + ((c & 1) ? 9 : 0);
            double P[12];
            for (int r = 0; r < 3; r++) {
                for (int k = 0; k < 3; k++) P[4 * r + k] = Rc[3 * r + k];
                P[4 * r + 3] = c < 2 ? R1R2t[18 + r] : -R1R2t[18 + r];
            }
            if (cheirality(x1, y1, x2, y2, P) && (!mask || mask[i])) {
                bits |= (uint8_t)(1u << c);
                good[c]++;
            }
        }
        masks[i] = bits;
    }
    int ch;
    if (good[0] >= good[1] && good[0] >= good[2] && good[0] >= good[3])
        ch = 0;
    else if (good[1] >= good[0] && good[1] >= good[2] && good[1] >= good[3])
        ch = 1;
    else if (good[2] >= good[0] && good[2] >= good[1] && good[2] >= good[3])
        ch = 2;
    else
        ch = 3;
    *chosen = ch;
    for (int k = 0; k < 9; k++) R[k] = R1R2t[((ch & 1) ? 9 : 0) + k];
    for (int r = 0; r < 3; r++) t[r] = ch < 2 ? R1R2t[18 + r] : -R1R2t[18 + r];
    double s = t[1] * t[1] + t[2] * t[2];
    s = s + t[0] * t[0];
    const double inv = 1.0 / sqrt(s);
    for (int r = 0; r < 3; r++) t[r] = t[r] * inv;
}

// checkEssentialScore / checkHomographyScore; E or H NULL: score 0, nothing kept
void ir_check_init_scores(const float* kp1, const float* kp2, const double* K4, const double* E, const int32_t* inl_e,
                          int n_e, const double* H, const int32_t* inl_h, int n_h, double sigma, double* score_e,
                          double* score_h, int32_t* kept_e, int32_t* n_kept_e, int32_t* kept_h, int32_t* n_kept_h) {
    const double inv_s2 = 1.0 / (sigma * sigma);
    double part[kLanes];
    *score_e = *score_h = 0;
    *n_kept_e = *n_kept_h = 0;
    if (E) {
        const double K[9] = {K4[0], 0, K4[2], 0, K4[1], K4[3], 0, 0, 1};
        double Ki[9], KiT[9], T[9], f[9];
        invert3(K, Ki);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) KiT[3 * i + j] = Ki[3 * j + i];
        mul3(KiT, E, T);
        mul3(T, Ki, f);
        const double th = 3.841, th_score = 5.991;
        for (int l = 0; l < kLanes; l++) part[l] = 0.0;
        int cnt = 0;
        for (int i = 0; i < n_e; i++) {
            const int j = inl_e[i];
            const double u1 = kp1[2 * j], v1 = kp1[2 * j + 1], u2 = kp2[2 * j], v2 = kp2[2 * j + 1];
            double& score = part[i % kLanes];
            bool good_point = true;
            const double a2 = f[0] * u1 + f[1] * v1 + f[2];
            const double b2 = f[3] * u1 + f[4] * v1 + f[5];
            const double c2 = f[6] * u1 + f[7] * v1 + f[8];
            const double num2 = a2 * u2 + b2 * v2 + c2;
            const double squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
            const double chiSquare1 = squareDist1 * inv_s2;
            if (chiSquare1 > th) {
                score += 0;
                good_point = false;
            } else
                score += th_score - chiSquare1;
            const double a1 = f[0] * u2 + f[3] * v2 + f[6];
            const double b1 = f[1] * u2 + f[4] * v2 + f[7];
            const double c1 = f[2] * u2 + f[5] * v2 + f[8];
            const double num1 = a1 * u1 + b1 * v1 + c1;
            const double squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
            const double chiSquare2 = squareDist2 * inv_s2;
            if (chiSquare2 > th) {
                score += 0;
                good_point = false;
            } else
                score += th_score - chiSquare2;
            if (good_point) kept_e[cnt++] = j;
        }
        double s = 0.0;
        for (int l = 0; l < kLanes; l++) s = s + part[l];
        *score_e = n_e ? s : 0.0;
        *n_kept_e = cnt;
    }
    if (H) {
        double Hi[9];
        invert3(H, Hi);
        const double th = 5.991;
        for (int l = 0; l < kLanes; l++) part[l] = 0.0;
        int cnt = 0;
        for (int i = 0; i < n_h; i++) {
            const int j = inl_h[i];
            const double u1 = kp1[2 * j], v1 = kp1[2 * j + 1], u2 = kp2[2 * j], v2 = kp2[2 * j + 1];
            double& score = part[i % kLanes];
            bool good_point = true;
            const double w2in1inv = 1.0 / (Hi[6] * u2 + Hi[7] * v2 + Hi[8]);
            const double u2in1 = (Hi[0] * u2 + Hi[1] * v2 + Hi[2]) * w2in1inv;
            const double v2in1 = (Hi[3] * u2 + Hi[4] * v2 + Hi[5]) * w2in1inv;
            const double squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
            const double chiSquare1 = squareDist1 * inv_s2;
            if (chiSquare1 > th)
                good_point = false;
            else
                score += th - chiSquare1;
            const double w1in2inv = 1.0 / (H[6] * u1 + H[7] * v1 + H[8]);
            const double u1in2 = (H[0] * u1 + H[1] * v1 + H[2]) * w1in2inv;
            const double v1in2 = (H[3] * u1 + H[4] * v1 + H[5]) * w1in2inv;
            const double squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
            const double chiSquare2 = squareDist2 * inv_s2;
            if (chiSquare2 > th)
                good_point = false;
            else
                score += th - chiSquare2;
            if (good_point) kept_h[cnt++] = j;
        }
        double s = 0.0;
        for (int l = 0; l < kLanes; l++) s = s + part[l];
        *score_h = n_h ? s : 0.0;
        *n_kept_h = cnt;
    }
}

void ir_invert3(const double* M, double* out) { invert3(M, out); }
}
