// tests/init_finish_restatement.cpp -- TEST INFRASTRUCTURE: the finish of the monocular initialisation (the rest of
// VisualOdometry::estimateMotionAnd3DPoints_ after helperEstimatePossibleRelativePosesByEpipolarGeometry,
// retainGoodTriangulationResult_ and isVoGoodToInit_, src/vo/vo.cpp:77-244) restated sequentially, one point after the
// other, in the arithmetic csrc/init_wave.h and DESIGN.md section 12 declare (compiled by tests/finish_restate.py with
// g++ -ffp-contract=off).  Everything up to the chosen slot comes from tests/pose_restate.py.
//   pose       T = T_ref * [R t; 0 1]^-1, the inverse by the oracle's partial-pivoting LU, the product summed k = 0..3
//   p_curr     (float)(((R_r0 x + R_r1 y) + R_r2 z) + t_r)
//   cosang     preTranslatePoint3f summed j = 0..3 from 0 and rounded to float; the two rays; dot, n1, n2 summed
//              r = 0..2 from 0; dot / (sqrt(n1) * sqrt(n2))
//   pixdist    float differences widened to double, sqrt(dx dx + dy dy)
//   tail       acos / 3.1415926 * 180, the median of a sorted copy, the keep rule in list order, N < 20, the depth
//              scaling, the three criteria
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../oracle/linalg_oracle.h"

namespace {

void compose(const double* T_ref, const double* R, const double* t, double* T) {
    const double M[16] = {R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2], 0, 0, 0, 1};
    double Mi[16];
    if (!orc_linalg::invert4x4_lu(M, Mi))
        for (double& v : Mi) v = 0;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double v = T_ref[4 * i] * Mi[j];
            v = v + T_ref[4 * i + 1] * Mi[4 + j];
            v = v + T_ref[4 * i + 2] * Mi[8 + j];
            T[4 * i + j] = v + T_ref[4 * i + 3] * Mi[12 + j];
        }
}

}  // namespace

extern "C" {

struct fr_params {
    double min_triang_angle, max_ratio_to_median, assumed_mean_depth;
    int min_inlier_matches;
    double min_pixel_dist, min_median_triangulation_angle;
};

void fr_compose(const double* T_ref, const double* R, const double* t, double* T) { compose(T_ref, R, t, T); }

// p1: the slot's points in camera 1 (m x 3), px1 / px2: the pixels of the slot's matches (m x 2 each), in list order.
// Outputs per entry: p_curr, cosang, pixdist, angle; the kept list (positions in the list), the kept (scaled) points
// and angles; scal[0..6] = mean_depth, scale, mean_pixel_dist, mean / median / min / max angle; flags[0..5] = n_kept,
// scaled, criteria 0..2, good.  R, t, T: in = the slot's motion, out = t scaled and the final pose.
// Returns the number of NaN angles (the tests require 0).
int fr_finish(const float* p1, const float* px1, const float* px2, int m, const double* R, double* t,
              const double* T_ref, const fr_params* prm, float* p_curr, double* cosang, double* pixdist, double* angle,
              int32_t* kept, float* kept_pts, double* kept_angles, double* T, double* scal, int32_t* flags) {
    compose(T_ref, R, t, T);
    int n_nan = 0;
    for (int i = 0; i < m; i++) {
        const float* p = p1 + 3 * i;
        float* pc = p_curr + 3 * i;
        for (int r = 0; r < 3; r++) {
            double s = R[3 * r] * (double)p[0] + R[3 * r + 1] * (double)p[1];
            s = s + R[3 * r + 2] * (double)p[2];
            pc[r] = (float)(s + t[r]);
        }
        double to_curr[3], to_ref[3];
        for (int r = 0; r < 3; r++) {
            double acc = 0;
            acc += T[4 * r] * (double)pc[0];
            acc += T[4 * r + 1] * (double)pc[1];
            acc += T[4 * r + 2] * (double)pc[2];
            acc += T[4 * r + 3] * 1.0;
            const double pw = (double)(float)acc;
            to_curr[r] = T[4 * r + 3] - pw;
            to_ref[r] = T_ref[4 * r + 3] - pw;
        }
        double dot = 0, n1 = 0, n2 = 0;
        for (int r = 0; r < 3; r++) dot += to_curr[r] * to_ref[r];
        for (int r = 0; r < 3; r++) n1 = n1 + to_curr[r] * to_curr[r];
        for (int r = 0; r < 3; r++) n2 = n2 + to_ref[r] * to_ref[r];
        cosang[i] = dot / (std::sqrt(n1) * std::sqrt(n2));
        angle[i] = std::acos(cosang[i]) / 3.1415926 * 180.0;
        n_nan += std::isnan(angle[i]) ? 1 : 0;
        const double dx = px1[2 * i] - px2[2 * i], dy = px1[2 * i + 1] - px2[2 * i + 1];
        pixdist[i] = std::sqrt(dx * dx + dy * dy);
    }
    int n_kept = 0;
    double sum_pix = 0;
    if (m > 0) {
        std::vector<double> sorted(angle, angle + m);
        std::sort(sorted.begin(), sorted.end());
        const double median = sorted[m / 2];
        for (int i = 0; i < m; i++) {
            if (angle[i] < prm->min_triang_angle || angle[i] / median > prm->max_ratio_to_median) continue;
            kept[n_kept] = i;
            std::memcpy(kept_pts + 3 * n_kept, p_curr + 3 * i, 12);
            kept_angles[n_kept] = angle[i];
            sum_pix += pixdist[i];
            n_kept++;
        }
    }
    for (int k = 0; k < 7; k++) scal[k] = 0;
    int scaled = 0;
    if (n_kept >= 20) {
        double mean_depth = 0;
        for (int i = 0; i < n_kept; i++) mean_depth += (double)kept_pts[3 * i + 2];
        mean_depth /= n_kept;
        const double scale = prm->assumed_mean_depth / mean_depth;
        for (int k = 0; k < 3; k++) t[k] *= scale;
        for (int k = 0; k < 3 * n_kept; k++) kept_pts[k] = (float)((double)kept_pts[k] * scale);
        compose(T_ref, R, t, T);
        scal[0] = mean_depth;
        scal[1] = scale;
        scaled = 1;
    }
    const int c0 = !(n_kept < prm->min_inlier_matches);
    scal[2] = sum_pix / n_kept;
    const int c1 = scal[2] > prm->min_pixel_dist;
    int c2 = 0;
    if (n_kept > 0) {
        std::vector<double> a(kept_angles, kept_angles + n_kept);
        std::sort(a.begin(), a.end());
        double acc = 0.0;
        for (double v : a) acc += v;
        scal[3] = acc / n_kept;
        scal[4] = a[n_kept / 2];
        scal[5] = a[0];
        scal[6] = a[n_kept - 1];
        c2 = scal[4] > prm->min_median_triangulation_angle;
    }
    flags[0] = n_kept;
    flags[1] = scaled;
    flags[2] = c0;
    flags[3] = c1;
    flags[4] = c2;
    flags[5] = c0 && c1 && c2;
    return n_nan;
}
}
