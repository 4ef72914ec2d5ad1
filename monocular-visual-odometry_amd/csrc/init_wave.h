// csrc/init_wave.h -- the per-point part of the finish of the monocular initialisation (track_kernels.hip:
// k_init_finish).  Reference: the rest of VisualOdometry::estimateMotionAnd3DPoints_ after
// helperEstimatePossibleRelativePosesByEpipolarGeometry (src/vo/vo.cpp:77-92), the angle of
// retainGoodTriangulationResult_ (vo.cpp:203-211) and the pixel distance of isVoGoodToInit_'s criteria_1
// (geometry::computeMeanDistBetweenKeypoints -> basics::calcDist, opencv_funcs.cpp:132-136).
//
// Per-lane code: every lane works on its own inlier of the chosen solution.  Declared arithmetic (DESIGN.md
// section 12), no fused multiply-add anywhere:
//   p_curr    basics::transCoord(p1, R, t) = pw::trans_coord: (float)(((R_r0 x + R_r1 y) + R_r2 z) + t_r)
//   p_world   basics::preTranslatePoint3f(p_curr, T_w_c_curr): acc = 0, then += T_rj * q_j for j = 0..3 with
//             q = (x, y, z, 1.0), rounded to float
//   rays      to_curr_r = T_w_c_curr(r, 3) - p_world_r, to_ref_r = T_w_c_ref(r, 3) - p_world_r
//   cosang    dot / (sqrt(n1) * sqrt(n2)); dot, n1, n2 start from 0 and add r = 0..2 in order (the cosine that
//             mvo_retain_good_triangulation passes to acos; the acos stays on the host)
//   pixdist   dx, dy are FLOAT differences of the two pixels widened to double; sqrt(dx * dx + dy * dy)
#ifndef MVO_INIT_WAVE_H
#define MVO_INIT_WAVE_H
#include "pnp_wave.h"

namespace pw {

// T_w_c_curr and T_w_c_ref (row-major 4 x 4) as k_init_finish takes them: kernel arguments
struct InitFinishPoses {
    double curr[16], ref[16];
};

PW_FN void init_finish_point(const float (&p1)[3], const double (&R)[9], const double (&t)[3], const InitFinishPoses& T,
                             const float (&px1)[2], const float (&px2)[2], float (&p_curr)[3], double* cosang,
                             double* pixdist) {
    trans_coord(p1, R, t, p_curr);
    double to_curr[3], to_ref[3];
    PW_UNROLL
    for (int r = 0; r < 3; r++) {
        double acc = 0;
        acc += T.curr[4 * r] * (double)p_curr[0];
        acc += T.curr[4 * r + 1] * (double)p_curr[1];
        acc += T.curr[4 * r + 2] * (double)p_curr[2];
        acc += T.curr[4 * r + 3] * 1.0;
        const double pw_r = (double)(float)acc;
        to_curr[r] = T.curr[4 * r + 3] - pw_r;
        to_ref[r] = T.ref[4 * r + 3] - pw_r;
    }
    double dot = 0, n1 = 0, n2 = 0;
    PW_UNROLL
    for (int r = 0; r < 3; r++) dot += to_curr[r] * to_ref[r];
    PW_UNROLL
    for (int r = 0; r < 3; r++) n1 = n1 + to_curr[r] * to_curr[r];
    PW_UNROLL
    for (int r = 0; r < 3; r++) n2 = n2 + to_ref[r] * to_ref[r];
    *cosang = dot / (sqrt(n1) * sqrt(n2));
    const double dx = px1[0] - px2[0], dy = px1[1] - px2[1];
    *pixdist = sqrt(dx * dx + dy * dy);
}

}  // namespace pw
#endif
