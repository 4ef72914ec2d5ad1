// my_slam/vo/pose_optimization.h -- the per-frame pose from a robust motion-only optimisation over all matches.  The reference's
// poseEstimationPnP_ (vo.cpp:291-347) hands its matches to cv::solvePnPRansac: 100 minimal subsets, then a fit on the winner's
// inliers.  With tracking by projection (my_slam/vo/projection_match.h) every match already lies within a few pixels of where a
// predicted pose put it; ORB-SLAM, which that step follows, has no RANSAC here: TrackWithMotionModel calls
// Optimizer::PoseOptimization, a Huber-weighted Levenberg-Marquardt over the six pose unknowns from the predicted pose over ALL
// matches, which classifies inliers and outliers in four rounds.  Executed by libmvo_hip.so through the hot-path context of the
// calling thread (mvo_optimize_pose, include/mvo_hip.h; declared arithmetic: DESIGN.md section 21).
//   optimizePoseFromMatches   the matches' map points and pixels, inv_sigma2 = (float)(1 / (scale scale)) with the f32 scale
//                             matchMapByProjection gives the matched keypoint (scale_factor multiplied octave times), the
//                             predicted pose in curr->T_w_c_; the call; on status 0 the non-outliers in ascending order and the
//                             optimised T_w_c
// poseEstimationPnP (pnp_tracking.h) calls it after matchMapByProjection when the optional key `tracking_pose_by_optimization` is 1
// (default 0: nothing is called, nothing changes) and there are at least min_inliers matches; the result stands in for the PnP
// inliers and for invT(convertRt2T(R, t)); on any other status the frame falls back to solvePnPRansac exactly as without the
// key.  The key requires `tracking_match_by_projection: 1`.  Optional keys `pose_optimization_rounds` (default 4),
// `pose_optimization_iterations` (10), `pose_optimization_min_inliers` (10), `pose_optimization_chi2_threshold` (5.991).
#ifndef MY_SLAM_POSE_OPTIMIZATION_H
#define MY_SLAM_POSE_OPTIMIZATION_H
#include <cmath>

#include "my_slam/vo/pnp_tracking.h"

// Bound weakly: a program that includes this header still links and runs against a build of the library without the pose
// optimisation; calling optimizePoseFromMatches with such a library is an error, not a fall-back.
#pragma weak mvo_optimize_pose

namespace my_slam {
namespace vo {

inline bool trackingPoseByOptimization() {  // the optional key, latched on first use
    static const bool on = basics::Config::has("tracking_pose_by_optimization") && basics::Config::get<int>("tracking_pose_by_optimization") != 0;
    return on;
}

inline mvo_pose_optimize_params poseOptimizationParams() {  // the optional keys, latched on first use
    static const mvo_pose_optimize_params p = [] {
        mvo_pose_optimize_params q{4, 10, 10, 5.991, std::sqrt(5.991), 1e-6};
        if (basics::Config::has("pose_optimization_rounds")) q.rounds = basics::Config::get<int>("pose_optimization_rounds");
        if (basics::Config::has("pose_optimization_iterations")) q.iterations = basics::Config::get<int>("pose_optimization_iterations");
        if (basics::Config::has("pose_optimization_min_inliers")) q.min_inliers = basics::Config::get<int>("pose_optimization_min_inliers");
        if (basics::Config::has("pose_optimization_chi2_threshold")) q.chi2_threshold = basics::Config::get<double>("pose_optimization_chi2_threshold");
        return q;
    }();
    return p;
}

inline int poseOptimizationMinInliers() { return poseOptimizationParams().min_inliers; }

// pts_3d[i] / pts_2d[i] belong to curr->matches_with_map_[i].  Returns the status; 0 fills inliers and T_w_c.  curr receives what
// the call saw and gave, for the frame log.
inline int optimizePoseFromMatches(const Frame::Ptr& curr, const vector<cv::Point3f>& pts_3d, const vector<cv::Point2f>& pts_2d,
                                   const cv::Mat& K, vector<int>& inliers, cv::Mat& T_w_c) {
    if (!mvo_optimize_pose) throw std::runtime_error("optimizePoseFromMatches: this libmvo_hip.so has no mvo_optimize_pose");
    static const double scale_factor = basics::Config::get<double>("scale_factor");
    const int n = (int)pts_3d.size();
    if ((int)pts_2d.size() != n || (int)curr->matches_with_map_.size() != n)
        throw std::runtime_error("optimizePoseFromMatches: one point and one pixel per match are required");
    vector<float> p3(3 * (size_t)n), p2(2 * (size_t)n), sigma(n);
    for (int i = 0; i < n; ++i) {
        p3[3 * i] = pts_3d[i].x, p3[3 * i + 1] = pts_3d[i].y, p3[3 * i + 2] = pts_3d[i].z;
        p2[2 * i] = pts_2d[i].x, p2[2 * i + 1] = pts_2d[i].y;
        double s = 1.0;
        for (int o = 0; o < curr->keypoints_[curr->matches_with_map_[i].trainIdx].octave; ++o) s *= scale_factor;
        const float scale = (float)s;  // (as matchMapByProjection computes it)
        sigma[i] = (float)(1.0 / ((double)scale * (double)scale));
    }
    vector<double> T0(16), Twc(16), Tcw(16), chi2(2);
    for (int i = 0; i < 16; ++i) T0[i] = curr->T_w_c_.at<double>(i / 4, i % 4);
    const mvo_pose_optimize_params params = poseOptimizationParams();
    const double fx = K.at<double>(0, 0), fy = K.at<double>(1, 1), cx = K.at<double>(0, 2), cy = K.at<double>(1, 2);
    vector<int> info(6);
    vector<unsigned char> outlier(n > 0 ? n : 1);
    mvo_check(mvo_optimize_pose(hot_path_ctx(), p3.data(), p2.data(), sigma.data(), n, T0.data(), fx, fy, cx, cy, &params, Twc.data(),
                                Tcw.data(), outlier.data(), chi2.data(), info.data()),
              "optimizePoseFromMatches");
    outlier.resize(n);
    inliers.clear();
    if (info[0] == 0) {
        for (int i = 0; i < n; ++i)
            if (!outlier[i]) inliers.push_back(i);
        T_w_c = cv::Mat(4, 4, CV_64FC1);
        for (int i = 0; i < 16; ++i) T_w_c.at<double>(i / 4, i % 4) = Twc[i];
    }
    curr->pose_opt_setup_ = {fx, fy, cx, cy, (double)params.rounds, (double)params.iterations, (double)params.min_inliers,
                             params.chi2_threshold, params.huber_delta, params.rel_tolerance};
    curr->pose_opt_init_ = T0;
    curr->pose_opt_p3_ = p3;
    curr->pose_opt_p2_ = p2;
    curr->pose_opt_sigma_ = sigma;
    curr->pose_opt_T_w_c_ = Twc;
    curr->pose_opt_T_c_w_ = Tcw;
    curr->pose_opt_info_ = info;
    curr->pose_opt_chi2_ = chi2;
    curr->pose_opt_outlier_ = outlier;
    return info[0];
}

}  // namespace vo
}  // namespace my_slam
#endif
