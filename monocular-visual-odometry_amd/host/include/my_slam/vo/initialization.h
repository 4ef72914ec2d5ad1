// my_slam/vo/initialization.h -- the DOING_INITIALIZATION branch of VisualOdometry::addFrame (reference
// src/vo/vo_addFrame.cpp:36-69) with the two members it calls, as free functions on the mirrored Frame:
//   estimateMotionAnd3DPoints   VisualOdometry::estimateMotionAnd3DPoints_ (src/vo/vo.cpp:53-110), executed by
//                               mvo_init_two_view of libmvo_hip.so (both RANSACs, the solution table, the E / H
//                               choice, transCoord, retainGoodTriangulationResult_ and the depth scaling)
//   isVoGoodToInit              VisualOdometry::isVoGoodToInit_ (vo.cpp:112-170) on the fields the first one filled
//   initializeWithFrame         the branch itself: matchFeatures, the two above, then pushCurrPointsToMap_ and
//                               addKeyFrame_ on success, curr->T_w_c_ = ref->T_w_c_ otherwise
// When the E / H rule picks a solution that does not exist (the reference would index list_R[-1]; DESIGN.md section 2,
// deviation 12) the frame gets no inliers and the reference keyframe's pose, and isVoGoodToInit is false.
// InitReport (optional last argument of the first and the third) keeps what mvo_init_two_view said about the frame and
// what the branch decided, for logs (host/driver/run_vo.cpp); nothing of the branch reads it.
#ifndef MY_SLAM_INITIALIZATION_H
#define MY_SLAM_INITIALIZATION_H
#include "my_slam/geometry/feature_match.h"
#include "my_slam/geometry/motion_estimation.h"
#include "my_slam/vo/tracking_loop.h"

namespace my_slam {
namespace vo {

struct InitReport {
    // mvo_init_result of the frame: the chosen solution, the length of its inlier list, the points kept, whether the depth
    // scaling ran, the device's three criteria; good: what isVoGoodToInit returned (the decision the branch took)
    int slot = -1, n_slot_inliers = 0, n_kept = 0, scaled = 0, criteria[3] = {0, 0, 0}, good = 0;
    double mean_depth = 0, scale = 0, median_angle = 0, mean_pixel_dist = 0;
};

inline void estimateMotionAnd3DPoints(const Frame::Ptr& curr, const Frame::Ptr& ref, const cv::Mat& K,
                                      InitReport* report = nullptr) {
    // -- Rename output
    vector<cv::DMatch>& inlier_matches = curr->inliers_matches_with_ref_;
    vector<cv::Point3f>& pts3d_in_curr = curr->inliers_pts3d_;
    vector<cv::DMatch>& inliers_matches_for_3d = curr->inliers_matches_for_3d_;
    vector<double>& angles = curr->triangulation_angles_of_inliers_;
    // epipolar_geometry.cpp:31-32 and vo.cpp:103-104,183-185: latched on first use
    static const double findEssentialMat_prob = basics::Config::get<double>("findEssentialMat_prob");
    static const double findEssentialMat_threshold = basics::Config::get<double>("findEssentialMat_threshold");
    static const mvo_init_params params = {
        basics::Config::get<double>("min_triang_angle"),
        basics::Config::get<double>("max_ratio_between_max_angle_and_median_angle"),
        basics::Config::get<double>("assumed_mean_pts_depth_during_vo_init"),
        basics::Config::get<int>("min_inlier_matches"),
        basics::Config::get<double>("min_pixel_dist"),
        basics::Config::get<double>("min_median_triangulation_angle")};
    const vector<cv::DMatch>& matches = curr->matches_with_ref_;
    vector<cv::Point2f> pts1, pts2;
    geometry::extractPtsFromMatches(ref->keypoints_, curr->keypoints_, matches, pts1, pts2);
    const int n = (int)pts1.size(), cap = n > 0 ? n : 1;
    vector<int32_t> inl_e(cap), inl_h(cap), for_3d(cap);
    vector<float> sols_pts((size_t)5 * cap * 3), pts((size_t)cap * 3);
    vector<double> ang(cap);
    mvo_init_poses poses{};
    poses.inliers_e = inl_e.data();
    poses.inliers_h = inl_h.data();
    poses.cap_inliers = cap;
    poses.pts3d = sols_pts.data();
    poses.cap_pts = 5 * cap;
    mvo_init_result res{};
    res.matches_for_3d = for_3d.data();
    res.pts3d_in_curr = pts.data();
    res.angles = ang.data();
    res.cap = cap;
    double T_ref[16];
    for (int i = 0; i < 16; ++i) T_ref[i] = ref->T_w_c_.at<double>(i / 4, i % 4);
    // estiMotionByHomography's threshold 3 and findHomography's default confidence; sigma 1 (motion_estimation.h:104,110)
    mvo_check(mvo_init_two_view(hot_path_ctx(), n ? &pts1[0].x : nullptr, n ? &pts2[0].x : nullptr, n, K.at<double>(0, 0),
                                K.at<double>(1, 1), K.at<double>(0, 2), K.at<double>(1, 2), findEssentialMat_prob,
                                findEssentialMat_threshold, 3.0, 0.995, 1.0, T_ref, &params, &poses, &res),
              "estimateMotionAnd3DPoints");
    // -- Only retain the data of the best solution
    inlier_matches.clear();
    pts3d_in_curr.clear();
    inliers_matches_for_3d.clear();
    angles.clear();
    if (res.slot >= 0) {
        const int32_t* list = res.slot == 0 ? poses.inliers_e : poses.inliers_h;
        for (int i = 0; i < res.n_slot_inliers; ++i) {  // motion_estimation.cpp:174-179
            const cv::DMatch& m = matches[list[i]];
            inlier_matches.push_back(cv::DMatch(m.queryIdx, m.trainIdx, m.distance));
        }
    }
    for (int i = 0; i < res.n_kept; ++i) {
        const cv::DMatch& m = matches[res.matches_for_3d[i]];
        inliers_matches_for_3d.push_back(cv::DMatch(m.queryIdx, m.trainIdx, m.distance));
        pts3d_in_curr.push_back(cv::Point3f(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]));
        angles.push_back(res.angles[i]);
    }
    // -- compute camera pose
    curr->T_w_c_ = cv::Mat(4, 4, CV_64FC1);
    for (int i = 0; i < 16; ++i) curr->T_w_c_.at<double>(i / 4, i % 4) = res.T_w_c[i];
    if (report) {
        report->slot = res.slot;
        report->n_slot_inliers = res.n_slot_inliers;
        report->n_kept = res.n_kept;
        report->scaled = res.scaled;
        for (int i = 0; i < 3; ++i) report->criteria[i] = res.criteria[i];
        report->mean_depth = res.mean_depth;
        report->scale = res.scale;
        report->median_angle = res.median_angle;
        report->mean_pixel_dist = res.mean_pixel_dist;
    }
}

inline bool isVoGoodToInit(const Frame::Ptr& curr, const Frame::Ptr& ref) {
    const vector<cv::DMatch>& matches = curr->inliers_matches_for_3d_;
    static const int min_inlier_matches = basics::Config::get<int>("min_inlier_matches");
    static const double min_pixel_dist = basics::Config::get<double>("min_pixel_dist");
    static const double min_median_triangulation_angle = basics::Config::get<double>("min_median_triangulation_angle");
    // -- Check CRITERIA_0: num inliers should be large
    const bool criteria_0 = !((int)matches.size() < min_inlier_matches);
    // -- Check criteria_1: init vo only when distance between matched keypoints are large
    const bool criteria_1 = geometry::computeMeanDistBetweenKeypoints(ref->keypoints_, curr->keypoints_, matches) > min_pixel_dist;
    // -- Check criteria_2: the median triangulation angle should be larger than threshold
    bool criteria_2 = false;
    if (curr->triangulation_angles_of_inliers_.size() > 0) {
        vector<double> sort_a = curr->triangulation_angles_of_inliers_;
        const int N = (int)sort_a.size();
        std::sort(sort_a.begin(), sort_a.end());
        if (sort_a[N / 2] > min_median_triangulation_angle) criteria_2 = true;
    }
    return criteria_0 && criteria_1 && criteria_2;
}

// vo_addFrame.cpp:36-69; st.ref_ is the first keyframe (the BLANK branch inserted it).  Returns whether the VO
// initialised with this frame (the caller then switches to trackFrame).
inline bool initializeWithFrame(TrackingState& st, const Frame::Ptr& curr, const cv::Mat& K, InitReport* report = nullptr) {
    static const float max_matching_pixel_dist_in_initialization =
        basics::Config::get<float>("max_matching_pixel_dist_in_initialization");
    static const int method_index = (int)basics::Config::get<float>("feature_match_method_index_initialization");
    st.pushFrameToBuff(curr);
    geometry::matchFeatures(st.ref_->descriptors_, curr->descriptors_, curr->matches_with_ref_, method_index, false,
                            st.ref_->keypoints_, curr->keypoints_, max_matching_pixel_dist_in_initialization);
    estimateMotionAnd3DPoints(curr, st.ref_, K, report);
    const bool good = isVoGoodToInit(curr, st.ref_);
    if (report) report->good = good ? 1 : 0;
    if (good) {
        pushCurrPointsToMap(st, curr);
        st.map_->insertKeyFrame(curr);  // addKeyFrame_
        st.ref_ = curr;
        return true;
    }
    curr->T_w_c_ = st.ref_->T_w_c_;  // skip this frame
    return false;
}

}  // namespace vo
}  // namespace my_slam
#endif
