// my_slam/vo/frame.h -- Frame / PtConn with the reference's field names (include/my_slam/vo/frame.h:16-96); only the
// members the hot path reads or writes are kept (camera / triangulation helpers live outside the hot path).
#ifndef MY_SLAM_FRAME_H
#define MY_SLAM_FRAME_H
#include "my_slam/common_include.h"
#include "my_slam/geometry/feature_match.h"
#include "my_slam/geometry/orb_distribute.h"

namespace my_slam {
namespace vo {

typedef struct PtConn_ {
    int pt_ref_idx;
    int pt_map_idx;
} PtConn;

class Frame {
public:
    typedef std::shared_ptr<Frame> Ptr;
    static int& factory_id() {
        static int id = 0;
        return id;
    }

public:
    int id_ = 0;
    double time_stamp_ = -1;

    // -- image features
    cv::Mat rgb_img_;
    vector<cv::KeyPoint> keypoints_;
    cv::Mat descriptors_;
    vector<vector<unsigned char>> kpts_colors_;  // rgb colors

    // -- Matches with reference keyframe / map
    vector<cv::DMatch> matches_with_ref_;
    vector<cv::DMatch> inliers_matches_with_ref_;
    vector<cv::DMatch> inliers_matches_for_3d_;
    vector<cv::Point3f> inliers_pts3d_;
    vector<double> triangulation_angles_of_inliers_;
    std::unordered_map<int, PtConn> inliers_to_mappt_connections_;  // curr idx -> idx in ref, and map
    vector<cv::DMatch> matches_with_map_;
    // (not in the reference) `triangulation_match_by_epipolar_line: 1`: the F that gated matches_with_ref_, the keyframe it
    // was taken against and that keyframe's pose at that moment (the window BA of later frames moves a keyframe's T_w_c_
    // after it was inserted); empty matrices otherwise
    cv::Mat epipolar_F_;
    cv::Mat epipolar_ref_T_w_c_;
    int epipolar_ref_id_ = -1;
    // (not in the reference) `tracking_match_by_projection: 1`: what the matcher of poseEstimationPnP saw -- the two poses the
    // prediction was made from (32 f64: T_prev2 then T_prev, T_prev twice without a prev2), the predicted pose, the map's
    // positions (n x 3) and descriptors (n x 32) as uploaded, and the matches handed to PnP before the inlier selection.  The
    // bundle adjustment rewrites poses and positions in place afterwards; empty otherwise
    vector<double> projection_prev_T_;
    cv::Mat projection_pred_T_;
    vector<float> projection_map_pos_;
    vector<unsigned char> projection_map_desc_;
    vector<cv::DMatch> projection_matches_;
    // (not in the reference) `tracking_pose_by_optimization: 1`: whether the frame fell back to solvePnPRansac (-1: the step was
    // not reached) and, if the optimisation was called (my_slam/vo/pose_optimization.h), what it saw and gave: the intrinsics and
    // parameters (fx, fy, cx, cy, rounds, iterations, min_inliers, chi2_threshold, huber_delta, rel_tolerance), the predicted pose
    // (16), the matches' map points (n x 3), pixels (n x 2) and inv_sigma2 (n), T_w_c and T_c_w (16 each), info (6), chi2 (2), the
    // outlier flags (n); empty otherwise
    int pose_opt_fallback_ = -1;
    vector<double> pose_opt_setup_, pose_opt_init_, pose_opt_T_w_c_, pose_opt_T_c_w_, pose_opt_chi2_;
    vector<float> pose_opt_p3_, pose_opt_p2_, pose_opt_sigma_;
    vector<int> pose_opt_info_;
    vector<unsigned char> pose_opt_outlier_;
    // (not in the reference) `tracking_local_map: 1` (my_slam/vo/local_map.h): whether the second search was made (-1: not) and
    // applied, its outcome (LocalMapOutcome) and what it saw and gave: the intrinsics, image size, number of levels, parameters
    // and level scales; the optimised pose going in (16); the skip mask (n), the keypoints' levels (nt, -2: connected), the map
    // as resident (n x 3 positions, n x 32 descriptors) with its view data (n x 3 normals, n largest distances); the new matches
    // (queryIdx = map row); then, if the second optimisation was called, its points (k x 3), pixels (k x 2), inv_sigma2 (k), T_w_c
    // (16), info (6), chi2 (2) and outlier flags (k); empty otherwise
    int local_map_applied_ = -1, local_map_outcome_ = -1;
    vector<double> local_map_setup_, local_map_init_, local_map_T_w_c_, local_map_chi2_;
    vector<unsigned char> local_map_skip_, local_map_desc_, local_map_outlier_;
    vector<int> local_map_t_level_, local_map_info_;
    vector<float> local_map_pos_, local_map_normal_, local_map_max_dist_, local_map_p3_, local_map_p2_, local_map_sigma_;
    vector<cv::DMatch> local_map_matches_;
    // (not in the reference) `map_point_refresh: 1`, on the keyframe after whose insertion the map points were refreshed
    // (my_slam/vo/map_refresh.h): the ids of MapOnDevice::order() as the frame's own tracking step saw it (the refresh re-reads
    // the map), then in the order of the refreshed map: the observation starts (n + 1), the observations' descriptors
    // (n_obs x 32) and camera centres (n_obs x 3), the positions as resident (n x 3), the chosen observation per point and the
    // normals (n x 3); empty otherwise
    vector<int> refresh_order_before_;
    vector<int> refresh_obs_start_;
    vector<unsigned char> refresh_obs_desc_;
    vector<double> refresh_obs_cam_;
    vector<float> refresh_pos_;
    vector<int> refresh_choice_;
    vector<double> refresh_norm_;
    bool refreshed_ = false;
    // (not in the reference) `map_point_refine_positions: 1`, on the keyframe after whose insertion the map point positions
    // were refined (my_slam/vo/map_refine.h): the ids of MapOnDevice::order() as the frame's own tracking step saw it, then
    // what the call saw and gave, in the order of the map it read: the intrinsics and parameters (fx, fy, cx, cy, max_trials,
    // min_observations, huber_delta, rel_tolerance), the poses of frames_buff_ (n_frames x 16), the observation starts
    // (n + 1), frame indices and pixels (n_obs, n_obs x 2), the positions before and after (n x 3 each), chi2 (n x 2), info
    // (n x 3), the outlier flags (n_obs); empty otherwise
    vector<int> refine_order_before_;
    vector<double> refine_setup_;
    vector<double> refine_T_w_c_;
    vector<int> refine_obs_start_;
    vector<int> refine_obs_frame_;
    vector<float> refine_obs_uv_;
    vector<float> refine_pos_before_;
    vector<float> refine_pos_after_;
    vector<double> refine_chi2_;
    vector<int> refine_info_;
    vector<unsigned char> refine_outlier_;
    bool positions_refined_ = false;
    // (not in the reference) `map_point_fuse: 1`, on the keyframe after whose insertion duplicate map points were fused
    // (my_slam/vo/map_fuse.h): the ids of MapOnDevice::order() as the frame's own tracking step saw it, then what the call saw and
    // gave: the intrinsics, image size and parameters (fx, fy, cx, cy, cols, rows, max_px, max_hamming), the map as resident (ids,
    // n x 3 positions, n x 32 descriptors), the frames of frames_buff_ (keypoints per frame, n_frames x 16 poses, then frame after
    // frame the descriptors, pixels, scales and connections), replaced_by (n), added (n_added x 3), counts (6) and the ids of the
    // map after the call; empty otherwise
    vector<int> fuse_order_before_;
    vector<double> fuse_setup_;
    vector<int> fuse_map_ids_;
    vector<float> fuse_map_pos_;
    vector<unsigned char> fuse_map_desc_;
    vector<int> fuse_kp_count_;
    vector<double> fuse_T_w_c_;
    vector<unsigned char> fuse_desc_;
    vector<float> fuse_xy_, fuse_scale_;
    vector<int> fuse_conn_;
    vector<int> fuse_replaced_by_;
    vector<int> fuse_added_;
    vector<int> fuse_counts_;
    vector<int> fuse_map_ids_after_;
    bool fused_ = false;
    // (not in the reference) `map_point_create_from_window: 1`, on the keyframe at whose insertion new map points were made from
    // every buffered frame (my_slam/vo/window_triangulate.h), what the call saw and gave: the intrinsics and parameters (fx, fy,
    // cx, cy, max_line_px, lowe_ratio, max_hamming, max_cos_parallax, max_reproj_chi2, ratio_factor, min_baseline), the frames of
    // frames_buff_ with the keyframe last (keypoints per frame, n_frames x 16 poses, then frame after frame the descriptors,
    // pixels, scales and connections), the points (keypoint, frame, train, hamming; p_curr; cos2), the pairs (frame, keypoint,
    // train, hamming, status; p_curr, p_frame; cos2), counts (12), the ids and world positions of the new map points and the
    // size of the map before and after; empty otherwise
    vector<double> window_setup_;
    vector<int> window_kp_count_;
    vector<double> window_T_w_c_;
    vector<unsigned char> window_desc_;
    vector<float> window_xy_, window_scale_;
    vector<int> window_conn_;
    vector<int> window_points_;
    vector<float> window_points_p_;
    vector<double> window_points_cos2_;
    vector<int> window_pairs_;
    vector<float> window_pairs_p_;
    vector<double> window_pairs_cos2_;
    vector<int> window_counts_;
    vector<int> window_ids_;
    vector<float> window_world_;
    vector<int> window_map_size_;
    bool window_created_ = false;
    // (not in the reference) `orb_distribute_keypoints: 1`: per pyramid level, the candidates of calcKeyPoints and the key
    // points it kept (before calcDescriptors drops those near the image border); empty otherwise
    vector<int> distribute_candidates_per_level_;
    vector<int> distribute_keypoints_per_level_;

    // -- Current pose (cam -> world, see vo.cpp:31,89)
    cv::Mat T_w_c_;

public:
    static Frame::Ptr createFrame(cv::Mat rgb_img, double time_stamp = -1) {
        Frame::Ptr f(new Frame());
        f->rgb_img_ = rgb_img;
        f->id_ = factory_id()++;
        f->time_stamp_ = time_stamp;
        f->T_w_c_ = cv::Mat::eye(4, 4, CV_64FC1);
        return f;
    }
    void clearNoUsed() {
        kpts_colors_.clear();
        matches_with_ref_.clear();
        inliers_matches_with_ref_.clear();
        inliers_matches_for_3d_.clear();
        matches_with_map_.clear();
        local_map_skip_.clear(), local_map_desc_.clear(), local_map_pos_.clear();  // (logged by now; local_map_applied_ stays)
        local_map_normal_.clear(), local_map_max_dist_.clear(), local_map_t_level_.clear(), local_map_matches_.clear();
        local_map_p3_.clear(), local_map_p2_.clear(), local_map_sigma_.clear(), local_map_outlier_.clear();
        refresh_order_before_.clear();  // (logged by now; refreshed_ stays)
        refresh_obs_start_.clear();
        refresh_obs_desc_.clear();
        refresh_obs_cam_.clear();
        refresh_pos_.clear();
        refresh_choice_.clear();
        refresh_norm_.clear();
        refine_order_before_.clear();  // (logged by now; positions_refined_ stays)
        refine_setup_.clear();
        refine_T_w_c_.clear();
        refine_obs_start_.clear();
        refine_obs_frame_.clear();
        refine_obs_uv_.clear();
        refine_pos_before_.clear();
        refine_pos_after_.clear();
        refine_chi2_.clear();
        refine_info_.clear();
        refine_outlier_.clear();
        fuse_order_before_.clear();  // (logged by now; fused_ stays)
        fuse_setup_.clear();
        fuse_map_ids_.clear();
        fuse_map_pos_.clear();
        fuse_map_desc_.clear();
        fuse_kp_count_.clear();
        fuse_T_w_c_.clear();
        fuse_desc_.clear();
        fuse_xy_.clear();
        fuse_scale_.clear();
        fuse_conn_.clear();
        fuse_replaced_by_.clear();
        fuse_added_.clear();
        fuse_counts_.clear();
        fuse_map_ids_after_.clear();
        window_setup_.clear();  // (logged by now; window_created_ stays)
        window_kp_count_.clear();
        window_T_w_c_.clear();
        window_desc_.clear();
        window_xy_.clear();
        window_scale_.clear();
        window_conn_.clear();
        window_points_.clear();
        window_points_p_.clear();
        window_points_cos2_.clear();
        window_pairs_.clear();
        window_pairs_p_.clear();
        window_pairs_cos2_.clear();
        window_counts_.clear();
        window_ids_.clear();
        window_world_.clear();
        window_map_size_.clear();
    }
    void calcKeyPoints() {
        if (geometry::orbDistributeKeypoints())  // the ORB-SLAM way (my_slam/geometry/orb_distribute.h)
            geometry::calcKeyPointsDistributed(rgb_img_, keypoints_, &distribute_candidates_per_level_, &distribute_keypoints_per_level_);
        else
            geometry::calcKeyPoints(rgb_img_, keypoints_);
        geometry::detail::pyramid_token() = (long long)id_ + 1;  // the ctx now caches THIS frame's pyramid
    }
    void calcDescriptors() {
        // same image as calcKeyPoints -> the device pyramid is reused (the reference builds it twice)
        geometry::detail::reuse_pyramid_flag() = geometry::detail::pyramid_token() == (long long)id_ + 1;
        geometry::calcDescriptors(rgb_img_, keypoints_, descriptors_);
        geometry::detail::reuse_pyramid_flag() = false;
        kpts_colors_.clear();
        for (const cv::KeyPoint& kpt : keypoints_) {  // frame.h:80-85 + basics::getPixelAt: BGR -> r,g,b
            int x = (int)std::floor(kpt.pt.x), y = (int)std::floor(kpt.pt.y);
            const unsigned char* px = rgb_img_.ptr<unsigned char>(y) + (size_t)x * rgb_img_.channels();
            if (rgb_img_.channels() >= 3)
                kpts_colors_.push_back({px[2], px[1], px[0]});
            else
                kpts_colors_.push_back({px[0], px[0], px[0]});
        }
    }
    bool isMappoint(int idx) { return inliers_to_mappt_connections_.find(idx) != inliers_to_mappt_connections_.end(); }

};

}  // namespace vo
}  // namespace my_slam
#endif
