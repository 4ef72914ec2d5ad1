// my_slam/vo/tracking_loop.h -- the DOING_TRACKING branch of VisualOdometry::addFrame (reference
// src/vo/vo_addFrame.cpp:70-124) composed from the mirrored hot-path pieces, plus the three small members it calls
// (checkLargeMoveForAddKeyFrame_ vo.cpp:247-266, pushCurrPointsToMap_ vo.cpp:528-576, optimizeMap_ vo.cpp:488-526).
// It exists so that the rows can be exercised TOGETHER the way the reference chains them (tests/); the initialisation
// branch is my_slam/vo/initialization.h, the state machine around both my_slam/vo/vo.h.  The display of the reference
// is not part of this repository.
#ifndef MY_SLAM_TRACKING_LOOP_H
#define MY_SLAM_TRACKING_LOOP_H
#include <deque>

#include "my_slam/vo/ba_window.h"
#include "my_slam/vo/keyframe.h"
#include "my_slam/vo/pnp_tracking.h"

namespace my_slam {
namespace vo {

struct TrackingState {  // the members of VisualOdometry the tracking branch touches (vo.h:58-77)
    Map::Ptr map_{new Map()};
    MapOnDevice dev_map_;
    std::deque<Frame::Ptr> frames_buff_;
    Frame::Ptr ref_, prev_;
    Frame::Ptr prev2_;  // the frame before prev_ (`tracking_match_by_projection: 1`: the constant-velocity prediction)
    double map_point_erase_ratio_ = 0.1;  // the function-local static of optimizeMap_
    static constexpr size_t kBuffSize_ = 20;
    void pushFrameToBuff(Frame::Ptr frame) {
        frames_buff_.push_back(frame);
        if (frames_buff_.size() > kBuffSize_) frames_buff_.pop_front();
    }
};

// my_slam/vo/map_refresh.h (included at the end of this header): the refresh of `map_point_refresh: 1`
inline void refreshMapPoints(TrackingState& st, const Frame::Ptr& curr = nullptr);
inline bool mapPointRefresh() {  // the optional key, latched on first use
    static const bool on = basics::Config::has("map_point_refresh") && basics::Config::get<int>("map_point_refresh") != 0;
    return on;
}

// my_slam/vo/map_refine.h (included at the end of map_refresh.h, whose traversal it shares): the position refinement of `map_point_refine_positions: 1`
inline void refineMapPointPositions(TrackingState& st, const cv::Mat& K, const Frame::Ptr& curr = nullptr);
inline bool mapPointRefinePositions() {  // the optional key, latched on first use
    static const bool on =
        basics::Config::has("map_point_refine_positions") && basics::Config::get<int>("map_point_refine_positions") != 0;
    return on;
}

// my_slam/vo/map_fuse.h (included at the end of map_refine.h): the fusion of duplicate map points of `map_point_fuse: 1`
inline void fuseMapPoints(TrackingState& st, const cv::Mat& K, const Frame::Ptr& curr = nullptr);
inline bool mapPointFuse() {  // the optional key, latched on first use
    static const bool on = basics::Config::has("map_point_fuse") && basics::Config::get<int>("map_point_fuse") != 0;
    return on;
}

// my_slam/vo/window_triangulate.h (included at the end of map_fuse.h): the new map points of `map_point_create_from_window: 1`
inline void createMapPointsFromWindow(TrackingState& st, const cv::Mat& K, const Frame::Ptr& curr = nullptr);
inline bool mapPointCreateFromWindow() {  // the optional key, latched on first use
    static const bool on =
        basics::Config::has("map_point_create_from_window") && basics::Config::get<int>("map_point_create_from_window") != 0;
    return on;
}

// my_slam/vo/local_map.h (included at the end of window_triangulate.h): the second search of `tracking_local_map: 1`
inline void trackLocalMap(TrackingState& st, const Frame::Ptr& curr, const cv::Mat& K);
inline bool trackingLocalMap() {  // the optional key, latched on first use
    static const bool on = basics::Config::has("tracking_local_map") && basics::Config::get<int>("tracking_local_map") != 0;
    return on;
}

inline double octaveScale(int octave) {  // scale_factor multiplied octave times in f64, as matchMapByProjection does
    static const double scale_factor = basics::Config::get<double>("scale_factor");
    double s = 1.0;
    for (int o = 0; o < octave; ++o) s *= scale_factor;
    return s;
}

inline cv::Point3f preTranslatePoint3f(const cv::Point3f& p, const cv::Mat& T) {  // opencv_funcs.cpp:67-78
    const double q[4] = {p.x, p.y, p.z, 1};
    double res[3] = {0, 0, 0};
    for (int r = 0; r < 3; r++)
        for (int j = 0; j < 4; j++) res[r] += T.at<double>(r, j) * q[j];
    return cv::Point3f((float)res[0], (float)res[1], (float)res[2]);
}

inline bool isInFrame(const Frame::Ptr& f, const cv::Point3f& p_world, const cv::Mat& K) {  // frame.cpp:29-36
    const cv::Point3f pc = preTranslatePoint3f(p_world, basics::invT(f->T_w_c_));
    if (pc.z < 0) return false;
    const float u = (float)(K.at<double>(0, 0) * pc.x / pc.z + K.at<double>(0, 2));
    const float v = (float)(K.at<double>(1, 1) * pc.y / pc.z + K.at<double>(1, 2));
    return u > 0 && v > 0 && u < f->rgb_img_.cols && v < f->rgb_img_.rows;
}

inline bool checkLargeMoveForAddKeyFrame(const Frame::Ptr& curr, const Frame::Ptr& ref) {
    static const double min_dist_between_two_keyframes = basics::Config::get<double>("min_dist_between_two_keyframes");
    const cv::Mat T_key_to_curr = getMotionFromFrame1to2(ref, curr);  // ref->T_w_c_.inv() * curr->T_w_c_
    double s = 0;
    for (int i = 0; i < 3; ++i) s = s + T_key_to_curr.at<double>(i, 3) * T_key_to_curr.at<double>(i, 3);
    return std::sqrt(s) > min_dist_between_two_keyframes;
}

inline void pushCurrPointsToMap(TrackingState& st, const Frame::Ptr& curr) {
    for (size_t i = 0; i < curr->inliers_matches_for_3d_.size(); i++) {
        const cv::DMatch& dm = curr->inliers_matches_for_3d_[i];
        const int pt_idx = dm.trainIdx;
        int map_point_id;
        if (st.ref_->isMappoint(dm.queryIdx)) {
            map_point_id = st.ref_->inliers_to_mappt_connections_[dm.queryIdx].pt_map_idx;
        } else {
            const cv::Point3f world_pos = preTranslatePoint3f(curr->inliers_pts3d_[i], curr->T_w_c_);
            cv::Mat desc(1, 32, CV_8UC1), norm(3, 1, CV_64FC1);
            std::memcpy(desc.data, curr->descriptors_.ptr<unsigned char>(pt_idx), 32);
            double len = 0;
            const double w[3] = {world_pos.x, world_pos.y, world_pos.z};
            for (int r = 0; r < 3; ++r) {
                norm.at<double>(r, 0) = w[r] - curr->T_w_c_.at<double>(r, 3);
                len += norm.at<double>(r, 0) * norm.at<double>(r, 0);
            }
            len = std::sqrt(len);
            for (int r = 0; r < 3; ++r) norm.at<double>(r, 0) /= len;
            const vector<unsigned char> rgb = pt_idx < (int)curr->kpts_colors_.size() ? curr->kpts_colors_[pt_idx]
                                                                                       : vector<unsigned char>{0, 0, 0};
            MapPoint::Ptr map_point(new MapPoint(world_pos, desc, norm, rgb[0], rgb[1], rgb[2]));
            if (trackingLocalMap()) map_point->max_dist_ = (float)(len * octaveScale(curr->keypoints_[pt_idx].octave));
            map_point_id = map_point->id_;
            st.map_->insertMapPoint(map_point);
        }
        curr->inliers_to_mappt_connections_.insert({pt_idx, PtConn{dm.queryIdx, map_point_id}});
    }
}

inline void optimizeMap(TrackingState& st, const Frame::Ptr& curr, const cv::Mat& K) {
    const double default_erase = 0.1;
    for (auto iter = st.map_->map_points_.begin(); iter != st.map_->map_points_.end();) {
        const MapPoint::Ptr& p = iter->second;
        if (!isInFrame(curr, p->pos_, K)) {
            iter = st.map_->map_points_.erase(iter);
            continue;
        }
        const float match_ratio = float(p->matched_times_) / p->visible_times_;
        if (match_ratio < st.map_point_erase_ratio_) {
            iter = st.map_->map_points_.erase(iter);
            continue;
        }
        double n[3], len = 0, dot = 0;  // getViewAngle_ (vo.cpp:578-584)
        const double w[3] = {p->pos_.x, p->pos_.y, p->pos_.z};
        for (int r = 0; r < 3; ++r) {
            n[r] = w[r] - curr->T_w_c_.at<double>(r, 3);
            len += n[r] * n[r];
        }
        len = std::sqrt(len);
        for (int r = 0; r < 3; ++r) dot += n[r] / len * p->norm_.at<double>(r, 0);
        if (std::acos(dot) > M_PI / 4.) {
            iter = st.map_->map_points_.erase(iter);
            continue;
        }
        iter++;
    }
    if (st.map_->map_points_.size() > 1000)
        st.map_point_erase_ratio_ += 0.05;
    else
        st.map_point_erase_ratio_ = default_erase;
}

// One frame of the tracking state (vo_addFrame.cpp:9-27 + 70-140); curr must carry its image size, keypoints and
// descriptors (Frame::calcKeyPoints / calcDescriptors in the real pipeline).  Returns is_pnp_good; *is_keyframe
// tells whether the frame was inserted as a keyframe.
inline bool trackFrame(TrackingState& st, const Frame::Ptr& curr, const cv::Mat& K, bool* is_keyframe = nullptr) {
    st.pushFrameToBuff(curr);
    if (is_keyframe) *is_keyframe = false;
    if (!st.prev_) st.prev_ = st.ref_;
    if (trackingMatchByProjection()) {  // the pose predicted from the last two frames in place of the last keyframe's
        // (a prev2 with the very pose of prev -- a frame whose PnP failed takes its predecessor's -- is no motion: as without a
        // prev2 the prediction is T_prev itself, not T_prev * (inv(T_prev) * T_prev))
        cv::Mat prev2 = st.prev2_ ? st.prev2_->T_w_c_ : cv::Mat();
        if (!prev2.empty() && std::memcmp(prev2.ptr<double>(0), st.prev_->T_w_c_.ptr<double>(0), 16 * sizeof(double)) == 0) prev2 = cv::Mat();
        curr->T_w_c_ = predictPose(prev2, st.prev_->T_w_c_);
        curr->projection_prev_T_.clear();
        for (const cv::Mat& T : {prev2.empty() ? st.prev_->T_w_c_ : prev2, st.prev_->T_w_c_})
            for (int i = 0; i < 16; ++i) curr->projection_prev_T_.push_back(T.at<double>(i / 4, i % 4));
        curr->projection_pred_T_ = curr->T_w_c_.clone();
    } else {
        curr->T_w_c_ = st.ref_->T_w_c_.clone();  // Initial estimation of the current pose
    }
    const bool is_pnp_good = poseEstimationPnP(st.dev_map_, st.map_, curr, st.prev_, K);
    if (trackingLocalMap()) {
        if (!trackingPoseByOptimization()) throw std::runtime_error("tracking_local_map requires tracking_pose_by_optimization: 1");
        // ORB-SLAM's TrackLocalMap: the map points the first search left unmatched, searched from the optimised pose
        if (is_pnp_good && curr->pose_opt_fallback_ == 0) trackLocalMap(st, curr, K);
    }
    if (is_pnp_good) {
        callBundleAdjustment(st.frames_buff_, st.map_, K);
        if (checkLargeMoveForAddKeyFrame(curr, st.ref_)) {
            triangulateWithReferenceKeyframe(curr, st.ref_, K);
            pushCurrPointsToMap(st, curr);
            if (mapPointCreateFromWindow()) createMapPointsFromWindow(st, K, curr);  // ... and from every other buffered frame
            optimizeMap(st, curr, K);
            if (mapPointFuse()) fuseMapPoints(st, K, curr);  // one point per physical point, every observation in the window
            if (mapPointRefinePositions()) refineMapPointPositions(st, K, curr);  // positions from all observations, poses fixed
            if (mapPointRefresh()) refreshMapPoints(st, curr);  // descriptor and normal from all observations in the window
            st.map_->insertKeyFrame(curr);  // addKeyFrame_
            st.ref_ = curr;
            if (is_keyframe) *is_keyframe = true;
        }
    }
    if (st.prev_ != curr) st.prev2_ = st.prev_;
    st.prev_ = curr;
    return is_pnp_good;
}

}  // namespace vo
}  // namespace my_slam

#include "my_slam/vo/map_refresh.h"
#endif
