// my_slam/vo/projection_match.h -- tracking by projection: pose-guided matching for the step that runs on every frame,
// poseEstimationPnP_ (vo.cpp:267-289).  The reference projects the map with the pose of the last keyframe
// (vo_addFrame.cpp:74) and searches without a prediction; its README.md:212 names the remedy ("doing guided matching based on
// the estimated camera motion") and has no function for it.  Executed by libmvo_hip.so through the hot-path context of the
// calling thread (mvo_predict_pose, mvo_map_match_features_projection, include/mvo_hip.h; declared arithmetic: DESIGN.md
// section 15).
//   predictPose            T_prev * (inv(T_prev2) * T_prev): the constant-velocity prediction; an empty prev2 gives T_prev
//   matchMapByProjection   the resident map projected with curr->T_w_c_ and matched against curr's keypoints in one launch:
//                          fills the candidate lists with ALL points in view, in map order (visible_times_++ on each, as
//                          getMappointsInCurrentView does), and `matches` with queryIdx -> index into that candidate list,
//                          trainIdx -> curr->keypoints_; so the rest of poseEstimationPnP runs unchanged
// poseEstimationPnP (pnp_tracking.h) and trackFrame (tracking_loop.h) use them when the optional key
// `tracking_match_by_projection` is 1 (default 0: unchanged).  Optional parameters, latched on first use:
// projection_match_max_pixel_dist (px at pyramid level 0, default 8.0; a keypoint of octave o gets scale_factor^o times as
// much), projection_match_lowe_ratio (default 0.8), projection_match_max_hamming (default 64).
#ifndef MY_SLAM_PROJECTION_MATCH_H
#define MY_SLAM_PROJECTION_MATCH_H
#include <algorithm>

#include "my_slam/vo/pnp_tracking.h"

// Bound weakly: a program that includes this header still links and runs against a build of the library without tracking by
// projection; calling one of the two functions with such a library is an error, not a fall-back.
#pragma weak mvo_predict_pose
#pragma weak mvo_map_match_features_projection

namespace my_slam {
namespace vo {

inline cv::Mat predictPose(const cv::Mat& T_w_c_prev2, const cv::Mat& T_w_c_prev) {
    if (!mvo_predict_pose) throw std::runtime_error("predictPose: this libmvo_hip.so has no mvo_predict_pose");
    double T2[16], T1[16];
    for (int i = 0; i < 16; ++i) {
        T1[i] = T_w_c_prev.at<double>(i / 4, i % 4);
        if (!T_w_c_prev2.empty()) T2[i] = T_w_c_prev2.at<double>(i / 4, i % 4);
    }
    cv::Mat T(4, 4, CV_64FC1);
    if (mvo_predict_pose(T_w_c_prev2.empty() ? nullptr : T2, T1, T.ptr<double>(0)) != MVO_OK)
        throw std::runtime_error("predictPose: singular pose matrix");
    return T;
}

inline void matchMapByProjection(MapOnDevice& dev_map, const Map::Ptr& map, const Frame::Ptr& curr, const cv::Mat& K,
                                 vector<MapPoint::Ptr>& candidate_mappoints_in_map, vector<cv::Point2f>& candidate_2d_pts_in_image,
                                 vector<cv::DMatch>& matches) {
    if (!mvo_map_match_features_projection)
        throw std::runtime_error("matchMapByProjection: this libmvo_hip.so has no mvo_map_match_features_projection");
    static const double max_pixel_dist =
        basics::Config::has("projection_match_max_pixel_dist") ? basics::Config::get<double>("projection_match_max_pixel_dist") : 8.0;
    static const double lowe_ratio =
        basics::Config::has("projection_match_lowe_ratio") ? basics::Config::get<double>("projection_match_lowe_ratio") : 0.8;
    static const int max_hamming =
        basics::Config::has("projection_match_max_hamming") ? basics::Config::get<int>("projection_match_max_hamming") : 64;
    static const double scale_factor = basics::Config::get<double>("scale_factor");
    candidate_mappoints_in_map.clear();
    matches.clear();
    dev_map.sync(map);
    const int m = (int)dev_map.order().size(), nt = (int)curr->keypoints_.size();
    if (curr->descriptors_.rows != nt || (nt && curr->descriptors_.cols != 32))
        throw std::runtime_error("matchMapByProjection: one 32-byte descriptor per keypoint is required");
    vector<unsigned char> pack;  // rows of 32 bytes back to back (a descriptor matrix with padded rows is packed first)
    const unsigned char* desc = nt ? curr->descriptors_.data : nullptr;
    if (nt && (int)curr->descriptors_.step != 32) {
        pack.resize((size_t)nt * 32);
        for (int r = 0; r < nt; ++r) std::memcpy(&pack[(size_t)r * 32], curr->descriptors_.ptr<unsigned char>(r), 32);
        desc = pack.data();
    }
    vector<float> txy(2 * (size_t)nt), scale(nt);
    for (int j = 0; j < nt; ++j) {
        txy[2 * j] = curr->keypoints_[j].pt.x, txy[2 * j + 1] = curr->keypoints_[j].pt.y;
        double s = 1.0;
        for (int o = 0; o < curr->keypoints_[j].octave; ++o) s *= scale_factor;
        scale[j] = (float)s;
    }
    double T[16];
    for (int i = 0; i < 16; ++i) T[i] = curr->T_w_c_.at<double>(i / 4, i % 4);
    vector<cv::Point2f> px(m > 0 ? m : 1);
    vector<unsigned char> in_view(m > 0 ? m : 1);
    vector<mvo_dmatch> out(std::max(1, std::min(m, nt)));
    int n = 0;
    mvo_check(mvo_map_match_features_projection(hot_path_ctx(), dev_map.handle(), T, K.at<double>(0, 0), K.at<double>(1, 1),
                                                K.at<double>(0, 2), K.at<double>(1, 2), curr->rgb_img_.cols, curr->rgb_img_.rows, desc,
                                                nt ? txy.data() : nullptr, nt ? scale.data() : nullptr, nt, max_pixel_dist, lowe_ratio,
                                                max_hamming, &px[0].x, in_view.data(), out.data(), (int)out.size(), &n),
              "matchMapByProjection");
    vector<int> slot(m > 0 ? m : 1, -1);  // map index -> index into the candidate list
    for (int i = 0; i < m; ++i) {
        if (!in_view[i]) continue;
        slot[i] = (int)candidate_mappoints_in_map.size();
        const MapPoint::Ptr& p_world = dev_map.order()[i];
        candidate_mappoints_in_map.push_back(p_world);
        candidate_2d_pts_in_image.push_back(px[i]);  // (like getMappointsInCurrentView, which does not clear this vector either)
        p_world->visible_times_++;
    }
    for (int i = 0; i < n; ++i) matches.push_back(cv::DMatch(slot[out[i].queryIdx], out[i].trainIdx, out[i].imgIdx, out[i].distance));
    // what the matcher saw, for the frame log (bundle adjustment rewrites poses and positions in place afterwards)
    curr->projection_map_pos_ = dev_map.positions();
    curr->projection_map_desc_ = dev_map.descriptors();
    curr->projection_matches_ = matches;
}

}  // namespace vo
}  // namespace my_slam
#endif
