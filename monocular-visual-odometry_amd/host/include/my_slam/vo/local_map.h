// my_slam/vo/local_map.h -- tracking the local map: the second search of a tracked frame.  The reference's per-frame step ends
// with the pose of poseEstimationPnP_ (vo.cpp:267-347); ORB-SLAM, whose TrackWithMotionModel the steps before this one follow
// (my_slam/vo/projection_match.h, my_slam/vo/pose_optimization.h), goes on with Tracking::TrackLocalMap: with the optimised pose it
// projects every local map point the first search left unmatched (SearchLocalPoints, Frame::isInFrustum,
// ORBmatcher::SearchByProjection(F, vpMapPoints, th)) and optimises the pose again over the union.  Executed by libmvo_hip.so
// through the hot-path context of the calling thread (mvo_map_upload_view, mvo_map_match_features_local, mvo_optimize_pose,
// include/mvo_hip.h; declared arithmetic: DESIGN.md sections 22 and 21).
//   trackLocalMap   the map and its view data (mean normal, max_dist_) synced; skip = the points connected in
//                   curr->inliers_to_mappt_connections_, t_level = the keypoints' octaves, -2 for a connected keypoint; the search
//                   with curr->T_w_c_, the optimised pose, and level_scale[l] = scale_factor multiplied l times; then, if there are
//                   new matches and the first pass's inlier matches plus the new ones are at most 4096, mvo_optimize_pose from
//                   curr->T_w_c_ over the first pass's inlier matches in their order followed by the new ones in trainIdx order,
//                   weighted as optimizePoseFromMatches weights them.  On status 0 with the new pose within
//                   max_possible_dist_to_prev_keyframe of prev: the pose is replaced, every new match that is not flagged gets
//                   its connection and matched_times_++, every first-pass connection that is now flagged is erased (with its
//                   match in matches_with_map_), as ORB-SLAM drops its mvbOutlier points.  visible_times_ is not touched:
//                   matchMapByProjection has counted the points in view.  On any other outcome the frame keeps what the first
//                   pass gave.
// trackFrame (tracking_loop.h) calls it after poseEstimationPnP and before callBundleAdjustment when the optional key
// `tracking_local_map` is 1 (default 0: nothing is called, nothing changes), the frame is good and its pose came from the
// optimisation (pose_opt_fallback_ == 0).  The key requires `tracking_pose_by_optimization: 1`.  Optional keys
// `local_map_min_view_cos` (default 0.5), `local_map_radius_near` (2.5), `local_map_radius_far` (4.0), `local_map_radius_scale`
// (1.0), `local_map_lowe_ratio` (0.8), `local_map_max_hamming` (100).
#ifndef MY_SLAM_LOCAL_MAP_H
#define MY_SLAM_LOCAL_MAP_H
#include <algorithm>
#include <unordered_map>

#include "my_slam/vo/tracking_loop.h"

// Bound weakly: a program that includes this header still links and runs against a build of the library without the second
// search; calling trackLocalMap with such a library is an error, not a fall-back.
#pragma weak mvo_map_upload_view
#pragma weak mvo_map_match_features_local

namespace my_slam {
namespace vo {

constexpr int kLocalMapMaxObservations = 4096;  // of mvo_optimize_pose

inline mvo_local_map_params localMapParams() {  // the optional keys, latched on first use
    static const mvo_local_map_params p = [] {
        mvo_local_map_params q{0.5, 2.5, 4.0, 0.998, 1.0, 0.8, 100, 0};
        auto real = [](const char* key, double& v) {
            if (basics::Config::has(key)) v = basics::Config::get<double>(key);
        };
        real("local_map_min_view_cos", q.min_view_cos);
        real("local_map_radius_near", q.radius_near);
        real("local_map_radius_far", q.radius_far);
        real("local_map_radius_scale", q.radius_scale);
        real("local_map_lowe_ratio", q.lowe_ratio);
        if (basics::Config::has("local_map_max_hamming")) q.max_hamming = basics::Config::get<int>("local_map_max_hamming");
        return q;
    }();
    return p;
}

// the outcomes of the pass (Frame::local_map_outcome_)
enum LocalMapOutcome { kLocalMapNoNewMatches = 0, kLocalMapTooManyObservations = 1, kLocalMapNotOptimised = 2, kLocalMapMovedTooFar = 3,
                       kLocalMapApplied = 4 };

inline void trackLocalMap(TrackingState& st, const Frame::Ptr& curr, const cv::Mat& K) {
    if (!mvo_map_upload_view || !mvo_map_match_features_local)
        throw std::runtime_error("trackLocalMap: this libmvo_hip.so has no mvo_map_match_features_local");
    if (!mvo_optimize_pose) throw std::runtime_error("trackLocalMap: this libmvo_hip.so has no mvo_optimize_pose");
    static const int n_levels = basics::Config::get<int>("level_pyramid");
    static const double max_possible_dist_to_prev_keyframe = basics::Config::get<double>("max_possible_dist_to_prev_keyframe");
    const mvo_local_map_params params = localMapParams();
    // 1. the map and its view data
    MapOnDevice& dev_map = st.dev_map_;
    dev_map.syncView(st.map_);
    const vector<MapPoint::Ptr>& order = dev_map.order();
    const int m = (int)order.size(), nt = (int)curr->keypoints_.size();
    if (curr->descriptors_.rows != nt || (nt && curr->descriptors_.cols != 32))
        throw std::runtime_error("trackLocalMap: one 32-byte descriptor per keypoint is required");
    vector<unsigned char> pack;  // rows of 32 bytes back to back (a descriptor matrix with padded rows is packed first)
    const unsigned char* desc = nt ? curr->descriptors_.data : nullptr;
    if (nt && (int)curr->descriptors_.step != 32) {
        pack.resize((size_t)nt * 32);
        for (int r = 0; r < nt; ++r) std::memcpy(&pack[(size_t)r * 32], curr->descriptors_.ptr<unsigned char>(r), 32);
        desc = pack.data();
    }
    // 2. the masks
    std::unordered_map<int, int> row_of_id;
    for (int i = 0; i < m; ++i) row_of_id[order[i]->id_] = i;
    vector<unsigned char> skip(m > 0 ? m : 1, 0);
    vector<float> txy(2 * (size_t)nt);
    vector<int> t_level(nt);
    for (int j = 0; j < nt; ++j) {
        txy[2 * j] = curr->keypoints_[j].pt.x, txy[2 * j + 1] = curr->keypoints_[j].pt.y;
        t_level[j] = curr->keypoints_[j].octave;
    }
    for (const auto& kv : curr->inliers_to_mappt_connections_) {
        if (kv.first >= 0 && kv.first < nt) t_level[kv.first] = -2;
        const auto it = row_of_id.find(kv.second.pt_map_idx);
        if (it != row_of_id.end()) skip[it->second] = 1;
    }
    // 3. the search from the optimised pose
    vector<double> level_scale(n_levels);
    for (int l = 0; l < n_levels; ++l) level_scale[l] = octaveScale(l);
    vector<double> T0(16);
    for (int i = 0; i < 16; ++i) T0[i] = curr->T_w_c_.at<double>(i / 4, i % 4);
    const double fx = K.at<double>(0, 0), fy = K.at<double>(1, 1), cx = K.at<double>(0, 2), cy = K.at<double>(1, 2);
    const int cols = curr->rgb_img_.cols, rows = curr->rgb_img_.rows;
    vector<mvo_dmatch> found(std::max(1, std::min(m, nt)));
    int n_new = 0;
    mvo_check(mvo_map_match_features_local(hot_path_ctx(), dev_map.handle(), T0.data(), fx, fy, cx, cy, cols, rows, desc,
                                           nt ? txy.data() : nullptr, nt ? t_level.data() : nullptr, nt, skip.data(), level_scale.data(),
                                           n_levels, &params, nullptr, nullptr, found.data(), (int)found.size(), &n_new),
              "trackLocalMap");
    found.resize(n_new);
    skip.resize(m);
    // what the call saw and gave, for the frame log (bundle adjustment rewrites poses and positions in place afterwards)
    curr->local_map_setup_ = {fx, fy, cx, cy, (double)cols, (double)rows, (double)n_levels, params.min_view_cos, params.radius_near,
                              params.radius_far, params.near_cos, params.radius_scale, params.lowe_ratio, (double)params.max_hamming};
    curr->local_map_setup_.insert(curr->local_map_setup_.end(), level_scale.begin(), level_scale.end());
    curr->local_map_init_ = T0;
    curr->local_map_skip_ = skip;
    curr->local_map_t_level_ = t_level;
    curr->local_map_pos_ = dev_map.positions();
    curr->local_map_desc_ = dev_map.descriptors();
    curr->local_map_normal_ = dev_map.normals();
    curr->local_map_max_dist_ = dev_map.maxDists();
    curr->local_map_matches_.clear();
    for (const mvo_dmatch& d : found) curr->local_map_matches_.push_back(cv::DMatch(d.queryIdx, d.trainIdx, d.imgIdx, d.distance));
    curr->local_map_p3_.clear(), curr->local_map_p2_.clear(), curr->local_map_sigma_.clear();
    curr->local_map_T_w_c_.clear(), curr->local_map_info_.clear(), curr->local_map_chi2_.clear(), curr->local_map_outlier_.clear();
    curr->local_map_applied_ = 0;
    // 4. no new matches: nothing changes
    if (n_new == 0) {
        curr->local_map_outcome_ = kLocalMapNoNewMatches;
        return;
    }
    // 5. more observations than the optimisation takes: the pass is skipped
    const int n_first = (int)curr->matches_with_map_.size(), n = n_first + n_new;
    if (n > kLocalMapMaxObservations) {
        curr->local_map_outcome_ = kLocalMapTooManyObservations;
        return;
    }
    // 6. the pose again, over the first pass's inlier matches in their order, then the new matches in trainIdx order
    vector<MapPoint::Ptr> point(n);
    vector<int> keypoint(n);
    for (int i = 0; i < n_first; ++i) {
        keypoint[i] = curr->matches_with_map_[i].trainIdx;
        const auto conn = curr->inliers_to_mappt_connections_.find(keypoint[i]);
        const auto it = conn == curr->inliers_to_mappt_connections_.end() ? row_of_id.end() : row_of_id.find(conn->second.pt_map_idx);
        if (it == row_of_id.end()) throw std::runtime_error("trackLocalMap: an inlier match of the first pass has no connected map point");
        point[i] = order[it->second];
    }
    for (int i = 0; i < n_new; ++i) {
        keypoint[n_first + i] = found[i].trainIdx;
        point[n_first + i] = order[found[i].queryIdx];
    }
    vector<float> p3(3 * (size_t)n), p2(2 * (size_t)n), sigma(n);
    for (int i = 0; i < n; ++i) {
        p3[3 * i] = point[i]->pos_.x, p3[3 * i + 1] = point[i]->pos_.y, p3[3 * i + 2] = point[i]->pos_.z;
        p2[2 * i] = curr->keypoints_[keypoint[i]].pt.x, p2[2 * i + 1] = curr->keypoints_[keypoint[i]].pt.y;
        const float scale = (float)octaveScale(curr->keypoints_[keypoint[i]].octave);  // (as optimizePoseFromMatches weights)
        sigma[i] = (float)(1.0 / ((double)scale * (double)scale));
    }
    vector<double> Twc(16), chi2(2);
    vector<int> info(6);
    vector<unsigned char> outlier(n);
    const mvo_pose_optimize_params opt = poseOptimizationParams();
    mvo_check(mvo_optimize_pose(hot_path_ctx(), p3.data(), p2.data(), sigma.data(), n, T0.data(), fx, fy, cx, cy, &opt, Twc.data(), nullptr,
                                outlier.data(), chi2.data(), info.data()),
              "trackLocalMap");
    curr->local_map_p3_ = p3, curr->local_map_p2_ = p2, curr->local_map_sigma_ = sigma;
    curr->local_map_T_w_c_ = Twc, curr->local_map_info_ = info, curr->local_map_chi2_ = chi2, curr->local_map_outlier_ = outlier;
    // 7. applied only if it optimised and the new pose is still a possible one
    if (info[0] != 0) {
        curr->local_map_outcome_ = kLocalMapNotOptimised;
        return;
    }
    double d2 = 0;  // (the test of poseEstimationPnP)
    for (int i = 0; i < 3; ++i) {
        const double d = Twc[4 * i + 3] - st.prev_->T_w_c_.at<double>(i, 3);
        d2 += d * d;
    }
    if (std::sqrt(d2) >= max_possible_dist_to_prev_keyframe) {
        curr->local_map_outcome_ = kLocalMapMovedTooFar;
        return;
    }
    for (int i = 0; i < 16; ++i) curr->T_w_c_.at<double>(i / 4, i % 4) = Twc[i];
    vector<cv::DMatch> kept;
    for (int i = 0; i < n_first; ++i) {
        if (outlier[i])
            curr->inliers_to_mappt_connections_.erase(keypoint[i]);
        else
            kept.push_back(curr->matches_with_map_[i]);
    }
    curr->matches_with_map_.swap(kept);
    for (int i = n_first; i < n; ++i) {
        if (outlier[i]) continue;
        point[i]->matched_times_++;
        curr->inliers_to_mappt_connections_[keypoint[i]] = PtConn{-1, point[i]->id_};
    }
    curr->local_map_applied_ = 1;
    curr->local_map_outcome_ = kLocalMapApplied;
}

}  // namespace vo
}  // namespace my_slam
#endif
