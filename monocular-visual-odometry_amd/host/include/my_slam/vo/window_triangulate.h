// my_slam/vo/window_triangulate.h -- new map points from every buffered frame.  The reference triangulates a new keyframe
// against its reference keyframe only (triangulateWithReferenceKeyframe, vo_addFrame.cpp:104-116; pushCurrPointsToMap_,
// vo.cpp:528-576): whether the pair yields anything is decided by the baseline between the two keyframes, and a keypoint without
// a partner there gets no map point although up to 19 other frames with wider baselines sit in frames_buff_.  ORB-SLAM's local
// mapping has LocalMapping::CreateNewMapPoints: every keypoint without a map point is searched along its epipolar line in every
// neighbouring keyframe, triangulated and verified.  Executed by libmvo_hip.so through the hot-path context of the calling thread
// (mvo_window_triangulate, include/mvo_hip.h; declared rule: DESIGN.md section 20).
//   createMapPointsFromWindow   curr = the newest frame of frames_buff_, the frames = the others, oldest first, as
//                       collectFuseFrames (map_fuse.h) makes them with the order of the resident map: a keypoint is free when it
//                       has no connection.  The call; then for every returned point a MapPoint as pushCurrPointsToMap makes one
//                       (world position preTranslatePoint3f(p_curr, curr->T_w_c_), descriptor and colour of curr's keypoint,
//                       normal from curr's centre), and two connections: curr's keypoint and the frame's keypoint name the new
//                       point (PtConn{-1, id}).
// trackFrame (tracking_loop.h) calls it right after pushCurrPointsToMap and before optimizeMap at every keyframe insertion when
// the optional key `map_point_create_from_window` is 1 (default 0: nothing is called, nothing changes): the new points pass the
// same culling, and the fusion, the refinement and the refresh, when their keys are on, work on them as on any other point.
// Optional keys `map_point_create_max_line_px` (default 2.0), `map_point_create_lowe_ratio` (0.8), `map_point_create_max_hamming`
// (64), `map_point_create_max_cos_parallax` (0.9998), `map_point_create_min_baseline` (0.0); ratio_factor = 1.5 scale_factor.
#ifndef MY_SLAM_WINDOW_TRIANGULATE_H
#define MY_SLAM_WINDOW_TRIANGULATE_H
#include "my_slam/vo/map_fuse.h"

// Bound weakly: a program that includes this header still links and runs against a build of the library without the step;
// calling createMapPointsFromWindow with such a library is an error, not a fall-back.
#pragma weak mvo_window_triangulate

namespace my_slam {
namespace vo {

inline mvo_window_triangulate_params mapPointCreateParams() {  // the optional keys, latched on first use
    static const mvo_window_triangulate_params p = [] {
        mvo_window_triangulate_params q{2.0, 0.8, 64, 0.9998, 5.991, 1.8, 0.0};
        if (basics::Config::has("map_point_create_max_line_px")) q.max_line_px = basics::Config::get<double>("map_point_create_max_line_px");
        if (basics::Config::has("map_point_create_lowe_ratio")) q.lowe_ratio = basics::Config::get<double>("map_point_create_lowe_ratio");
        if (basics::Config::has("map_point_create_max_hamming")) q.max_hamming = basics::Config::get<int>("map_point_create_max_hamming");
        if (basics::Config::has("map_point_create_max_cos_parallax"))
            q.max_cos_parallax = basics::Config::get<double>("map_point_create_max_cos_parallax");
        if (basics::Config::has("map_point_create_min_baseline")) q.min_baseline = basics::Config::get<double>("map_point_create_min_baseline");
        q.ratio_factor = 1.5 * basics::Config::get<double>("scale_factor");
        return q;
    }();
    return p;
}

// `curr` (may be null; trackFrame passes the keyframe, which is the newest frame) receives what the call saw and gave, for the frame log
inline void createMapPointsFromWindow(TrackingState& st, const cv::Mat& K, const Frame::Ptr& curr) {
    if (!mvo_window_triangulate) throw std::runtime_error("createMapPointsFromWindow: this libmvo_hip.so has no mvo_window_triangulate");
    if (st.frames_buff_.empty()) return;
    const Frame::Ptr& newest = st.frames_buff_.back();
    const FuseFrames ff = collectFuseFrames(st.frames_buff_, st.dev_map_.order());
    const int n_frames = (int)st.frames_buff_.size() - 1, n_curr = ff.n.back();
    const mvo_window_triangulate_params params = mapPointCreateParams();
    const double fx = K.at<double>(0, 0), fy = K.at<double>(1, 1), cx = K.at<double>(0, 2), cy = K.at<double>(1, 2);
    size_t cap_pairs = 1;
    for (int f = 0; f < n_frames; ++f) cap_pairs += (size_t)ff.n[f];
    vector<mvo_window_point> points(n_curr > 0 ? n_curr : 1);
    vector<mvo_window_pair> pairs(cap_pairs);
    vector<int> counts(12);
    int n_points = 0, n_pairs = 0;
    mvo_check(mvo_window_triangulate(hot_path_ctx(), &ff.rows.back(), n_frames ? ff.rows.data() : nullptr, n_frames, fx, fy, cx, cy, &params,
                                     points.data(), (int)points.size(), &n_points, pairs.data(), (int)pairs.size(), &n_pairs, counts.data()),
              "createMapPointsFromWindow");
    points.resize(n_points), pairs.resize(n_pairs);
    const int size_before = (int)st.map_->map_points_.size();
    vector<int> ids;
    vector<float> world;
    for (const mvo_window_point& w : points) {
        const cv::Point3f world_pos = preTranslatePoint3f(cv::Point3f(w.p_curr[0], w.p_curr[1], w.p_curr[2]), newest->T_w_c_);
        cv::Mat desc(1, 32, CV_8UC1), norm(3, 1, CV_64FC1);
        std::memcpy(desc.data, newest->descriptors_.ptr<unsigned char>(w.keypoint), 32);
        double len = 0;
        const double p[3] = {world_pos.x, world_pos.y, world_pos.z};
        for (int r = 0; r < 3; ++r) {
            norm.at<double>(r, 0) = p[r] - newest->T_w_c_.at<double>(r, 3);
            len += norm.at<double>(r, 0) * norm.at<double>(r, 0);
        }
        len = std::sqrt(len);
        for (int r = 0; r < 3; ++r) norm.at<double>(r, 0) /= len;
        const vector<unsigned char> rgb = w.keypoint < (int)newest->kpts_colors_.size() ? newest->kpts_colors_[w.keypoint]
                                                                                      : vector<unsigned char>{0, 0, 0};
        MapPoint::Ptr map_point(new MapPoint(world_pos, desc, norm, rgb[0], rgb[1], rgb[2]));
        if (trackingLocalMap()) map_point->max_dist_ = (float)(len * octaveScale(newest->keypoints_[w.keypoint].octave));
        st.map_->insertMapPoint(map_point);
        newest->inliers_to_mappt_connections_.insert({w.keypoint, PtConn{-1, map_point->id_}});
        st.frames_buff_[w.frame]->inliers_to_mappt_connections_.insert({w.train, PtConn{-1, map_point->id_}});
        ids.push_back(map_point->id_);
        world.push_back(world_pos.x), world.push_back(world_pos.y), world.push_back(world_pos.z);
    }
    if (curr) {
        curr->window_created_ = true;
        curr->window_setup_ = {fx, fy, cx, cy, params.max_line_px, params.lowe_ratio, (double)params.max_hamming, params.max_cos_parallax,
                              params.max_reproj_chi2, params.ratio_factor, params.min_baseline};
        curr->window_kp_count_ = ff.n;
        curr->window_T_w_c_ = ff.T_w_c;
        curr->window_desc_ = ff.desc;
        curr->window_xy_ = ff.xy;
        curr->window_scale_ = ff.scale;
        curr->window_conn_ = ff.conn;
        curr->window_points_.clear(), curr->window_points_p_.clear(), curr->window_points_cos2_.clear();
        for (const mvo_window_point& w : points) {
            for (int v : {w.keypoint, w.frame, w.train, w.hamming}) curr->window_points_.push_back(v);
            curr->window_points_p_.insert(curr->window_points_p_.end(), w.p_curr, w.p_curr + 3);
            curr->window_points_cos2_.push_back(w.cos2);
        }
        curr->window_pairs_.clear(), curr->window_pairs_p_.clear(), curr->window_pairs_cos2_.clear();
        for (const mvo_window_pair& w : pairs) {
            for (int v : {w.frame, w.keypoint, w.train, w.hamming, w.status}) curr->window_pairs_.push_back(v);
            curr->window_pairs_p_.insert(curr->window_pairs_p_.end(), w.p_curr, w.p_curr + 3);
            curr->window_pairs_p_.insert(curr->window_pairs_p_.end(), w.p_frame, w.p_frame + 3);
            curr->window_pairs_cos2_.push_back(w.cos2);
        }
        curr->window_counts_ = counts;
        curr->window_ids_ = ids;
        curr->window_world_ = world;
        curr->window_map_size_ = {size_before, (int)st.map_->map_points_.size()};
    }
}

}  // namespace vo
}  // namespace my_slam

#include "my_slam/vo/local_map.h"  // (declared in tracking_loop.h)
#endif
