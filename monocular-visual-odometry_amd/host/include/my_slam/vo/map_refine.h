// my_slam/vo/map_refine.h -- map point positions refined from all their observations.  The reference sets a map point's position
// once, from two views (triangulation against ref_, stored by pushCurrPointsToMap_, vo.cpp:528-576), and its bundle adjustment
// runs with the points fixed (config.yaml:123, is_ba_fix_map_points: "true"): the BA moves poses against these positions and
// nothing corrects them.  This is the other half of that alternation, as ORB-SLAM's local mapping and g2o's structure-only
// solver do it: the poses fixed, every point an independent 3-unknown Huber-weighted least-squares problem over its
// observations in the 20-frame window.  Executed by libmvo_hip.so through the hot-path context of the calling thread
// (mvo_map_refine_positions, include/mvo_hip.h; declared arithmetic: DESIGN.md section 18).
//   refineMapPointPositions   dev_map_.sync(map_); the observations of collectObservations (my_slam/vo/map_refresh.h: the same
//                             traversal, the same order, the newest 64) as (position of the frame in frames_buff_,
//                             keypoints_[k].pt); the frames are those of frames_buff_ with T_w_c_ as it stands after the bundle
//                             adjustment; the call; then MapPoint::pos_ for every point with status 0, and MapOnDevice's host
//                             copy follows
// trackFrame (tracking_loop.h) calls it after optimizeMap and before refreshMapPoints at every keyframe insertion when the
// optional key `map_point_refine_positions` is 1 (default 0: nothing is called, nothing changes).  Optional keys
// `map_point_refine_max_trials` (default 20) and `map_point_refine_huber_delta` (default sqrt(5.991)).
#ifndef MY_SLAM_MAP_REFINE_H
#define MY_SLAM_MAP_REFINE_H
#include <cmath>

#include "my_slam/vo/map_refresh.h"

// Bound weakly: a program that includes this header still links and runs against a build of the library without the
// refinement; calling refineMapPointPositions with such a library is an error, not a fall-back.
#pragma weak mvo_map_refine_positions

namespace my_slam {
namespace vo {

inline mvo_map_refine_params mapPointRefineParams() {  // the optional keys, latched on first use
    static const mvo_map_refine_params p = [] {
        mvo_map_refine_params q{20, 2, std::sqrt(5.991), 1e-6};
        if (basics::Config::has("map_point_refine_max_trials")) q.max_trials = basics::Config::get<int>("map_point_refine_max_trials");
        if (basics::Config::has("map_point_refine_huber_delta")) q.huber_delta = basics::Config::get<double>("map_point_refine_huber_delta");
        return q;
    }();
    return p;
}

// `curr` (may be null) receives what the call saw and gave, for the frame log
inline void refineMapPointPositions(TrackingState& st, const cv::Mat& K, const Frame::Ptr& curr) {
    if (!mvo_map_refine_positions) throw std::runtime_error("refineMapPointPositions: this libmvo_hip.so has no mvo_map_refine_positions");
    vector<int> order_before;
    for (const MapPoint::Ptr& p : st.dev_map_.order()) order_before.push_back(p->id_);
    st.dev_map_.sync(st.map_);
    const vector<MapPoint::Ptr>& order = st.dev_map_.order();
    const int n = (int)order.size(), n_frames = (int)st.frames_buff_.size();
    const MapObservations o = collectObservations(st.frames_buff_, order);
    const int n_obs = o.obs_start.back();
    vector<double> T(16 * (size_t)n_frames);
    for (int f = 0; f < n_frames; ++f)
        for (int i = 0; i < 16; ++i) T[16 * (size_t)f + i] = st.frames_buff_[f]->T_w_c_.at<double>(i / 4, i % 4);
    const mvo_map_refine_params params = mapPointRefineParams();
    const double fx = K.at<double>(0, 0), fy = K.at<double>(1, 1), cx = K.at<double>(0, 2), cy = K.at<double>(1, 2);
    const vector<float> before = st.dev_map_.positions();
    vector<float> pos(3 * (size_t)(n > 0 ? n : 1));
    vector<double> chi2(2 * (size_t)(n > 0 ? n : 1));
    vector<int> info(3 * (size_t)(n > 0 ? n : 1));
    vector<unsigned char> outlier(n_obs > 0 ? n_obs : 1);
    mvo_check(mvo_map_refine_positions(hot_path_ctx(), st.dev_map_.handle(), n_frames ? T.data() : nullptr, n_frames, fx, fy, cx, cy,
                                       n_obs ? o.obs_frame.data() : nullptr, n_obs ? o.obs_uv.data() : nullptr, o.obs_start.data(), n_obs,
                                       &params, pos.data(), chi2.data(), info.data(), outlier.data()),
              "refineMapPointPositions");
    for (int i = 0; i < n; ++i) {
        if (info[3 * (size_t)i] != 0) continue;
        const float* p = &pos[3 * (size_t)i];
        order[i]->pos_ = cv::Point3f(p[0], p[1], p[2]);
        st.dev_map_.setPosition(i, p);
    }
    if (curr) {
        curr->positions_refined_ = true;
        curr->refine_order_before_ = order_before;
        curr->refine_setup_ = {fx, fy, cx, cy, (double)params.max_trials, (double)params.min_observations, params.huber_delta, params.rel_tolerance};
        curr->refine_T_w_c_ = T;
        curr->refine_obs_start_ = o.obs_start;
        curr->refine_obs_frame_ = o.obs_frame;
        curr->refine_obs_uv_ = o.obs_uv;
        curr->refine_pos_before_ = before;
        pos.resize(3 * (size_t)n), chi2.resize(2 * (size_t)n), info.resize(3 * (size_t)n), outlier.resize(n_obs);
        curr->refine_pos_after_ = pos;
        curr->refine_chi2_ = chi2;
        curr->refine_info_ = info;
        curr->refine_outlier_ = outlier;
    }
}

}  // namespace vo
}  // namespace my_slam

#include "my_slam/vo/map_fuse.h"  // (declared in tracking_loop.h)
#endif
