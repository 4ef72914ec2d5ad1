// my_slam/vo/map_fuse.h -- duplicate map points fused, missed observations added.  The reference reuses a map point only when
// the matched keypoint of ref_ is one already and otherwise creates a new point (pushCurrPointsToMap_, vo.cpp:528-576), even
// when the keypoint of curr is connected to a map point through the PnP inliers: one physical point enters the map under
// several ids, each with part of the observations; and a buffered frame that sees a point without having matched it
// contributes nothing.  ORB-SLAM's local mapping answers both with SearchInNeighbors: ORBmatcher::Fuse projects every map point
// into every neighbouring keyframe, MapPoint::Replace merges two points that claim one keypoint.  Executed by libmvo_hip.so
// through the hot-path context of the calling thread (mvo_map_fuse, include/mvo_hip.h; declared rule: DESIGN.md section 19).
//   collectFuseFrames   one mvo_fuse_frame per frame of frames_buff_, oldest first: descriptors_, keypoints_[k].pt, the scale
//                       projection_match.h passes (scale_factor^octave), T_w_c_ as it stands, and per keypoint the row of the
//                       map point inliers_to_mappt_connections_ names (-1 without a connection, -2 when the id is no longer
//                       in the map)
//   fuseMapPoints       dev_map_.sync(map_); the call; then for every replaced point r -> s: every connection in frames_buff_
//                       with r's id takes s's id, s gains r's matched_times_ and visible_times_, r leaves map_->map_points_;
//                       every added observation becomes inliers_to_mappt_connections_.insert({keypoint, PtConn{-1, id(s)}});
//                       dev_map_ follows
// trackFrame (tracking_loop.h) calls it after optimizeMap and before refineMapPointPositions and refreshMapPoints at every
// keyframe insertion when the optional key `map_point_fuse` is 1 (default 0: nothing is called, nothing changes).  Optional keys
// `map_point_fuse_max_px` (default 3.0) and `map_point_fuse_max_hamming` (default 50).
#ifndef MY_SLAM_MAP_FUSE_H
#define MY_SLAM_MAP_FUSE_H
#include <unordered_map>

#include "my_slam/vo/map_refresh.h"

// Bound weakly: a program that includes this header still links and runs against a build of the library without the fusion;
// calling fuseMapPoints with such a library is an error, not a fall-back.
#pragma weak mvo_map_fuse

namespace my_slam {
namespace vo {

inline mvo_map_fuse_params mapPointFuseParams() {  // the optional keys, latched on first use
    static const mvo_map_fuse_params p = [] {
        mvo_map_fuse_params q{3.0, 50};
        if (basics::Config::has("map_point_fuse_max_px")) q.max_px = basics::Config::get<double>("map_point_fuse_max_px");
        if (basics::Config::has("map_point_fuse_max_hamming")) q.max_hamming = basics::Config::get<int>("map_point_fuse_max_hamming");
        return q;
    }();
    return p;
}

struct FuseFrames {  // the arrays the mvo_fuse_frame rows point into, frame after frame
    vector<int> n;   // keypoints per frame
    vector<double> T_w_c;
    vector<unsigned char> desc;
    vector<float> xy, scale;
    vector<int> conn;
    vector<mvo_fuse_frame> rows;
};

inline FuseFrames collectFuseFrames(const std::deque<Frame::Ptr>& frames_buff, const vector<MapPoint::Ptr>& order) {
    static const double scale_factor = basics::Config::get<double>("scale_factor");
    std::unordered_map<int, int> row_of_id;  // MapPoint::id_ -> position in `order`
    for (int i = 0; i < (int)order.size(); ++i) row_of_id[order[i]->id_] = i;
    FuseFrames ff;
    for (const Frame::Ptr& fr : frames_buff) {
        const int nk = (int)fr->keypoints_.size();
        if (fr->descriptors_.rows != nk || (nk && fr->descriptors_.cols != 32))
            throw std::runtime_error("collectFuseFrames: one 32-byte descriptor per keypoint is required");
        ff.n.push_back(nk);
        for (int i = 0; i < 16; ++i) ff.T_w_c.push_back(fr->T_w_c_.at<double>(i / 4, i % 4));
        for (int j = 0; j < nk; ++j) {
            const unsigned char* d = fr->descriptors_.ptr<unsigned char>(j);
            ff.desc.insert(ff.desc.end(), d, d + 32);
            ff.xy.push_back(fr->keypoints_[j].pt.x);
            ff.xy.push_back(fr->keypoints_[j].pt.y);
            double s = 1.0;
            for (int o = 0; o < fr->keypoints_[j].octave; ++o) s *= scale_factor;
            ff.scale.push_back((float)s);
            const auto c = fr->inliers_to_mappt_connections_.find(j);
            if (c == fr->inliers_to_mappt_connections_.end()) {
                ff.conn.push_back(-1);
            } else {
                const auto it = row_of_id.find(c->second.pt_map_idx);
                ff.conn.push_back(it == row_of_id.end() ? -2 : it->second);
            }
        }
    }
    size_t first = 0;
    for (size_t f = 0; f < ff.n.size(); ++f) {
        mvo_fuse_frame row;
        row.desc = ff.desc.data() + 32 * first, row.xy = ff.xy.data() + 2 * first;
        row.scale = ff.scale.data() + first, row.conn = ff.conn.data() + first;
        row.n = ff.n[f];
        std::memcpy(row.T_w_c, &ff.T_w_c[16 * f], sizeof row.T_w_c);
        ff.rows.push_back(row);
        first += (size_t)ff.n[f];
    }
    return ff;
}

// `curr` (may be null) receives what the call saw and gave, for the frame log
inline void fuseMapPoints(TrackingState& st, const cv::Mat& K, const Frame::Ptr& curr) {
    if (!mvo_map_fuse) throw std::runtime_error("fuseMapPoints: this libmvo_hip.so has no mvo_map_fuse");
    vector<int> order_before;
    for (const MapPoint::Ptr& p : st.dev_map_.order()) order_before.push_back(p->id_);
    st.dev_map_.sync(st.map_);
    const vector<MapPoint::Ptr> order = st.dev_map_.order();  // (a copy: the sync at the end rewrites it)
    const int n = (int)order.size(), n_frames = (int)st.frames_buff_.size();
    const FuseFrames ff = collectFuseFrames(st.frames_buff_, order);
    const mvo_map_fuse_params params = mapPointFuseParams();
    const double fx = K.at<double>(0, 0), fy = K.at<double>(1, 1), cx = K.at<double>(0, 2), cy = K.at<double>(1, 2);
    const Frame::Ptr& newest = st.frames_buff_.back();
    const int cols = newest->rgb_img_.cols, rows = newest->rgb_img_.rows;
    vector<int> replaced_by(n > 0 ? n : 1), counts(6);
    vector<mvo_fuse_observation> added(ff.conn.size() > 0 ? ff.conn.size() : 1);
    int n_added = 0;
    mvo_check(mvo_map_fuse(hot_path_ctx(), st.dev_map_.handle(), n_frames ? ff.rows.data() : nullptr, n_frames, fx, fy, cx, cy, cols, rows,
                           &params, replaced_by.data(), added.data(), (int)added.size(), &n_added, counts.data()),
              "fuseMapPoints");
    replaced_by.resize(n), added.resize(n_added);
    vector<int> map_ids, map_ids_after;
    for (const MapPoint::Ptr& p : order) map_ids.push_back(p->id_);
    std::unordered_map<int, int> new_id;  // id of a replaced point -> id of its survivor
    for (int i = 0; i < n; ++i) {
        if (replaced_by[i] == i) continue;
        const MapPoint::Ptr &r = order[i], &s = order[replaced_by[i]];
        new_id[r->id_] = s->id_;
        s->matched_times_ += r->matched_times_;
        s->visible_times_ += r->visible_times_;
        st.map_->map_points_.erase(r->id_);
    }
    if (!new_id.empty())
        for (const Frame::Ptr& fr : st.frames_buff_)
            for (auto& kv : fr->inliers_to_mappt_connections_) {
                const auto it = new_id.find(kv.second.pt_map_idx);
                if (it != new_id.end()) kv.second.pt_map_idx = it->second;
            }
    for (const mvo_fuse_observation& a : added)
        st.frames_buff_[a.frame]->inliers_to_mappt_connections_.insert({a.keypoint, PtConn{-1, order[a.point]->id_}});
    const vector<float> pos = st.dev_map_.positions();
    const vector<unsigned char> desc = st.dev_map_.descriptors();
    st.dev_map_.sync(st.map_);  // the replaced rows leave the resident map
    for (const MapPoint::Ptr& p : st.dev_map_.order()) map_ids_after.push_back(p->id_);
    if (curr) {
        curr->fused_ = true;
        curr->fuse_order_before_ = order_before;
        curr->fuse_setup_ = {fx, fy, cx, cy, (double)cols, (double)rows, params.max_px, (double)params.max_hamming};
        curr->fuse_map_ids_ = map_ids;
        curr->fuse_map_pos_ = pos;
        curr->fuse_map_desc_ = desc;
        curr->fuse_kp_count_ = ff.n;
        curr->fuse_T_w_c_ = ff.T_w_c;
        curr->fuse_desc_ = ff.desc;
        curr->fuse_xy_ = ff.xy;
        curr->fuse_scale_ = ff.scale;
        curr->fuse_conn_ = ff.conn;
        curr->fuse_replaced_by_ = replaced_by;
        curr->fuse_added_.clear();
        for (const mvo_fuse_observation& a : added) {
            curr->fuse_added_.push_back(a.frame);
            curr->fuse_added_.push_back(a.keypoint);
            curr->fuse_added_.push_back(a.point);
        }
        curr->fuse_counts_ = counts;
        curr->fuse_map_ids_after_ = map_ids_after;
    }
}

}  // namespace vo
}  // namespace my_slam

#include "my_slam/vo/window_triangulate.h"  // (declared in tracking_loop.h)
#endif
