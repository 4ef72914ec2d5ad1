// my_slam/vo/map_refresh.h -- a map point as the summary of its observations.  The reference gives a map point the descriptor
// and the viewing direction of the one frame that created it (pushCurrPointsToMap_, vo.cpp:528-576) and never writes them again;
// ORB-SLAM, whose matching my_slam/geometry/epipolar_match.h and my_slam/vo/projection_match.h follow, recomputes both from all
// observations (MapPoint::ComputeDistinctiveDescriptors: the observation with the least median Hamming distance to the others;
// MapPoint::UpdateNormalAndDepth: the mean of the unit viewing directions).  Executed by libmvo_hip.so through the hot-path
// context of the calling thread (mvo_map_refresh, include/mvo_hip.h; declared arithmetic: DESIGN.md section 17).
//   collectObservations   for every point of MapOnDevice::order(): the (frame, keypoint) pairs of frames_buff_ whose
//                         inliers_to_mappt_connections_[keypoint].pt_map_idx is the point's id_, sorted by (position of the
//                         frame in the deque, oldest first; keypoint index); of more than 64 the newest 64 are kept.  The
//                         descriptor is the frame's descriptors_ row, the camera centre column 3 of its T_w_c_ as it stands
//   refreshMapPoints      dev_map_.sync(map_), mvo_map_refresh, then MapPoint::descriptor_ for every point with an observation
//                         and MapPoint::norm_ where the three components are finite; MapOnDevice's host copy follows
// trackFrame (tracking_loop.h) calls refreshMapPoints right after optimizeMap at every keyframe insertion when the optional key
// `map_point_refresh` is 1 (default 0: nothing is called, nothing changes).
#ifndef MY_SLAM_MAP_REFRESH_H
#define MY_SLAM_MAP_REFRESH_H
#include <algorithm>
#include <cmath>
#include <deque>
#include <unordered_map>

#include "my_slam/vo/tracking_loop.h"

// Bound weakly: a program that includes this header still links and runs against a build of the library without the refresh;
// calling refreshMapPoints with such a library is an error, not a fall-back.
#pragma weak mvo_map_refresh

namespace my_slam {
namespace vo {

struct MapObservations {  // the three input arrays of mvo_map_refresh
    vector<int> obs_start;           // n + 1
    vector<unsigned char> obs_desc;  // n_obs x 32
    vector<double> obs_cam;          // n_obs x 3
    // the same observations as mvo_map_refine_positions takes them (my_slam/vo/map_refine.h)
    vector<int> obs_frame;  // n_obs: position of the frame in frames_buff
    vector<float> obs_uv;   // n_obs x 2: keypoints_[k].pt
};

inline MapObservations collectObservations(const std::deque<Frame::Ptr>& frames_buff, const vector<MapPoint::Ptr>& order) {
    constexpr size_t kMaxObs = 64;
    const int n = (int)order.size();
    std::unordered_map<int, int> row_of_id;  // MapPoint::id_ -> position in `order`
    for (int i = 0; i < n; ++i) row_of_id[order[i]->id_] = i;
    struct Obs {
        int frame, kpt;
    };
    vector<vector<Obs>> per_point(n);
    for (int f = 0; f < (int)frames_buff.size(); ++f) {  // oldest first
        vector<std::pair<int, int>> conns;               // (keypoint, row): the connection map iterates in no order of its own
        for (const auto& kv : frames_buff[f]->inliers_to_mappt_connections_) {
            const auto it = row_of_id.find(kv.second.pt_map_idx);
            if (it != row_of_id.end()) conns.push_back({kv.first, it->second});
        }
        std::sort(conns.begin(), conns.end());
        for (const auto& c : conns) per_point[c.second].push_back(Obs{f, c.first});
    }
    MapObservations o;
    o.obs_start.push_back(0);
    for (int i = 0; i < n; ++i) {
        const vector<Obs>& v = per_point[i];
        for (size_t k = v.size() > kMaxObs ? v.size() - kMaxObs : 0; k < v.size(); ++k) {  // the newest 64
            const Frame::Ptr& fr = frames_buff[v[k].frame];
            if (v[k].kpt < 0 || v[k].kpt >= fr->descriptors_.rows || fr->descriptors_.cols != 32)
                throw std::runtime_error("collectObservations: a connection without its 32-byte descriptor row");
            const unsigned char* d = fr->descriptors_.ptr<unsigned char>(v[k].kpt);
            o.obs_desc.insert(o.obs_desc.end(), d, d + 32);
            for (int r = 0; r < 3; ++r) o.obs_cam.push_back(fr->T_w_c_.at<double>(r, 3));
            o.obs_frame.push_back(v[k].frame);
            const bool has_kpt = v[k].kpt < (int)fr->keypoints_.size();  // (a hand-built frame may carry descriptors only)
            o.obs_uv.push_back(has_kpt ? fr->keypoints_[v[k].kpt].pt.x : 0.f);
            o.obs_uv.push_back(has_kpt ? fr->keypoints_[v[k].kpt].pt.y : 0.f);
        }
        o.obs_start.push_back((int)(o.obs_desc.size() / 32));
    }
    return o;
}

// `curr` (may be null) receives what the refresh saw and gave, for the frame log
inline void refreshMapPoints(TrackingState& st, const Frame::Ptr& curr) {
    if (!mvo_map_refresh) throw std::runtime_error("refreshMapPoints: this libmvo_hip.so has no mvo_map_refresh");
    vector<int> order_before;
    for (const MapPoint::Ptr& p : st.dev_map_.order()) order_before.push_back(p->id_);
    st.dev_map_.sync(st.map_);
    const vector<MapPoint::Ptr>& order = st.dev_map_.order();
    const int n = (int)order.size();
    const MapObservations o = collectObservations(st.frames_buff_, order);
    const int n_obs = o.obs_start.back();
    vector<int> choice(n > 0 ? n : 1);
    vector<unsigned char> desc(32 * (size_t)(n > 0 ? n : 1));
    vector<double> norm(3 * (size_t)(n > 0 ? n : 1));
    mvo_check(mvo_map_refresh(hot_path_ctx(), st.dev_map_.handle(), n_obs ? o.obs_desc.data() : nullptr, n_obs ? o.obs_cam.data() : nullptr,
                              o.obs_start.data(), n_obs, choice.data(), desc.data(), norm.data()),
              "refreshMapPoints");
    for (int i = 0; i < n; ++i) {
        if (choice[i] < 0) continue;
        std::memcpy(order[i]->descriptor_.data, &desc[32 * (size_t)i], 32);
        st.dev_map_.setDescriptor(i, &desc[32 * (size_t)i]);
        const double* v = &norm[3 * (size_t)i];
        if (std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]))
            for (int r = 0; r < 3; ++r) order[i]->norm_.at<double>(r, 0) = v[r];
    }
    if (curr) {
        curr->refreshed_ = true;
        curr->refresh_order_before_ = order_before;
        curr->refresh_obs_start_ = o.obs_start;
        curr->refresh_obs_desc_ = o.obs_desc;
        curr->refresh_obs_cam_ = o.obs_cam;
        curr->refresh_pos_ = st.dev_map_.positions();
        choice.resize(n);
        norm.resize(3 * (size_t)n);
        curr->refresh_choice_ = choice;
        curr->refresh_norm_ = norm;
    }
}

}  // namespace vo
}  // namespace my_slam

#include "my_slam/vo/map_refine.h"  // (shares collectObservations; declared in tracking_loop.h)
#endif
