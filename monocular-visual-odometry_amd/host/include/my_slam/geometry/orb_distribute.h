// my_slam/geometry/orb_distribute.h -- key points the ORB-SLAM way: the first of the two remedies the reference names for its
// failure on low-texture sequences (README.md section 5: "use the ORB-SLAM's method for extracting enough uniformly distributed
// keypoints across different scales") and has no function for.  Executed by libmvo_hip.so through the hot-path context of the
// calling thread (mvo_orb_distribute_configure, mvo_calc_keypoints_distributed, include/mvo_hip.h; declared arithmetic:
// DESIGN.md section 16).
//   orbDistributeKeypoints     the optional key `orb_distribute_keypoints` (0 / 1, default 0), latched on first use
//   calcKeyPointsDistributed   calcKeyPoints(image, keypoints) by cell-wise FAST with two thresholds and a quadtree spread
// Optional keys, latched on first use: orb_distribute_ini_threshold (default 20), orb_distribute_min_threshold (7),
// orb_distribute_cell_size (30), orb_distribute_edge_threshold (19).  The pyramid, the number of key points and the grid
// selection that follows are the ones of calcKeyPoints (number_of_keypoints_to_extract, scale_factor, level_pyramid, ...);
// score_threshold is not used.
#ifndef MY_SLAM_ORB_DISTRIBUTE_H
#define MY_SLAM_ORB_DISTRIBUTE_H
#include "my_slam/basics/config.h"
#include "my_slam/common_include.h"
#include "my_slam/geometry/feature_match.h"

// Bound weakly: a program that includes this header still links and runs against a build of the library without this
// detector; calling calcKeyPointsDistributed with such a library is an error, not a fall-back.
#pragma weak mvo_orb_distribute_configure
#pragma weak mvo_calc_keypoints_distributed
#pragma weak mvo_debug_get_distribute_candidates

namespace my_slam {
namespace geometry {

namespace detail {
// host/src/feature_match_mvo.cpp: hands the ORB parameters of config.yaml to the ctx of the calling thread, once per ctx
void latch_orb_params();
}  // namespace detail

inline bool orbDistributeKeypoints() {
    static const bool on = basics::Config::has("orb_distribute_keypoints") && basics::Config::get<int>("orb_distribute_keypoints") != 0;
    return on;
}

inline mvo_orb_distribute_params orbDistributeParams() {
    auto opt = [](const char* key, int def) { return basics::Config::has(key) ? basics::Config::get<int>(key) : def; };
    static const mvo_orb_distribute_params p = {opt("orb_distribute_ini_threshold", 20), opt("orb_distribute_min_threshold", 7),
                                                opt("orb_distribute_cell_size", 30), opt("orb_distribute_edge_threshold", 19)};
    return p;
}

// candidates_per_level / keypoints_per_level (optional): how many candidates every pyramid level gave and how many key points
// of it are in `keypoints`
inline void calcKeyPointsDistributed(const cv::Mat& image, vector<cv::KeyPoint>& keypoints, vector<int>* candidates_per_level = nullptr,
                                     vector<int>* keypoints_per_level = nullptr) {
    if (!mvo_orb_distribute_configure || !mvo_calc_keypoints_distributed || !mvo_debug_get_distribute_candidates)
        throw std::runtime_error("calcKeyPointsDistributed: this libmvo_hip.so has no mvo_calc_keypoints_distributed");
    detail::latch_orb_params();
    detail::pyramid_token() = 0;
    const mvo_orb_distribute_params p = orbDistributeParams();
    mvo_check(mvo_orb_distribute_configure(hot_path_ctx(), &p), "mvo_orb_distribute_configure");
    const int cap = basics::Config::get<int>("max_number_of_keypoints") + 16;
    keypoints.resize(cap);
    int n = 0;
    mvo_check(mvo_calc_keypoints_distributed(hot_path_ctx(), image.data, image.cols, image.rows, (int)image.step, image.channels(),
                                             reinterpret_cast<mvo_keypoint*>(keypoints.data()), cap, &n),
              "calcKeyPointsDistributed");
    keypoints.resize(n);
    const int nlevels = basics::Config::get<int>("level_pyramid");
    if (candidates_per_level) {
        int nc = 0;
        mvo_check(mvo_debug_get_distribute_candidates(hot_path_ctx(), nullptr, 0, &nc), "mvo_debug_get_distribute_candidates");
        vector<mvo_distribute_candidate> c(nc > 0 ? nc : 1);
        mvo_check(mvo_debug_get_distribute_candidates(hot_path_ctx(), c.data(), (int)c.size(), &nc), "mvo_debug_get_distribute_candidates");
        candidates_per_level->assign(nlevels, 0);
        for (int i = 0; i < nc; ++i) (*candidates_per_level)[c[i].level]++;
    }
    if (keypoints_per_level) {
        keypoints_per_level->assign(nlevels, 0);
        for (const cv::KeyPoint& k : keypoints) (*keypoints_per_level)[k.octave]++;
    }
}

}  // namespace geometry
}  // namespace my_slam
#endif
