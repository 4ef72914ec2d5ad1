// my_slam/geometry/epipolar_match.h -- matching under the epipolar constraint of two frames whose poses are known: what
// the reference names as its missing piece (README.md:212 "doing guided matching based on the estimated camera motion",
// README.md:272 "Utilize epipolar constraint to do feature matching") and has no function for.  Executed by libmvo_hip.so
// through the hot-path context of the calling thread (mvo_fundamental_from_poses, mvo_match_features_epipolar,
// include/mvo_hip.h; declared arithmetic: DESIGN.md section 14).
//   fundamentalFromPoses          F with x2^T F x1 = 0 in pixels from two camera-to-world poses and K
//   matchFeaturesByEpipolarLine   matchFeatures(desc1, desc2) in which keypoint j of frame 2 competes for keypoint i of
//                                 frame 1 only within a tolerance of i's epipolar line; queryIdx -> frame 1, trainIdx -> frame 2
// Optional keys, latched on first use: epipolar_match_max_line_dist (px at pyramid level 0, default 2.0; a keypoint of
// octave o gets scale_factor^o times as much), epipolar_match_lowe_ratio (default 0.8), epipolar_match_max_hamming
// (default 64).
#ifndef MY_SLAM_EPIPOLAR_MATCH_H
#define MY_SLAM_EPIPOLAR_MATCH_H
#include <algorithm>

#include "my_slam/basics/config.h"
#include "my_slam/common_include.h"

// Bound weakly: a program that includes this header still links and runs against a build of the library without the
// pose-guided matcher; calling one of the two functions with such a library is an error, not a fall-back.
#pragma weak mvo_fundamental_from_poses
#pragma weak mvo_match_features_epipolar

namespace my_slam {
namespace geometry {

inline cv::Mat fundamentalFromPoses(const cv::Mat& T_w_c_1, const cv::Mat& T_w_c_2, const cv::Mat& K) {
    if (!mvo_fundamental_from_poses) throw std::runtime_error("fundamentalFromPoses: this libmvo_hip.so has no mvo_fundamental_from_poses");
    double T1[16], T2[16];
    for (int i = 0; i < 16; ++i) {
        T1[i] = T_w_c_1.at<double>(i / 4, i % 4);
        T2[i] = T_w_c_2.at<double>(i / 4, i % 4);
    }
    cv::Mat F(3, 3, CV_64FC1);
    if (mvo_fundamental_from_poses(T1, T2, K.at<double>(0, 0), K.at<double>(1, 1), K.at<double>(0, 2), K.at<double>(1, 2),
                                   F.ptr<double>(0)) != MVO_OK)
        throw std::runtime_error("fundamentalFromPoses: singular pose or camera matrix");
    return F;
}

inline void matchFeaturesByEpipolarLine(const cv::Mat1b& descriptors_1, const cv::Mat1b& descriptors_2,
                                        const vector<cv::KeyPoint>& keypoints_1, const vector<cv::KeyPoint>& keypoints_2,
                                        const cv::Mat& F, vector<cv::DMatch>& matches) {
    if (!mvo_match_features_epipolar)
        throw std::runtime_error("matchFeaturesByEpipolarLine: this libmvo_hip.so has no mvo_match_features_epipolar");
    static const double max_line_dist =
        basics::Config::has("epipolar_match_max_line_dist") ? basics::Config::get<double>("epipolar_match_max_line_dist") : 2.0;
    static const double lowe_ratio =
        basics::Config::has("epipolar_match_lowe_ratio") ? basics::Config::get<double>("epipolar_match_lowe_ratio") : 0.8;
    static const int max_hamming =
        basics::Config::has("epipolar_match_max_hamming") ? basics::Config::get<int>("epipolar_match_max_hamming") : 64;
    static const double scale_factor = basics::Config::get<double>("scale_factor");
    const int n1 = (int)keypoints_1.size(), n2 = (int)keypoints_2.size();
    if (descriptors_1.rows != n1 || descriptors_2.rows != n2 || (n1 && descriptors_1.cols != 32) || (n2 && descriptors_2.cols != 32))
        throw std::runtime_error("matchFeaturesByEpipolarLine: one 32-byte descriptor per keypoint is required");
    // rows of 32 bytes back to back (a descriptor matrix with padded rows is packed first)
    vector<unsigned char> pack1, pack2;
    auto packed = [](const cv::Mat1b& d, vector<unsigned char>& buf) -> const unsigned char* {
        if (d.rows == 0) return nullptr;
        if ((int)d.step == 32) return d.data;
        buf.resize((size_t)d.rows * 32);
        for (int r = 0; r < d.rows; ++r) std::copy(d.data + (size_t)r * d.step, d.data + (size_t)r * d.step + 32, buf.begin() + (size_t)r * 32);
        return buf.data();
    };
    const unsigned char *d1 = packed(descriptors_1, pack1), *d2 = packed(descriptors_2, pack2);
    vector<float> xy1(2 * (size_t)n1), xy2(2 * (size_t)n2), scale2(n2);
    for (int i = 0; i < n1; ++i) xy1[2 * i] = keypoints_1[i].pt.x, xy1[2 * i + 1] = keypoints_1[i].pt.y;
    for (int j = 0; j < n2; ++j) {
        xy2[2 * j] = keypoints_2[j].pt.x, xy2[2 * j + 1] = keypoints_2[j].pt.y;
        double s = 1.0;
        for (int o = 0; o < keypoints_2[j].octave; ++o) s *= scale_factor;
        scale2[j] = (float)s;
    }
    double f[9];
    for (int i = 0; i < 9; ++i) f[i] = F.at<double>(i / 3, i % 3);
    vector<mvo_dmatch> out(std::max(1, std::min(n1, n2)));
    int n = 0;
    mvo_check(mvo_match_features_epipolar(hot_path_ctx(), d1, n1 ? xy1.data() : nullptr, n1,
                                          d2, n2 ? xy2.data() : nullptr, n2 ? scale2.data() : nullptr, n2,
                                          f, max_line_dist, lowe_ratio, max_hamming, out.data(), (int)out.size(), &n),
              "matchFeaturesByEpipolarLine");
    matches.clear();
    for (int i = 0; i < n; ++i) matches.push_back(cv::DMatch(out[i].queryIdx, out[i].trainIdx, out[i].imgIdx, out[i].distance));
}

}  // namespace geometry
}  // namespace my_slam
#endif
