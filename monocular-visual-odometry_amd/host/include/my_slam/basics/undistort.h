// my_slam/basics/undistort.h -- cv::undistort(img, dst, K, dist) as the reference's python_tools/undistort_all_images.py:11-37
// applies it to a dataset before run_vo reads it (config/config.yaml:17,39: "The images should all be undistorted"), on the
// MI355X through the hot-path context of the calling thread (mvo_undistort_configure + mvo_undistort, include/mvo_hip.h;
// declared arithmetic: DESIGN.md section 13).  The map is built on first use and again whenever K, dist or the image
// size change: the library compares them, the same values cost nothing.
#ifndef MY_SLAM_UNDISTORT_H
#define MY_SLAM_UNDISTORT_H
#include "my_slam/common_include.h"

namespace my_slam {
namespace basics {

// img: CV_8UC1 / CV_8UC3 / CV_8UC4; K: 3 x 3 CV_64F; dist: 4, 5 or 8 coefficients (k1, k2, p1, p2[, k3[, k4, k5, k6]])
inline cv::Mat undistort(const cv::Mat& img, const cv::Mat& K, const std::vector<double>& dist) {
    if (img.empty() || img.depth() != CV_8U) throw std::runtime_error("basics::undistort: an 8-bit image is required");
    if (dist.size() > 8) throw std::runtime_error("basics::undistort: at most 8 distortion coefficients are supported");
    mvo_undistort_params p{};
    p.fx = K.at<double>(0, 0);
    p.fy = K.at<double>(1, 1);
    p.cx = K.at<double>(0, 2);
    p.cy = K.at<double>(1, 2);
    p.n_coeffs = (int32_t)dist.size();
    for (size_t i = 0; i < dist.size(); i++) p.coeffs[i] = dist[i];
    mvo_check(mvo_undistort_configure(hot_path_ctx(), &p, img.cols, img.rows), "mvo_undistort_configure");
    cv::Mat out(img.rows, img.cols, img.type());
    mvo_check(mvo_undistort(hot_path_ctx(), img.data, img.cols, img.rows, (int)img.step, img.channels(), out.data, (int)out.step),
              "mvo_undistort");
    return out;
}

}  // namespace basics
}  // namespace my_slam
#endif
