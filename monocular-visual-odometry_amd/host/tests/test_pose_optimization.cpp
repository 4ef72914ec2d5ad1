// host/tests/test_pose_optimization.cpp -- drives the mirror of the robust motion-only pose optimisation
// (my_slam/vo/pose_optimization.h) and dumps the results for tests/test_pose_optimization_host.py.
//   test_pose_optimization <scene.bin> <out.bin> [key=value ...]
// scene.bin: int32 n (matches), nk (keypoints); double fx, fy, cx, cy; double T_w_c[16] (the predicted pose); float kpt[nk*2] (the
//            keypoints' pixels); int32 octave[nk]; float p3[n*3] (the matched map points); int32 train[n] (the keypoint of match
//            i).  key=value pairs are set in basics::Config before anything is latched.
// out.bin (each a uint64 count followed by the items): [trackingPoseByOptimization(), poseOptimizationMinInliers(), status]
// (int32); the inliers (int32); T_w_c as returned (f64, 16, or none for a status other than 0); what optimizePoseFromMatches
// recorded: the set-up (f64), the initial pose (f64), the points, pixels and inv_sigma2 (f32), T_w_c and T_c_w (f64), info
// (int32), chi2 (f64), the outlier flags.
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "my_slam/vo/pose_optimization.h"

using namespace my_slam;

template <class T>
static void rd(std::ifstream& f, T* p, size_t n) {
    if (!f.read(reinterpret_cast<char*>(p), (std::streamsize)(n * sizeof(T)))) {
        fprintf(stderr, "short scene file\n");
        exit(2);
    }
}
template <class T>
static void dump(std::ofstream& o, const T* p, size_t n) {
    unsigned long long cnt = n;
    o.write(reinterpret_cast<const char*>(&cnt), 8);
    o.write(reinterpret_cast<const char*>(p), (std::streamsize)(n * sizeof(T)));
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    std::ofstream out(argv[2], std::ios::binary);
    for (int a = 3; a < argc; ++a) {
        const string kv = argv[a];
        const size_t eq = kv.find('=');
        if (eq == string::npos) return 2;
        basics::Config::set(kv.substr(0, eq), kv.substr(eq + 1));
    }
    int hdr[2];
    rd(in, hdr, 2);
    const int n = hdr[0], nk = hdr[1];
    double k4[4], T[16];
    rd(in, k4, 4);
    rd(in, T, 16);
    cv::Mat K = cv::Mat::eye(3, 3, CV_64FC1);
    K.at<double>(0, 0) = k4[0], K.at<double>(1, 1) = k4[1], K.at<double>(0, 2) = k4[2], K.at<double>(1, 2) = k4[3];
    vector<float> kpt(2 * (size_t)nk), p3(3 * (size_t)n);
    vector<int> octave(nk), train(n);
    rd(in, kpt.data(), kpt.size());
    rd(in, octave.data(), octave.size());
    rd(in, p3.data(), p3.size());
    rd(in, train.data(), train.size());
    try {
        cv::Mat img(8, 8, CV_8UC3);
        vo::Frame::Ptr curr = vo::Frame::createFrame(img);
        for (int i = 0; i < 16; ++i) curr->T_w_c_.at<double>(i / 4, i % 4) = T[i];
        curr->keypoints_.resize(nk);
        for (int k = 0; k < nk; ++k) {
            curr->keypoints_[k].pt = cv::Point2f(kpt[2 * k], kpt[2 * k + 1]);
            curr->keypoints_[k].octave = octave[k];
        }
        vector<cv::Point3f> pts_3d;
        vector<cv::Point2f> pts_2d;
        for (int i = 0; i < n; ++i) {
            curr->matches_with_map_.push_back(cv::DMatch(i, train[i], 0, 0.f));
            pts_3d.push_back(cv::Point3f(p3[3 * i], p3[3 * i + 1], p3[3 * i + 2]));
            pts_2d.push_back(curr->keypoints_[train[i]].pt);
        }
        vector<int> inliers;
        cv::Mat T_w_c;
        const int status = vo::optimizePoseFromMatches(curr, pts_3d, pts_2d, K, inliers, T_w_c);
        const int head[3] = {vo::trackingPoseByOptimization() ? 1 : 0, vo::poseOptimizationMinInliers(), status};
        dump(out, head, 3);
        dump(out, inliers.data(), inliers.size());
        vector<double> Tout;
        if (!T_w_c.empty())
            for (int i = 0; i < 16; ++i) Tout.push_back(T_w_c.at<double>(i / 4, i % 4));
        dump(out, Tout.data(), Tout.size());
        dump(out, curr->pose_opt_setup_.data(), curr->pose_opt_setup_.size());
        dump(out, curr->pose_opt_init_.data(), curr->pose_opt_init_.size());
        dump(out, curr->pose_opt_p3_.data(), curr->pose_opt_p3_.size());
        dump(out, curr->pose_opt_p2_.data(), curr->pose_opt_p2_.size());
        dump(out, curr->pose_opt_sigma_.data(), curr->pose_opt_sigma_.size());
        dump(out, curr->pose_opt_T_w_c_.data(), curr->pose_opt_T_w_c_.size());
        dump(out, curr->pose_opt_T_c_w_.data(), curr->pose_opt_T_c_w_.size());
        dump(out, curr->pose_opt_info_.data(), curr->pose_opt_info_.size());
        dump(out, curr->pose_opt_chi2_.data(), curr->pose_opt_chi2_.size());
        dump(out, curr->pose_opt_outlier_.data(), curr->pose_opt_outlier_.size());
    } catch (const std::exception& e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
