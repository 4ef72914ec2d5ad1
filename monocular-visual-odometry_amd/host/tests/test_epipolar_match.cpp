// host/tests/test_epipolar_match.cpp -- drives the mirror of the pose-guided matcher (my_slam/geometry/epipolar_match.h) and
// the keyframe insertion that can use it (my_slam/vo/keyframe.h) and dumps the results for tests/test_epipolar_host.py.
//   test_epipolar_match <scene.bin> <out.bin> [key=value ...]
// scene.bin: int32 N1, N2; double K[4]; double T_w_ref[16], T_w_cur[16]; then per frame (ref, cur): float xy[N*2];
//            int32 octave[N]; uint8 desc[N*32].  key=value pairs are set in basics::Config before anything is latched.
// out.bin (each a uint64 count followed by the items): F of fundamentalFromPoses (9 f64); the matches of
// matchFeaturesByEpipolarLine; those of mvo_match_features_epipolar called directly with the same parameters; those of
// matchFeatures as the keyframe insertion calls it; then, after triangulateWithReferenceKeyframe: matches_with_ref_,
// inliers_matches_with_ref_, inliers_matches_for_3d_, epipolar_F_ (9 f64 or none), epipolar_ref_id_ (1 int32).
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "my_slam/vo/keyframe.h"

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
    const int N1 = hdr[0], N2 = hdr[1];
    double K4[4], Tr[16], Tc[16];
    rd(in, K4, 4);
    rd(in, Tr, 16);
    rd(in, Tc, 16);
    try {
        cv::Mat K = cv::Mat::eye(3, 3, CV_64FC1);
        K.at<double>(0, 0) = K4[0];
        K.at<double>(1, 1) = K4[1];
        K.at<double>(0, 2) = K4[2];
        K.at<double>(1, 2) = K4[3];
        vo::Frame::Ptr ref = vo::Frame::createFrame(cv::Mat()), curr = vo::Frame::createFrame(cv::Mat());
        for (int i = 0; i < 16; ++i) {
            ref->T_w_c_.at<double>(i / 4, i % 4) = Tr[i];
            curr->T_w_c_.at<double>(i / 4, i % 4) = Tc[i];
        }
        vector<float> xy[2], scale2;
        int f = 0;
        for (auto& fn : {std::make_pair(ref, N1), std::make_pair(curr, N2)}) {
            xy[f].resize(2 * (size_t)fn.second);
            vector<int> octave(fn.second);
            rd(in, xy[f].data(), xy[f].size());
            rd(in, octave.data(), octave.size());
            for (int i = 0; i < fn.second; ++i)
                fn.first->keypoints_.push_back(cv::KeyPoint(xy[f][2 * i], xy[f][2 * i + 1], 31, -1, 0, octave[i]));
            fn.first->descriptors_.create(fn.second, 32, CV_8UC1);
            rd(in, fn.first->descriptors_.data, (size_t)fn.second * 32);
            if (f == 1)
                for (int i = 0; i < fn.second; ++i) {
                    double s = 1.0;
                    for (int o = 0; o < octave[i]; ++o) s *= basics::Config::get<double>("scale_factor");
                    scale2.push_back((float)s);
                }
            ++f;
        }
        // the mirror functions ...
        const cv::Mat F = geometry::fundamentalFromPoses(ref->T_w_c_, curr->T_w_c_, K);
        dump(out, F.ptr<double>(0), 9);
        vector<cv::DMatch> mirror;
        geometry::matchFeaturesByEpipolarLine(ref->descriptors_, curr->descriptors_, ref->keypoints_, curr->keypoints_, F, mirror);
        dump(out, mirror.data(), mirror.size());
        // ... and the C-ABI with the parameters the mirror latched
        vector<mvo_dmatch> direct(std::max(1, std::min(N1, N2)));
        int n = 0;
        mvo_check(mvo_match_features_epipolar(hot_path_ctx(), ref->descriptors_.data, xy[0].data(), N1, curr->descriptors_.data,
                                              xy[1].data(), scale2.data(), N2, F.ptr<double>(0),
                                              basics::Config::get<double>("epipolar_match_max_line_dist"),
                                              basics::Config::get<double>("epipolar_match_lowe_ratio"),
                                              basics::Config::get<int>("epipolar_match_max_hamming"), direct.data(), (int)direct.size(), &n),
                  "mvo_match_features_epipolar");
        dump(out, direct.data(), (size_t)n);
        vector<cv::DMatch> blind;
        geometry::matchFeatures(ref->descriptors_, curr->descriptors_, blind, (int)basics::Config::get<float>("feature_match_method_index_pnp"),
                                false, ref->keypoints_, curr->keypoints_, basics::Config::get<float>("max_matching_pixel_dist_in_triangulation"));
        dump(out, blind.data(), blind.size());
        // the keyframe insertion
        vo::triangulateWithReferenceKeyframe(curr, ref, K);
        dump(out, curr->matches_with_ref_.data(), curr->matches_with_ref_.size());
        dump(out, curr->inliers_matches_with_ref_.data(), curr->inliers_matches_with_ref_.size());
        dump(out, curr->inliers_matches_for_3d_.data(), curr->inliers_matches_for_3d_.size());
        dump(out, curr->epipolar_F_.empty() ? nullptr : curr->epipolar_F_.ptr<double>(0), curr->epipolar_F_.empty() ? 0 : 9);
        const int ids[2] = {curr->epipolar_ref_id_, ref->id_};
        dump(out, ids, 2);
    } catch (const std::exception& e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
