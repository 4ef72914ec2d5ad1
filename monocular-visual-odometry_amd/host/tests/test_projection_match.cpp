// host/tests/test_projection_match.cpp -- drives the mirror of tracking by projection (my_slam/vo/projection_match.h) and the
// poseEstimationPnP that can use it (my_slam/vo/pnp_tracking.h) and dumps the results for tests/test_projection_host.py.
//   test_projection_match <scene.bin> <out.bin> [key=value ...]
// scene.bin: int32 n_map, nt, cols, rows; double K[4]; double T_prev2[16], T_prev[16]; float pos[n_map*3];
//            uint8 desc[n_map*32]; float txy[nt*2]; int32 octave[nt]; uint8 tdesc[nt*32].  key=value pairs are set in
//            basics::Config before anything is latched.
// out.bin (each a uint64 count followed by the items): predictPose (16 f64); for every position of MapOnDevice::order() the
// index of that point in the scene (int32); of matchMapByProjection under the predicted pose: the candidates (scene
// indices), their pixels (f32 pairs), the matches; the matches of mvo_map_match_features_projection called directly with the
// same parameters (queryIdx = map index); of getMappointsInCurrentView under the pose trackFrame would give the
// frame (the predicted one with the key on, prev's without): candidates, pixels; the
// matches of matchFeatures on them as poseEstimationPnP calls it; then, after poseEstimationPnP from the pose trackFrame
// would give it: [ran, is_pnp_good] (int32), Frame::projection_matches_, matches_with_map_, the resulting T_w_c_ (16 f64).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>

#include "my_slam/vo/projection_match.h"

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
    int hdr[4];
    rd(in, hdr, 4);
    const int n_map = hdr[0], nt = hdr[1], cols = hdr[2], rows = hdr[3];
    double K4[4], T2[16], T1[16];
    rd(in, K4, 4);
    rd(in, T2, 16);
    rd(in, T1, 16);
    vector<float> pos(3 * (size_t)n_map), txy(2 * (size_t)nt);
    vector<unsigned char> desc(32 * (size_t)n_map);
    vector<int> octave(nt);
    rd(in, pos.data(), pos.size());
    rd(in, desc.data(), desc.size());
    rd(in, txy.data(), txy.size());
    rd(in, octave.data(), octave.size());
    try {
        cv::Mat K = cv::Mat::eye(3, 3, CV_64FC1);
        K.at<double>(0, 0) = K4[0];
        K.at<double>(1, 1) = K4[1];
        K.at<double>(0, 2) = K4[2];
        K.at<double>(1, 2) = K4[3];
        cv::Mat img(rows, cols, CV_8UC3);
        vo::Frame::Ptr prev2 = vo::Frame::createFrame(img), prev = vo::Frame::createFrame(img), curr = vo::Frame::createFrame(img);
        for (int i = 0; i < 16; ++i) {
            prev2->T_w_c_.at<double>(i / 4, i % 4) = T2[i];
            prev->T_w_c_.at<double>(i / 4, i % 4) = T1[i];
        }
        vector<float> scale;
        for (int j = 0; j < nt; ++j) {
            curr->keypoints_.push_back(cv::KeyPoint(txy[2 * j], txy[2 * j + 1], 31, -1, 0, octave[j]));
            double s = 1.0;
            for (int o = 0; o < octave[j]; ++o) s *= basics::Config::get<double>("scale_factor");
            scale.push_back((float)s);
        }
        curr->descriptors_.create(nt, 32, CV_8UC1);
        rd(in, curr->descriptors_.data, (size_t)nt * 32);
        vo::Map::Ptr map(new vo::Map());
        std::map<int, int> scene_index;  // MapPoint::id_ -> index in the scene
        for (int i = 0; i < n_map; ++i) {
            cv::Mat d(1, 32, CV_8UC1), norm(3, 1, CV_64FC1);
            std::memcpy(d.data, &desc[32 * (size_t)i], 32);
            for (int r = 0; r < 3; ++r) norm.at<double>(r, 0) = r == 2 ? 1.0 : 0.0;
            vo::MapPoint::Ptr p(new vo::MapPoint(cv::Point3f(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]), d, norm));
            scene_index[p->id_] = i;
            map->insertMapPoint(p);
        }
        vo::MapOnDevice dev_map;
        auto ids_of = [&](const vector<vo::MapPoint::Ptr>& v) {
            vector<int> ids;
            for (const vo::MapPoint::Ptr& p : v) ids.push_back(scene_index[p->id_]);
            return ids;
        };
        const cv::Mat pred = vo::predictPose(prev2->T_w_c_, prev->T_w_c_);
        dump(out, pred.ptr<double>(0), 16);
        // the mirror under the predicted pose ...
        curr->T_w_c_ = pred.clone();
        vector<vo::MapPoint::Ptr> cand;
        vector<cv::Point2f> cand_px;
        vector<cv::DMatch> mirror;
        vo::matchMapByProjection(dev_map, map, curr, K, cand, cand_px, mirror);
        const vector<int> order = ids_of(dev_map.order());
        dump(out, order.data(), order.size());
        const vector<int> cand_ids = ids_of(cand);
        dump(out, cand_ids.data(), cand_ids.size());
        dump(out, cand_px.data(), cand_px.size());
        dump(out, mirror.data(), mirror.size());
        // ... the C-ABI with the parameters the mirror latched ...
        vector<mvo_dmatch> direct(std::max(1, std::min(n_map, nt)));
        int n = 0;
        mvo_check(mvo_map_match_features_projection(hot_path_ctx(), dev_map.handle(), pred.ptr<double>(0), K4[0], K4[1], K4[2], K4[3], cols,
                                                    rows, curr->descriptors_.data, txy.data(), scale.data(), nt,
                                                    basics::Config::get<double>("projection_match_max_pixel_dist"),
                                                    basics::Config::get<double>("projection_match_lowe_ratio"),
                                                    basics::Config::get<int>("projection_match_max_hamming"), nullptr, nullptr,
                                                    direct.data(), (int)direct.size(), &n),
                  "mvo_map_match_features_projection");
        dump(out, direct.data(), (size_t)n);
        // ... and the reference's two steps under the pose trackFrame would give the frame: the prediction with the key on, else
        // the last keyframe's, which in this scene is prev's
        const cv::Mat start = vo::trackingMatchByProjection() ? pred : prev->T_w_c_;
        curr->T_w_c_ = start.clone();
        vector<vo::MapPoint::Ptr> cand0;
        vector<cv::Point2f> cand0_px;
        cv::Mat cand0_desc;
        vo::getMappointsInCurrentView(dev_map, map, curr, K, cand0, cand0_px, cand0_desc);
        const vector<int> cand0_ids = ids_of(cand0);
        dump(out, cand0_ids.data(), cand0_ids.size());
        dump(out, cand0_px.data(), cand0_px.size());
        vector<cv::KeyPoint> cand0_kpts;
        for (const cv::Point2f& pt : cand0_px) cand0_kpts.push_back(cv::KeyPoint(pt, 10));
        vector<cv::DMatch> blind;
        geometry::matchFeatures(cand0_desc, curr->descriptors_, blind, (int)basics::Config::get<float>("feature_match_method_index_pnp"), false,
                                cand0_kpts, curr->keypoints_, basics::Config::get<float>("max_matching_pixel_dist_in_pnp"));
        dump(out, blind.data(), blind.size());
        // poseEstimationPnP from that pose
        curr->T_w_c_ = start.clone();
        curr->projection_matches_.clear();
        int flags[2] = {1, 0};
        try {
            flags[1] = vo::poseEstimationPnP(dev_map, map, curr, prev, K) ? 1 : 0;
        } catch (const std::runtime_error& e) {
            fprintf(stderr, "poseEstimationPnP: %s\n", e.what());
            flags[0] = 0;
        }
        dump(out, flags, 2);
        dump(out, curr->projection_matches_.data(), curr->projection_matches_.size());
        dump(out, curr->matches_with_map_.data(), curr->matches_with_map_.size());
        dump(out, curr->T_w_c_.ptr<double>(0), 16);
    } catch (const std::exception& e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
