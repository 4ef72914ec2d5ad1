// host/tests/test_map_refine.cpp -- drives the mirror of the map-point position refinement (my_slam/vo/map_refine.h) and dumps
// the results for tests/test_map_refine_host.py.
//   test_map_refine <scene.bin> <out.bin> [key=value ...]
// scene.bin: int32 n_pts, n_frames (<= 20), nk; double fx, fy, cx, cy; float pos[n_pts*3]; then per frame, oldest first:
//            double T_w_c[16]; float kpt[nk*2] (the keypoints' pixels); int32 conn[nk] (the scene index of the map point keypoint
//            k is connected to, -1: none, -2: a point that is no longer in the map).  key=value pairs are set in basics::Config
//            before anything is latched.  Every frame's connection map is filled in a scrambled keypoint order.
// out.bin (each a uint64 count followed by the items): [mapPointRefinePositions()] (int32); for every position of
// MapOnDevice::order() the index of that point in the scene (int32); collectObservations: obs_start (int32), obs_frame (int32),
// obs_uv (f32); what refineMapPointPositions recorded: the set-up (f64), the positions before and after (f32), chi2 (f64), info
// (int32), the outlier flags; then, per position of order(): MapPoint::pos_ (f32), MapOnDevice's host copy of the positions
// and the resident positions (mvo_debug_get_map).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>

#include "my_slam/vo/map_refine.h"

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
    int hdr[3];
    rd(in, hdr, 3);
    const int n_pts = hdr[0], n_frames = hdr[1], nk = hdr[2];
    double k4[4];
    rd(in, k4, 4);
    cv::Mat K = cv::Mat::eye(3, 3, CV_64FC1);
    K.at<double>(0, 0) = k4[0], K.at<double>(1, 1) = k4[1], K.at<double>(0, 2) = k4[2], K.at<double>(1, 2) = k4[3];
    vector<float> pos(3 * (size_t)n_pts);
    rd(in, pos.data(), pos.size());
    try {
        const int flag = vo::mapPointRefinePositions() ? 1 : 0;
        dump(out, &flag, 1);
        vo::TrackingState st;
        std::map<int, int> scene_index;  // MapPoint::id_ -> index in the scene
        vector<int> id_of(n_pts);
        for (int i = 0; i < n_pts; ++i) {
            cv::Mat d = cv::Mat::zeros(1, 32, CV_8UC1), norm(3, 1, CV_64FC1);
            for (int r = 0; r < 3; ++r) norm.at<double>(r, 0) = r == 2 ? 1.0 : 0.0;
            vo::MapPoint::Ptr p(new vo::MapPoint(cv::Point3f(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]), d, norm));
            scene_index[p->id_] = i;
            id_of[i] = p->id_;
            st.map_->insertMapPoint(p);
        }
        const int gone_id = vo::MapPoint::factory_id() + 1000;  // a point culled long ago
        cv::Mat img(8, 8, CV_8UC3);
        for (int f = 0; f < n_frames; ++f) {
            vo::Frame::Ptr fr = vo::Frame::createFrame(img);
            double T[16];
            rd(in, T, 16);
            for (int i = 0; i < 16; ++i) fr->T_w_c_.at<double>(i / 4, i % 4) = T[i];
            vector<float> kpt(2 * (size_t)nk);
            rd(in, kpt.data(), kpt.size());
            fr->keypoints_.resize(nk);
            for (int k = 0; k < nk; ++k) fr->keypoints_[k].pt = cv::Point2f(kpt[2 * k], kpt[2 * k + 1]);
            fr->descriptors_ = cv::Mat::zeros(nk, 32, CV_8UC1);
            vector<int> conn(nk);
            rd(in, conn.data(), conn.size());
            for (int s = 0; s < nk; ++s) {  // scrambled: a stride coprime to nk, starting somewhere else in every frame
                const int k = (int)(((long long)s * 7919 + 13 * f) % nk);
                if (conn[k] == -1) continue;
                fr->inliers_to_mappt_connections_[k] = vo::PtConn{-1, conn[k] == -2 ? gone_id : id_of[conn[k]]};
            }
            st.pushFrameToBuff(fr);
        }
        st.dev_map_.sync(st.map_);
        vector<int> order;
        for (const vo::MapPoint::Ptr& p : st.dev_map_.order()) order.push_back(scene_index[p->id_]);
        dump(out, order.data(), order.size());
        const vo::MapObservations o = vo::collectObservations(st.frames_buff_, st.dev_map_.order());
        dump(out, o.obs_start.data(), o.obs_start.size());
        dump(out, o.obs_frame.data(), o.obs_frame.size());
        dump(out, o.obs_uv.data(), o.obs_uv.size());
        vo::Frame::Ptr probe = vo::Frame::createFrame(img);
        vo::refineMapPointPositions(st, K, probe);
        dump(out, probe->refine_setup_.data(), probe->refine_setup_.size());
        dump(out, probe->refine_pos_before_.data(), probe->refine_pos_before_.size());
        dump(out, probe->refine_pos_after_.data(), probe->refine_pos_after_.size());
        dump(out, probe->refine_chi2_.data(), probe->refine_chi2_.size());
        dump(out, probe->refine_info_.data(), probe->refine_info_.size());
        dump(out, probe->refine_outlier_.data(), probe->refine_outlier_.size());
        const int n = (int)st.dev_map_.order().size();
        vector<float> ppos;
        for (const vo::MapPoint::Ptr& p : st.dev_map_.order()) ppos.push_back(p->pos_.x), ppos.push_back(p->pos_.y), ppos.push_back(p->pos_.z);
        dump(out, ppos.data(), ppos.size());
        dump(out, st.dev_map_.positions().data(), st.dev_map_.positions().size());
        vector<float> rpos(3 * (size_t)n + 1);
        int got = 0;
        mvo_check(mvo_debug_get_map(hot_path_ctx(), st.dev_map_.handle(), rpos.data(), nullptr, n, &got), "mvo_debug_get_map");
        dump(out, rpos.data(), 3 * (size_t)got);
    } catch (const std::exception& e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
