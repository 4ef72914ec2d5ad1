// host/tests/test_window_triangulate.cpp -- drives the mirror of the new map points from every buffered frame
// (my_slam/vo/window_triangulate.h) and dumps the results for tests/test_window_triangulate_host.py.
//   test_window_triangulate <scene.bin> <out.bin> [key=value ...]
// scene.bin: int32 n_pts, n_frames (<= 20, the keyframe last), cols, rows; double fx, fy, cx, cy; float pos[n_pts*3]; uint8
//            desc[n_pts*32]; then per frame, oldest first: int32 nk; double T_w_c[16]; float kpt[nk*2]; uint8 desc[nk*32]; int32
//            octave[nk]; int32 conn[nk] (the scene index of the map point keypoint k is connected to, -1: none, -2: a point that is
//            no longer in the map).  key=value pairs are set in basics::Config before anything is latched.  Keypoint k of the
//            keyframe has the colour (k, 2 k, 3 k) mod 256.
// out.bin (each a uint64 count followed by the items): [mapPointCreateFromWindow()] (int32); what createMapPointsFromWindow
// recorded: the set-up (f64), the keypoints per frame (int32), the connections (int32), the scales (f32), the points (int32, f32,
// f64), the pairs (int32, f32, f64), the counts, the ids of the new points (int32), their world positions (f32), the size of the
// map before and after (int32); then the state after the call: per new id, in the order of the ids, the position (f32 x 3), the
// descriptor (uint8 x 32), the normal (f64 x 3), the colour (uint8 x 3) as the map holds them; per keypoint of every frame what
// its connection names (-1: none, -2: the departed point, i >= 0: scene point i, 1000000 + k: the k-th new point, -3: anything
// else); the number of scene points still in the map (int32); the number of resident rows (mvo_map_size) before and after.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>

#include "my_slam/vo/window_triangulate.h"

using namespace my_slam;

template <class T>
static void rd(std::ifstream& f, T* p, size_t n) {
    if (!f.read(reinterpret_cast<char*>(p), (std::streamsize)(n * sizeof(T)))) {
        fprintf(stderr, "short scene file\n");
        exit(2);
    }
}
template <class T>
static void dump(std::ofstream& o, const vector<T>& v) {
    unsigned long long cnt = v.size();
    o.write(reinterpret_cast<const char*>(&cnt), 8);
    o.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
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
    const int n_pts = hdr[0], n_frames = hdr[1], cols = hdr[2], rows = hdr[3];
    double k4[4];
    rd(in, k4, 4);
    cv::Mat K = cv::Mat::eye(3, 3, CV_64FC1);
    K.at<double>(0, 0) = k4[0], K.at<double>(1, 1) = k4[1], K.at<double>(0, 2) = k4[2], K.at<double>(1, 2) = k4[3];
    vector<float> pos(3 * (size_t)n_pts);
    vector<unsigned char> desc(32 * (size_t)n_pts);
    rd(in, pos.data(), pos.size());
    rd(in, desc.data(), desc.size());
    try {
        dump(out, vector<int>{vo::mapPointCreateFromWindow() ? 1 : 0});
        vo::TrackingState st;
        std::map<int, int> scene_index;  // MapPoint::id_ -> index in the scene
        vector<int> id_of(n_pts);
        for (int i = 0; i < n_pts; ++i) {
            cv::Mat d(1, 32, CV_8UC1), norm(3, 1, CV_64FC1);
            std::memcpy(d.data, &desc[32 * (size_t)i], 32);
            for (int r = 0; r < 3; ++r) norm.at<double>(r, 0) = r == 2 ? 1.0 : 0.0;
            vo::MapPoint::Ptr p(new vo::MapPoint(cv::Point3f(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]), d, norm));
            scene_index[p->id_] = i;
            id_of[i] = p->id_;
            st.map_->insertMapPoint(p);
        }
        const int gone_id = vo::MapPoint::factory_id() + 1000;  // a point culled long ago
        vo::MapPoint::factory_id() += 2000;                     // (the new points take ids beyond it)
        cv::Mat img(rows, cols, CV_8UC3);
        for (int f = 0; f < n_frames; ++f) {
            vo::Frame::Ptr fr = vo::Frame::createFrame(img);
            int nk;
            rd(in, &nk, 1);
            double T[16];
            rd(in, T, 16);
            for (int i = 0; i < 16; ++i) fr->T_w_c_.at<double>(i / 4, i % 4) = T[i];
            vector<float> kpt(2 * (size_t)nk);
            rd(in, kpt.data(), kpt.size());
            fr->descriptors_ = cv::Mat::zeros(nk, 32, CV_8UC1);
            if (nk) rd(in, fr->descriptors_.ptr<unsigned char>(0), 32 * (size_t)nk);
            vector<int> octave(nk), conn(nk);
            rd(in, octave.data(), octave.size());
            rd(in, conn.data(), conn.size());
            fr->keypoints_.resize(nk);
            for (int k = 0; k < nk; ++k) {
                fr->keypoints_[k].pt = cv::Point2f(kpt[2 * k], kpt[2 * k + 1]);
                fr->keypoints_[k].octave = octave[k];
                fr->kpts_colors_.push_back({(unsigned char)(k % 256), (unsigned char)(2 * k % 256), (unsigned char)(3 * k % 256)});
            }
            for (int k = 0; k < nk; ++k) {
                if (conn[k] == -1) continue;
                fr->inliers_to_mappt_connections_[k] = vo::PtConn{-1, conn[k] == -2 ? gone_id : id_of[conn[k]]};
            }
            st.pushFrameToBuff(fr);
        }
        st.dev_map_.sync(st.map_);
        int resident_before = -1, resident_after = -1;
        mvo_check(mvo_map_size(hot_path_ctx(), st.dev_map_.handle(), &resident_before), "mvo_map_size");
        const vo::Frame::Ptr curr = st.frames_buff_.back();
        vo::createMapPointsFromWindow(st, K, curr);
        dump(out, curr->window_setup_);
        dump(out, curr->window_kp_count_);
        dump(out, curr->window_conn_);
        dump(out, curr->window_scale_);
        dump(out, curr->window_points_);
        dump(out, curr->window_points_p_);
        dump(out, curr->window_points_cos2_);
        dump(out, curr->window_pairs_);
        dump(out, curr->window_pairs_p_);
        dump(out, curr->window_pairs_cos2_);
        dump(out, curr->window_counts_);
        dump(out, curr->window_ids_);
        dump(out, curr->window_world_);
        dump(out, curr->window_map_size_);
        std::map<int, int> new_index;
        vector<float> n_pos;
        vector<unsigned char> n_desc, n_rgb;
        vector<double> n_norm;
        for (int k = 0; k < (int)curr->window_ids_.size(); ++k) {
            new_index[curr->window_ids_[k]] = k;
            const vo::MapPoint::Ptr& p = st.map_->map_points_.at(curr->window_ids_[k]);
            n_pos.push_back(p->pos_.x), n_pos.push_back(p->pos_.y), n_pos.push_back(p->pos_.z);
            n_desc.insert(n_desc.end(), p->descriptor_.data, p->descriptor_.data + 32);
            for (int r = 0; r < 3; ++r) n_norm.push_back(p->norm_.at<double>(r, 0));
            n_rgb.insert(n_rgb.end(), p->color_.begin(), p->color_.end());
        }
        dump(out, n_pos);
        dump(out, n_desc);
        dump(out, n_norm);
        dump(out, n_rgb);
        vector<int> conn_after;
        for (const vo::Frame::Ptr& fr : st.frames_buff_)
            for (int k = 0; k < (int)fr->keypoints_.size(); ++k) {
                const auto c = fr->inliers_to_mappt_connections_.find(k);
                if (c == fr->inliers_to_mappt_connections_.end()) {
                    conn_after.push_back(-1);
                    continue;
                }
                const int id = c->second.pt_map_idx;
                if (id == gone_id)
                    conn_after.push_back(-2);
                else if (scene_index.count(id))
                    conn_after.push_back(scene_index[id]);
                else if (new_index.count(id) && c->second.pt_ref_idx == -1)
                    conn_after.push_back(1000000 + new_index[id]);
                else
                    conn_after.push_back(-3);
            }
        dump(out, conn_after);
        int still = 0;
        for (const auto& kv : st.map_->map_points_) still += scene_index.count(kv.first) ? 1 : 0;
        mvo_check(mvo_map_size(hot_path_ctx(), st.dev_map_.handle(), &resident_after), "mvo_map_size");
        dump(out, vector<int>{still, resident_before, resident_after});
    } catch (const std::exception& e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
