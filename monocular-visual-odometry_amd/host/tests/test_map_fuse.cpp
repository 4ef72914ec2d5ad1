// host/tests/test_map_fuse.cpp -- drives the mirror of the fusion of duplicate map points (my_slam/vo/map_fuse.h) and dumps the
// results for tests/test_map_fuse_host.py.
//   test_map_fuse <scene.bin> <out.bin> [key=value ...]
// scene.bin: int32 n_pts, n_frames (<= 20), cols, rows; double fx, fy, cx, cy; float pos[n_pts*3]; uint8 desc[n_pts*32]; int32
//            matched_times[n_pts], visible_times[n_pts]; then per frame, oldest first: int32 nk; double T_w_c[16]; float
//            kpt[nk*2]; uint8 desc[nk*32]; int32 octave[nk]; int32 conn[nk] (the scene index of the map point keypoint k is
//            connected to, -1: none, -2: a point that is no longer in the map).  key=value pairs are set in basics::Config
//            before anything is latched.  Every frame's connection map is filled in a scrambled keypoint order.
// out.bin (each a uint64 count followed by the items): [mapPointFuse()] (int32); for every position of MapOnDevice::order()
// before the call the index of that point in the scene (int32); collectFuseFrames: the keypoints per frame (int32), the
// connections as map rows (int32), the scales (f32); what fuseMapPoints recorded: the set-up (f64), replaced_by, added, counts
// (int32); the scene indices of MapOnDevice::order() after the call and of Map::map_points_ (sorted); per keypoint of every
// frame the scene index its connection names after the call (-1: none, -2: the departed point, -3: an id that is in neither);
// per scene point matched_times_ and visible_times_ (-1 for a point that left the map); the number of resident rows
// (mvo_map_size).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>

#include "my_slam/vo/map_fuse.h"

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
    vector<int> matched(n_pts), visible(n_pts);
    rd(in, pos.data(), pos.size());
    rd(in, desc.data(), desc.size());
    rd(in, matched.data(), matched.size());
    rd(in, visible.data(), visible.size());
    try {
        dump(out, vector<int>{vo::mapPointFuse() ? 1 : 0});
        vo::TrackingState st;
        std::map<int, int> scene_index;  // MapPoint::id_ -> index in the scene
        vector<int> id_of(n_pts);
        vector<vo::MapPoint::Ptr> points;
        for (int i = 0; i < n_pts; ++i) {
            cv::Mat d(1, 32, CV_8UC1), norm(3, 1, CV_64FC1);
            std::memcpy(d.data, &desc[32 * (size_t)i], 32);
            for (int r = 0; r < 3; ++r) norm.at<double>(r, 0) = r == 2 ? 1.0 : 0.0;
            vo::MapPoint::Ptr p(new vo::MapPoint(cv::Point3f(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]), d, norm));
            p->matched_times_ = matched[i], p->visible_times_ = visible[i];
            scene_index[p->id_] = i;
            id_of[i] = p->id_;
            points.push_back(p);
            st.map_->insertMapPoint(p);
        }
        const int gone_id = vo::MapPoint::factory_id() + 1000;  // a point culled long ago
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
            }
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
        dump(out, order);
        {
            const vo::FuseFrames ff = vo::collectFuseFrames(st.frames_buff_, st.dev_map_.order());
            dump(out, ff.n);
            dump(out, ff.conn);
            dump(out, ff.scale);
        }
        vo::Frame::Ptr probe = vo::Frame::createFrame(img);
        vo::fuseMapPoints(st, K, probe);
        dump(out, probe->fuse_setup_);
        dump(out, probe->fuse_replaced_by_);
        dump(out, probe->fuse_added_);
        dump(out, probe->fuse_counts_);
        vector<int> after, in_map;
        for (const vo::MapPoint::Ptr& p : st.dev_map_.order()) after.push_back(scene_index[p->id_]);
        for (const auto& kv : st.map_->map_points_) in_map.push_back(scene_index[kv.first]);
        std::sort(in_map.begin(), in_map.end());
        dump(out, after);
        dump(out, in_map);
        vector<int> conn_after;
        for (const vo::Frame::Ptr& fr : st.frames_buff_)
            for (int k = 0; k < (int)fr->keypoints_.size(); ++k) {
                const auto c = fr->inliers_to_mappt_connections_.find(k);
                if (c == fr->inliers_to_mappt_connections_.end()) {
                    conn_after.push_back(-1);
                    continue;
                }
                const int id = c->second.pt_map_idx;
                const bool here = st.map_->map_points_.count(id) != 0;
                conn_after.push_back(id == gone_id ? -2 : (here ? scene_index[id] : -3));
            }
        dump(out, conn_after);
        vector<int> m_after(n_pts, -1), v_after(n_pts, -1);
        for (const auto& kv : st.map_->map_points_)
            m_after[scene_index[kv.first]] = kv.second->matched_times_, v_after[scene_index[kv.first]] = kv.second->visible_times_;
        dump(out, m_after);
        dump(out, v_after);
        int resident = -1;
        mvo_check(mvo_map_size(hot_path_ctx(), st.dev_map_.handle(), &resident), "mvo_map_size");
        dump(out, vector<int>{resident});
    } catch (const std::exception& e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
