// host/tests/test_map_refresh.cpp -- drives the mirror of the map-point refresh (my_slam/vo/map_refresh.h) and dumps the results
// for tests/test_map_refresh_host.py.
//   test_map_refresh <scene.bin> <out.bin> [key=value ...]
// scene.bin: int32 n_pts, n_frames (<= 20), nk; float pos[n_pts*3]; uint8 desc[n_pts*32]; then per frame, oldest first:
//            double T_w_c[16]; uint8 kdesc[nk*32]; int32 conn[nk] (the scene index of the map point keypoint k is connected to,
//            -1: none, -2: a point that is no longer in the map).  key=value pairs are set in basics::Config before anything is
//            latched.  Every frame's connection map is filled in a scrambled keypoint order.
// out.bin (each a uint64 count followed by the items): [mapPointRefresh()] (int32); for every position of MapOnDevice::order()
// the index of that point in the scene (int32); collectObservations: obs_start (int32), obs_desc, obs_cam (f64); what
// refreshMapPoints recorded: choice (int32), norm (f64); then, per position of order(): MapPoint::descriptor_, MapPoint::norm_
// (f64), MapOnDevice's host copy of the descriptors, and the resident positions (f32) and descriptors (mvo_debug_get_map).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>

#include "my_slam/vo/map_refresh.h"

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
    vector<float> pos(3 * (size_t)n_pts);
    vector<unsigned char> desc(32 * (size_t)n_pts);
    rd(in, pos.data(), pos.size());
    rd(in, desc.data(), desc.size());
    try {
        const int flag = vo::mapPointRefresh() ? 1 : 0;
        dump(out, &flag, 1);
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
        cv::Mat img(8, 8, CV_8UC3);
        for (int f = 0; f < n_frames; ++f) {
            vo::Frame::Ptr fr = vo::Frame::createFrame(img);
            double T[16];
            rd(in, T, 16);
            for (int i = 0; i < 16; ++i) fr->T_w_c_.at<double>(i / 4, i % 4) = T[i];
            fr->descriptors_.create(nk, 32, CV_8UC1);
            rd(in, fr->descriptors_.data, (size_t)nk * 32);
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
        dump(out, o.obs_desc.data(), o.obs_desc.size());
        dump(out, o.obs_cam.data(), o.obs_cam.size());
        vo::Frame::Ptr probe = vo::Frame::createFrame(img);
        vo::refreshMapPoints(st, probe);
        dump(out, probe->refresh_choice_.data(), probe->refresh_choice_.size());
        dump(out, probe->refresh_norm_.data(), probe->refresh_norm_.size());
        const int n = (int)st.dev_map_.order().size();
        vector<unsigned char> pdesc;
        vector<double> pnorm;
        for (const vo::MapPoint::Ptr& p : st.dev_map_.order()) {
            pdesc.insert(pdesc.end(), p->descriptor_.data, p->descriptor_.data + 32);
            for (int r = 0; r < 3; ++r) pnorm.push_back(p->norm_.at<double>(r, 0));
        }
        dump(out, pdesc.data(), pdesc.size());
        dump(out, pnorm.data(), pnorm.size());
        dump(out, st.dev_map_.descriptors().data(), st.dev_map_.descriptors().size());
        vector<float> rpos(3 * (size_t)n + 1);
        vector<unsigned char> rdesc(32 * (size_t)n + 1);
        int got = 0;
        mvo_check(mvo_debug_get_map(hot_path_ctx(), st.dev_map_.handle(), rpos.data(), rdesc.data(), n, &got), "mvo_debug_get_map");
        dump(out, rpos.data(), 3 * (size_t)got);
        dump(out, rdesc.data(), 32 * (size_t)got);
    } catch (const std::exception& e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
