// host/tests/test_local_map.cpp -- drives the mirror of the second search of a tracked frame (my_slam/vo/local_map.h) and dumps
// the results for tests/test_local_map_host.py.
//   test_local_map <scene.bin> <out.bin> [key=value ...]
// scene.bin: int32 n (map points), nk (keypoints), nc (connections), nm (first-pass inlier matches), cols, rows; double fx, fy,
//            cx, cy; double T_w_c[16] (the optimised pose of the frame); double T_prev[16]; per map point float pos[3], float
//            normal[3], float max_dist, uint8 desc[32]; float kpt[nk*2]; int32 octave[nk]; uint8 kdesc[nk*32]; int32 conn[nc*2]
//            (keypoint, map point id); int32 match[nm] (the keypoints of the first pass's inlier matches, in their order).  The
//            map points get the ids 0..n-1 in file order.  key=value pairs are set in basics::Config before anything is latched.
// out.bin (each a uint64 count followed by the items): [trackingLocalMap(), applied, outcome] (int32); the ids of the map in the
// order of the resident copy (int32); what trackLocalMap recorded: the set-up, the pose going in (f64), the skip mask, the
// keypoints' levels (int32), the new matches (16 bytes each), the second optimisation's points, pixels, inv_sigma2 (f32), pose
// (f64), info (int32), chi2 (f64), outlier flags; then the frame afterwards: T_w_c (f64), the connections sorted by keypoint
// (keypoint, map point id: int32), the keypoints of matches_with_map_ (int32), and matched_times_ and visible_times_ of every map
// point by id (int32).
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "my_slam/vo/local_map.h"

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
template <class T>
static void dump(std::ofstream& o, const vector<T>& v) {
    dump(o, v.data(), v.size());
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
    int hdr[6];
    rd(in, hdr, 6);
    const int n = hdr[0], nk = hdr[1], nc = hdr[2], nm = hdr[3];
    double k4[4], T[16], Tp[16];
    rd(in, k4, 4);
    rd(in, T, 16);
    rd(in, Tp, 16);
    cv::Mat K = cv::Mat::eye(3, 3, CV_64FC1);
    K.at<double>(0, 0) = k4[0], K.at<double>(1, 1) = k4[1], K.at<double>(0, 2) = k4[2], K.at<double>(1, 2) = k4[3];
    try {
        vo::TrackingState st;
        vo::MapPoint::factory_id() = 0;
        vector<vo::MapPoint::Ptr> by_id;
        for (int i = 0; i < n; ++i) {
            float v[7];
            rd(in, v, 7);
            cv::Mat desc(1, 32, CV_8UC1), norm(3, 1, CV_64FC1);
            rd(in, desc.data, 32);
            for (int r = 0; r < 3; ++r) norm.at<double>(r, 0) = (double)v[3 + r];
            vo::MapPoint::Ptr p(new vo::MapPoint(cv::Point3f(v[0], v[1], v[2]), desc, norm));
            p->max_dist_ = v[6];
            st.map_->insertMapPoint(p);
            by_id.push_back(p);
        }
        vector<float> kpt(2 * (size_t)nk);
        vector<int> octave(nk), conn(2 * (size_t)nc), match(nm);
        rd(in, kpt.data(), kpt.size());
        rd(in, octave.data(), octave.size());
        cv::Mat img(hdr[5], hdr[4], CV_8UC3);
        vo::Frame::Ptr curr = vo::Frame::createFrame(img), prev = vo::Frame::createFrame(img);
        curr->descriptors_.create(nk > 0 ? nk : 1, 32, CV_8UC1);
        curr->descriptors_.rows = nk;
        for (int k = 0; k < nk; ++k) rd(in, curr->descriptors_.ptr<unsigned char>(k), 32);
        rd(in, conn.data(), conn.size());
        rd(in, match.data(), match.size());
        for (int i = 0; i < 16; ++i) curr->T_w_c_.at<double>(i / 4, i % 4) = T[i], prev->T_w_c_.at<double>(i / 4, i % 4) = Tp[i];
        curr->keypoints_.resize(nk);
        for (int k = 0; k < nk; ++k) {
            curr->keypoints_[k].pt = cv::Point2f(kpt[2 * k], kpt[2 * k + 1]);
            curr->keypoints_[k].octave = octave[k];
        }
        for (int c = 0; c < nc; ++c) curr->inliers_to_mappt_connections_[conn[2 * c]] = vo::PtConn{-1, conn[2 * c + 1]};
        for (int i = 0; i < nm; ++i) curr->matches_with_map_.push_back(cv::DMatch(i, match[i], 0, 0.f));
        st.prev_ = prev;
        vo::trackLocalMap(st, curr, K);
        const int head[3] = {vo::trackingLocalMap() ? 1 : 0, curr->local_map_applied_, curr->local_map_outcome_};
        dump(out, head, 3);
        vector<int> order;
        for (const vo::MapPoint::Ptr& p : st.dev_map_.order()) order.push_back(p->id_);
        dump(out, order);
        dump(out, curr->local_map_setup_);
        dump(out, curr->local_map_init_);
        dump(out, curr->local_map_skip_);
        dump(out, curr->local_map_t_level_);
        static_assert(sizeof(cv::DMatch) == 16, "record layout");
        dump(out, curr->local_map_matches_);
        dump(out, curr->local_map_p3_);
        dump(out, curr->local_map_p2_);
        dump(out, curr->local_map_sigma_);
        dump(out, curr->local_map_T_w_c_);
        dump(out, curr->local_map_info_);
        dump(out, curr->local_map_chi2_);
        dump(out, curr->local_map_outlier_);
        vector<double> Tout;
        for (int i = 0; i < 16; ++i) Tout.push_back(curr->T_w_c_.at<double>(i / 4, i % 4));
        dump(out, Tout);
        vector<std::pair<int, int>> cs;
        for (const auto& kv : curr->inliers_to_mappt_connections_) cs.push_back({kv.first, kv.second.pt_map_idx});
        std::sort(cs.begin(), cs.end());
        vector<int> flat, kept, times;
        for (const auto& c : cs) flat.push_back(c.first), flat.push_back(c.second);
        dump(out, flat);
        for (const cv::DMatch& d : curr->matches_with_map_) kept.push_back(d.trainIdx);
        dump(out, kept);
        for (const vo::MapPoint::Ptr& p : by_id) times.push_back(p->matched_times_), times.push_back(p->visible_times_);
        dump(out, times);
    } catch (const std::exception& e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
