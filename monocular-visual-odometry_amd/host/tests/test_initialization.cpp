// host/tests/test_initialization.cpp -- drives the initialisation mirror (my_slam/vo/initialization.h) the way
// VisualOdometry::addFrame does in its DOING_INITIALIZATION state (src/vo/vo_addFrame.cpp:36-69) and checks it against
// a direct mvo_init_two_view on the same matches, for tests/test_host_initialization.py.
//   test_initialization <scene.bin>
// scene.bin: int32 N[3]; double K[4]; double T_w_ref[16]; then for the first keyframe, a frame with a tiny baseline and
//            a frame with a large one: float kp[N*2]; uint8 desc[N*32]
// Sequence: the tiny-baseline frame (must not initialise), the large-baseline frame (must), the tiny-baseline frame
// again against the first keyframe (must leave the map as it is).  Prints one line of counts and "INIT-OK".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "my_slam/vo/initialization.h"

using namespace my_slam;

template <class T>
static void rd(std::ifstream& f, T* p, size_t n) {
    if (!f.read(reinterpret_cast<char*>(p), (std::streamsize)(n * sizeof(T)))) {
        fprintf(stderr, "short scene file\n");
        exit(2);
    }
}

#define CHECK(cond)                                              \
    do {                                                         \
        if (!(cond)) {                                           \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);   \
            return 1;                                            \
        }                                                        \
    } while (0)

static vo::Frame::Ptr copyFeatures(const vo::Frame::Ptr& src) {
    vo::Frame::Ptr f = vo::Frame::createFrame(cv::Mat());
    f->keypoints_ = src->keypoints_;
    f->descriptors_ = src->descriptors_;
    return f;
}

static bool samePose(const cv::Mat& a, const cv::Mat& b) { return std::memcmp(a.ptr<double>(0), b.ptr<double>(0), 128) == 0; }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    int N[3];
    rd(in, N, 3);
    double K4[4], Tr[16];
    rd(in, K4, 4);
    rd(in, Tr, 16);
    try {
        cv::Mat K = cv::Mat::eye(3, 3, CV_64FC1);
        K.at<double>(0, 0) = K4[0];
        K.at<double>(1, 1) = K4[1];
        K.at<double>(0, 2) = K4[2];
        K.at<double>(1, 2) = K4[3];
        vo::Frame::Ptr fr[3];
        for (int k = 0; k < 3; ++k) {
            fr[k] = vo::Frame::createFrame(cv::Mat());
            vector<float> xy(2 * (size_t)N[k]);
            rd(in, xy.data(), xy.size());
            for (int i = 0; i < N[k]; ++i) fr[k]->keypoints_.push_back(cv::KeyPoint(xy[2 * i], xy[2 * i + 1], 31));
            fr[k]->descriptors_.create(N[k], 32, CV_8UC1);
            rd(in, fr[k]->descriptors_.data, (size_t)N[k] * 32);
        }
        const vo::Frame::Ptr ref = fr[0], tiny = fr[1], wide = fr[2];
        for (int i = 0; i < 16; ++i) ref->T_w_c_.at<double>(i / 4, i % 4) = Tr[i];
        vo::TrackingState st;
        st.map_->insertKeyFrame(ref);  // the BLANK branch: addKeyFrame_(curr_)
        st.ref_ = ref;

        // -- a tiny baseline: not initialised, the pose of the first keyframe, nothing in the map
        CHECK(!vo::initializeWithFrame(st, tiny, K));
        CHECK(samePose(tiny->T_w_c_, ref->T_w_c_));
        CHECK(st.map_->map_points_.empty() && st.map_->keyframes_.size() == 1 && st.ref_ == ref);

        // -- a large baseline: initialised
        CHECK(vo::initializeWithFrame(st, wide, K));
        CHECK(!st.map_->map_points_.empty() && st.map_->keyframes_.size() == 2 && st.ref_ == wide);
        CHECK(st.map_->hasKeyFrame(ref->id_) && st.map_->hasKeyFrame(wide->id_));
        // the same matches through the C-ABI: the pose and the kept, scaled points bit for bit
        vector<cv::Point2f> pts1, pts2;
        geometry::extractPtsFromMatches(ref->keypoints_, wide->keypoints_, wide->matches_with_ref_, pts1, pts2);
        const int n = (int)pts1.size();
        CHECK(n > 0);
        vector<int32_t> ie(n), ih(n), m3(n);
        vector<float> sp((size_t)15 * n), p3((size_t)3 * n);
        vector<double> ang(n);
        mvo_init_poses poses{};
        poses.inliers_e = ie.data();
        poses.inliers_h = ih.data();
        poses.cap_inliers = n;
        poses.pts3d = sp.data();
        poses.cap_pts = 5 * n;
        mvo_init_result res{};
        res.matches_for_3d = m3.data();
        res.pts3d_in_curr = p3.data();
        res.angles = ang.data();
        res.cap = n;
        const mvo_init_params prm = {1.0, 20.0, 0.8, 15, 50.0, 2.0};  // config/config.yaml:105-113
        mvo_check(mvo_init_two_view(hot_path_ctx(), &pts1[0].x, &pts2[0].x, n, K4[0], K4[1], K4[2], K4[3], 0.999, 1.0, 3.0,
                                    0.995, 1.0, Tr, &prm, &poses, &res),
                  "mvo_init_two_view");
        CHECK(res.good && res.scaled && res.n_kept >= 20);
        CHECK(std::memcmp(wide->T_w_c_.ptr<double>(0), res.T_w_c, 128) == 0);
        CHECK((int)wide->inliers_pts3d_.size() == res.n_kept);
        CHECK(std::memcmp(&wide->inliers_pts3d_[0].x, res.pts3d_in_curr, (size_t)res.n_kept * 12) == 0);
        CHECK((int)wide->inliers_matches_for_3d_.size() == res.n_kept && (int)wide->inliers_matches_with_ref_.size() == res.n_slot_inliers);
        for (int i = 0; i < res.n_kept; ++i) {
            CHECK(wide->inliers_matches_for_3d_[i].queryIdx == wide->matches_with_ref_[res.matches_for_3d[i]].queryIdx);
            CHECK(wide->triangulation_angles_of_inliers_[i] == res.angles[i]);
        }
        CHECK(st.map_->map_points_.size() == (size_t)res.n_kept);  // no point of the first keyframe was in the map yet
        CHECK(wide->inliers_to_mappt_connections_.size() == (size_t)res.n_kept);

        // -- the tiny baseline against the first keyframe again: the map stays as it is
        const size_t n_map = st.map_->map_points_.size();
        vo::Frame::Ptr tiny2 = copyFeatures(tiny);
        st.ref_ = ref;
        CHECK(!vo::initializeWithFrame(st, tiny2, K));
        CHECK(samePose(tiny2->T_w_c_, ref->T_w_c_));
        CHECK(st.map_->map_points_.size() == n_map && st.map_->keyframes_.size() == 2 && st.ref_ == ref);
        printf("matches %d slot %d inliers %d kept %d map %zu tiny_matches %zu tiny_kept %zu\n", n, res.slot, res.n_slot_inliers,
               res.n_kept, n_map, tiny->matches_with_ref_.size(), tiny->inliers_matches_for_3d_.size());
        printf("INIT-OK\n");
    } catch (const std::exception& e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
