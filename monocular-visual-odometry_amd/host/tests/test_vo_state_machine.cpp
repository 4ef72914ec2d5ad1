// host/tests/test_vo_state_machine.cpp -- drives my_slam::vo::VisualOdometry (my_slam/vo/vo.h = the reference's class,
// vo.h:36-54 / vo_addFrame.cpp:10-142) over feature-level frames, for tests/test_host_vo_state_machine.py.
//   test_vo_state_machine <scene.bin>
// scene.bin: int32 cols, rows; double K[4]; int32 N[7]; then seven frames, each float kp[N*2]; uint8 desc[N*32]:
//            a first view, a tiny-baseline view, a wide-baseline view and two further views of the same points, then a
//            first and a wide-baseline view of points on a plane.
// Three sequences, each on a VisualOdometry of its own:
//   1  first, tiny (rejected), wide (initialises; held to mvo_init_two_view on the same matches), the two further views
//      (tracked)
//   2  the plane: initialises through a homography slot
//   3  first and 30 copies of the tiny view: all rejected, the frame buffer stops at 20
// Prints one line of counts and "VO-OK".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "my_slam/vo/vo.h"

using namespace my_slam;
typedef vo::VisualOdometry VO;

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

static int g_cols, g_rows;

static vo::Frame::Ptr copyFeatures(const vo::Frame::Ptr& src) {
    vo::Frame::Ptr f = vo::Frame::createFrame(cv::Mat(g_rows, g_cols, CV_8UC3));
    f->keypoints_ = src->keypoints_;
    f->descriptors_ = src->descriptors_;
    return f;
}

static bool isIdentity(const cv::Mat& T) {
    for (int i = 0; i < 16; ++i)
        if (T.at<double>(i / 4, i % 4) != (i / 4 == i % 4 ? 1.0 : 0.0)) return false;
    return true;
}
static bool samePose(const cv::Mat& a, const cv::Mat& b) { return std::memcmp(a.ptr<double>(0), b.ptr<double>(0), 128) == 0; }

// the frame sits in the buffer exactly once, as the newest entry
static bool pushedOnce(const VO& v, const vo::Frame::Ptr& f) {
    const std::deque<vo::Frame::Ptr>& b = v.getFramesBuff();
    return std::count(b.begin(), b.end(), f) == 1 && b.back() == f;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    int size[2], N[7];
    double K4[4];
    rd(in, size, 2);
    rd(in, K4, 4);
    rd(in, N, 7);
    g_cols = size[0];
    g_rows = size[1];
    try {
        cv::Mat K = cv::Mat::eye(3, 3, CV_64FC1);
        K.at<double>(0, 0) = K4[0];
        K.at<double>(1, 1) = K4[1];
        K.at<double>(0, 2) = K4[2];
        K.at<double>(1, 2) = K4[3];
        vo::Frame::Ptr fr[7];
        for (int k = 0; k < 7; ++k) {
            fr[k] = vo::Frame::createFrame(cv::Mat(g_rows, g_cols, CV_8UC3));
            vector<float> xy(2 * (size_t)N[k]);
            rd(in, xy.data(), xy.size());
            for (int i = 0; i < N[k]; ++i) fr[k]->keypoints_.push_back(cv::KeyPoint(xy[2 * i], xy[2 * i + 1], 31));
            fr[k]->descriptors_.create(N[k], 32, CV_8UC1);
            rd(in, fr[k]->descriptors_.data, (size_t)N[k] * 32);
        }
        const vo::Frame::Ptr first = fr[0], tiny = fr[1], wide = fr[2];

        // ---- 1: BLANK -> DOING_INITIALIZATION -> (rejected) -> DOING_TRACKING -> tracked
        VO::Ptr v(new VO(K));
        CHECK(v->vo_state_ == VO::BLANK && !v->isInitialized() && v->getMap()->keyframes_.empty());
        for (int i = 0; i < 16; ++i) first->T_w_c_.at<double>(i / 4, i % 4) = 0.5 + i;  // addFrame must overwrite it
        v->addFrame(first);
        CHECK(v->vo_state_ == VO::DOING_INITIALIZATION && !v->isInitialized());
        CHECK(isIdentity(first->T_w_c_) && v->getMap()->keyframes_.size() == 1 && v->getMap()->hasKeyFrame(first->id_));
        CHECK(v->getRef() == first && v->getMap()->map_points_.empty() && pushedOnce(*v, first));
        CHECK(v->last().state_before == VO::BLANK && v->last().is_keyframe && !v->last().initialized);
        CHECK((int)first->keypoints_.size() == N[0]);  // features that are there are not computed again

        v->addFrame(tiny);  // rejected: the first keyframe's pose bit for bit, one keyframe, an empty map
        CHECK(v->vo_state_ == VO::DOING_INITIALIZATION && !v->isInitialized());
        CHECK(samePose(tiny->T_w_c_, first->T_w_c_) && isIdentity(tiny->T_w_c_));
        CHECK(v->getMap()->keyframes_.size() == 1 && v->getMap()->map_points_.empty() && v->getRef() == first);
        CHECK(pushedOnce(*v, tiny) && v->getFramesBuff().size() == 2);
        CHECK(v->last().state_before == VO::DOING_INITIALIZATION && !v->last().is_keyframe && !v->last().initialized && !v->last().init.good);
        CHECK(tiny->inliers_to_mappt_connections_.empty());
        const int tiny_matches = (int)tiny->matches_with_ref_.size();
        first->clearNoUsed();  // what run_vo does after every frame: the first keyframe keeps what the matching needs
        tiny->clearNoUsed();
        CHECK((int)first->keypoints_.size() == N[0] && first->descriptors_.rows == N[0]);

        v->addFrame(wide);  // initialises
        const vo::InitReport rep = v->last().init;
        CHECK(v->vo_state_ == VO::DOING_TRACKING && v->isInitialized());
        CHECK(v->last().initialized && v->last().is_keyframe && rep.good && rep.criteria[0] && rep.criteria[1] && rep.criteria[2]);
        CHECK(v->getMap()->keyframes_.size() == 2 && v->getMap()->hasKeyFrame(first->id_) && v->getMap()->hasKeyFrame(wide->id_));
        CHECK(v->getRef() == wide && v->getPrevRef() == first && pushedOnce(*v, wide) && v->getFramesBuff().size() == 3);
        CHECK(v->getMap()->map_points_.size() == (size_t)rep.n_kept && rep.n_kept >= 20);
        // the same matches through the C-ABI: the pose and the kept, scaled points bit for bit
        vector<cv::Point2f> pts1, pts2;
        geometry::extractPtsFromMatches(first->keypoints_, wide->keypoints_, wide->matches_with_ref_, pts1, pts2);
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
        const double I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        mvo_check(mvo_init_two_view(hot_path_ctx(), &pts1[0].x, &pts2[0].x, n, K4[0], K4[1], K4[2], K4[3], 0.999, 1.0, 3.0, 0.995,
                                    1.0, I4, &prm, &poses, &res),
                  "mvo_init_two_view");
        CHECK(res.good && res.scaled && res.slot == rep.slot && res.n_kept == rep.n_kept && res.n_slot_inliers == rep.n_slot_inliers);
        CHECK(std::memcmp(wide->T_w_c_.ptr<double>(0), res.T_w_c, 128) == 0);
        CHECK((int)wide->inliers_pts3d_.size() == res.n_kept);
        CHECK(std::memcmp(&wide->inliers_pts3d_[0].x, res.pts3d_in_curr, (size_t)res.n_kept * 12) == 0);
        CHECK((int)wide->inliers_matches_for_3d_.size() == res.n_kept && (int)wide->inliers_matches_with_ref_.size() == res.n_slot_inliers);
        for (int i = 0; i < res.n_kept; ++i) {
            const cv::DMatch& m = wide->matches_with_ref_[res.matches_for_3d[i]];
            CHECK(wide->inliers_matches_for_3d_[i].queryIdx == m.queryIdx && wide->inliers_matches_for_3d_[i].trainIdx == m.trainIdx);
        }
        CHECK(wide->inliers_to_mappt_connections_.size() == (size_t)res.n_kept);
        const cv::Mat pose_wide = wide->T_w_c_.clone();
        wide->clearNoUsed();

        int tracked_matches[2];
        for (int k = 0; k < 2; ++k) {  // the two further views: tracked, the state stays
            const vo::Frame::Ptr& f = fr[3 + k];
            v->addFrame(f);
            CHECK(v->vo_state_ == VO::DOING_TRACKING && v->last().state_before == VO::DOING_TRACKING && v->last().is_pnp_good);
            CHECK(!v->last().initialized && pushedOnce(*v, f) && (int)v->getFramesBuff().size() == 4 + k);
            CHECK(!samePose(f->T_w_c_, pose_wide) && f->matches_with_map_.size() >= 100);
            tracked_matches[k] = (int)f->matches_with_map_.size();
            f->clearNoUsed();
        }
        CHECK(v->getMap()->keyframes_.size() >= 2);

        // ---- 2: points on a plane initialise through a homography slot
        VO::Ptr vp(new VO(K));
        vp->addFrame(fr[5]);
        vp->addFrame(fr[6]);
        const vo::InitReport rp = vp->last().init;
        CHECK(vp->isInitialized() && vp->last().initialized && rp.good && rp.slot >= 1 && rp.slot <= 4);
        CHECK(vp->getMap()->keyframes_.size() == 2 && vp->getMap()->map_points_.size() == (size_t)rp.n_kept && rp.n_kept >= 20);
        CHECK((int)fr[6]->inliers_matches_with_ref_.size() == rp.n_slot_inliers);

        // ---- 3: 30 rejected frames: the buffer holds the newest 20, each once; nothing else moves
        VO::Ptr vr(new VO(K));
        const vo::Frame::Ptr first3 = copyFeatures(first);
        vr->addFrame(first3);
        vector<vo::Frame::Ptr> fed = {first3};
        for (int k = 0; k < 30; ++k) {
            vo::Frame::Ptr f = copyFeatures(tiny);
            vr->addFrame(f);
            fed.push_back(f);
            CHECK(vr->vo_state_ == VO::DOING_INITIALIZATION && !vr->last().init.good && isIdentity(f->T_w_c_));
            CHECK(vr->getFramesBuff().size() == std::min<size_t>(fed.size(), 20) && pushedOnce(*vr, f));
            f->clearNoUsed();
        }
        CHECK(vr->getFramesBuff().size() == 20 && vo::TrackingState::kBuffSize_ == 20);
        for (size_t i = 0; i < 20; ++i) CHECK(vr->getFramesBuff()[i] == fed[fed.size() - 20 + i]);
        CHECK(vr->getMap()->keyframes_.size() == 1 && vr->getMap()->map_points_.empty() && vr->getRef() == first3 && !vr->isInitialized());

        printf("tiny_matches %d matches %d slot %d inliers %d kept %d map %zu tracked0 %d tracked1 %d plane_slot %d plane_kept %d buffer %zu\n",
               tiny_matches, n, res.slot, res.n_slot_inliers, res.n_kept, v->getMap()->map_points_.size(), tracked_matches[0],
               tracked_matches[1], rp.slot, rp.n_kept, vr->getFramesBuff().size());
        printf("VO-OK\n");
    } catch (const std::exception& e) {
        fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
    return 0;
}
