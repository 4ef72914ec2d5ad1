// my_slam/vo/vo.h -- VisualOdometry, the state machine of the reference (include/my_slam/vo/vo.h:36-54,
// src/vo/vo_addFrame.cpp:10-142) on the mirrored Frame / Map:
//   BLANK                 the first frame: identity pose, first keyframe, -> DOING_INITIALIZATION
//   DOING_INITIALIZATION  initializeWithFrame (my_slam/vo/initialization.h) against the first keyframe; a frame that
//                         does not pass isVoGoodToInit takes the first keyframe's pose and nothing else changes (a
//                         frame whose E / H rule picks no solution, DESIGN.md section 2 deviation 12, is one of
//                         them); the frame that passes fills the map, becomes the second keyframe, -> DOING_TRACKING
//   DOING_TRACKING        trackFrame (my_slam/vo/tracking_loop.h); a frame whose PnP fails takes the previous frame's
//                         pose and the state stays (the reference declares LOST but never enters it, and has no
//                         re-initialisation)
// Differences to the reference's class: the mirrored Frame has no camera_, so the constructor takes K (the reference
// reads curr_->camera_->K_, vo_addFrame.cpp:18); the members live in a TrackingState (the struct the two branch
// mirrors work on), vo_state_ and the enum are public so that callers can follow the transitions, and last_ tells what
// the last addFrame did (the reference prints it).  Every frame enters frames_buff_ exactly once, as pushFrameToBuff_
// at vo_addFrame.cpp:13 does it: here for the first frame, inside initializeWithFrame / trackFrame for the others.
#ifndef MY_SLAM_VO_H
#define MY_SLAM_VO_H
#include "my_slam/vo/initialization.h"
#include "my_slam/vo/tracking_loop.h"

namespace my_slam {
namespace vo {

class VisualOdometry {
public:
    typedef std::shared_ptr<VisualOdometry> Ptr;
    enum VOState { BLANK, DOING_INITIALIZATION, DOING_TRACKING };

    struct LastFrame {  // what the last addFrame did
        VOState state_before = BLANK;
        bool is_keyframe = false;   // inserted as a keyframe (the first frame, the frame that initialised, tracking keyframes)
        bool initialized = false;   // the frame that took DOING_INITIALIZATION to DOING_TRACKING
        bool is_pnp_good = false;   // DOING_TRACKING only
        InitReport init;            // DOING_INITIALIZATION only
    };

    explicit VisualOdometry(const cv::Mat& K) : vo_state_(BLANK), K_(K.clone()) {}

    // Add a new frame to the visual odometry system and compute its pose.
    void addFrame(Frame::Ptr frame) {
        const Frame::Ptr& curr = frame;
        if (curr->keypoints_.empty() && curr->descriptors_.rows == 0) {  // vo_addFrame.cpp:24-25
            curr->calcKeyPoints();
            curr->calcDescriptors();
        }
        prev_ref_ = st_.ref_;
        last_ = LastFrame();
        last_.state_before = vo_state_;
        if (vo_state_ == BLANK) {
            st_.pushFrameToBuff(curr);
            curr->T_w_c_ = cv::Mat::eye(4, 4, CV_64FC1);
            vo_state_ = DOING_INITIALIZATION;
            st_.map_->insertKeyFrame(curr);  // addKeyFrame_: curr becomes the ref_
            st_.ref_ = curr;
            last_.is_keyframe = true;
        } else if (vo_state_ == DOING_INITIALIZATION) {
            if (initializeWithFrame(st_, curr, K_, &last_.init)) {
                vo_state_ = DOING_TRACKING;
                last_.is_keyframe = last_.initialized = true;
            }
        } else {
            last_.is_pnp_good = trackFrame(st_, curr, K_, &last_.is_keyframe);
        }
        st_.prev_ = curr;
    }

    bool isInitialized() const { return vo_state_ == DOING_TRACKING; }
    Frame::Ptr getPrevRef() const { return prev_ref_; }
    Map::Ptr getMap() const { return st_.map_; }
    Frame::Ptr getRef() const { return st_.ref_; }
    const std::deque<Frame::Ptr>& getFramesBuff() const { return st_.frames_buff_; }
    const MapOnDevice& getMapOnDevice() const { return st_.dev_map_; }
    const LastFrame& last() const { return last_; }

    VOState vo_state_;

private:
    TrackingState st_;  // map_, frames_buff_ (kBuffSize_ = 20), ref_, prev_ (vo.h:58-86)
    Frame::Ptr prev_ref_;
    cv::Mat K_;
    LastFrame last_;
};

}  // namespace vo
}  // namespace my_slam
#endif
