"""tests/vo_chain_init.py -- TEST AID: the run of host/driver/run_vo.cpp with `init_from_images: 1` composed from the CPU
oracle and the restatements, the way the reference's state machine chains it (src/vo/vo_addFrame.cpp:10-142):

    vo_addFrame.cpp:30-35       BLANK: the first frame is the first keyframe at the identity
    vo_addFrame.cpp:36-69       DOING_INITIALIZATION: matchFeatures with the first keyframe, estimateMotionAnd3DPoints_ and
                                isVoGoodToInit_ (= finish_restate.Restatement().init_two_view, the composition of the
                                restatements mvo_init_two_view is held to), then pushCurrPointsToMap_ + addKeyFrame_ or
                                "skip this frame" with the first keyframe's pose
    vo_addFrame.cpp:70-140      DOING_TRACKING: tests/vo_chain.py unchanged

Like tests/vo_chain.py it takes nothing from the run but the iteration order of the host's map container (`map_order`).
"""
import numpy as np

import finish_restate
import vo_chain

MATCH_KEYS = dict(feature_match_method_index_initialization=1, max_matching_pixel_dist_in_initialization=100.0)


class OracleChainFromImages(vo_chain.OracleChain):
    def __init__(self, *args, init_params=None, **kwargs):
        super().__init__(*args, **kwargs)
        prm = dict(init_params or {})
        self.match_method = int(prm.pop("feature_match_method_index_initialization",
                                        MATCH_KEYS["feature_match_method_index_initialization"]))
        self.match_dist = float(prm.pop("max_matching_pixel_dist_in_initialization",
                                        MATCH_KEYS["max_matching_pixel_dist_in_initialization"]))
        self.init_params = prm                       # the keys of finish_restate.DEFAULTS
        self.restatement = finish_restate.Restatement()
        self.K3 = np.array([[self.K["fx"], 0, self.K["cx"]], [0, self.K["fy"], self.K["cy"]], [0, 0, 1.0]])
        self.state = "BLANK"
        self.init_frame = None

    def first_keyframe(self, fr):                    # vo_addFrame.cpp:30-35
        self.push_to_buff(fr)
        fr.T = np.eye(4)
        self.ref = fr
        self.state = "DOING_INITIALIZATION"

    def initialize(self, fr):                        # vo_addFrame.cpp:36-69
        O, ref = self.O, self.ref
        self.push_to_buff(fr)
        m = O.match_features(ref.desc, fr.desc, self.match_method, 2.0, 1.0, ref.xy, fr.xy, self.match_dist)
        a, b = ref.xy[m["queryIdx"]], fr.xy[m["trainIdx"]]
        res = self.restatement.init_two_view(O, a, b, self.K3, ref.T, **self.init_params)
        slot = res["slot"]
        if slot >= 0:
            inl = np.asarray(res["poses"]["solutions"][slot]["inliers"], np.int64)
        else:                                        # DESIGN.md section 2, deviation 12: a rejected frame like any other
            inl = np.zeros(0, np.int64)
        mi, m3 = m[inl].copy(), m[np.asarray(res["matches_for_3d"], np.int64)].copy()
        mi["imgIdx"] = -1                            # cv::DMatch(queryIdx, trainIdx, distance), motion_estimation.cpp:174-179
        m3["imgIdx"] = -1
        fr.T = np.array(res["T_w_c"], np.float64)
        fr.rec.update(matches_with_ref=m, inliers_matches_with_ref=mi, inliers_matches_for_3d=m3,
                      inliers_pts3d=np.asarray(res["pts3d_in_curr"], np.float32).reshape(-1, 3), init=res, T_init=fr.T.copy())
        good = bool(res["good"])
        if good:
            self.push_points_to_map(fr)
            self.ref = fr
            self.state = "DOING_TRACKING"
            self.init_frame = fr.idx
        else:
            fr.T = ref.T.copy()                      # skip this frame
        return good

    def add_frame(self, fr):
        """VisualOdometry::addFrame; fr.rec["state"] is the state the frame met."""
        fr.rec["state"] = self.state
        if self.state == "BLANK":
            self.first_keyframe(fr)
        elif self.state == "DOING_INITIALIZATION":
            if self.initialize(fr):
                fr.rec["map_after"] = {m: self.map[m].pos.copy() for m in self.map}
        else:
            _, is_key = self.track(fr)
            if is_key:
                fr.rec["map_after"] = {m: self.map[m].pos.copy() for m in self.map}
        self.prev = fr                               # vo_addFrame.cpp:140


def run_oracle_chain_from_images(O, images, K, orb_params, init_params=None, fix_map_points=True, map_order=None):
    """The loop of host/driver/run_vo.cpp under `init_from_images: 1`.  init_params: the keys of finish_restate.DEFAULTS
    plus, optionally, the two matching keys of MATCH_KEYS.  Returns (chain, poses [n, 4, 4] as they stood when each frame
    was done); chain.init_frame is the frame that initialised, None when none did."""
    rows, cols = images[0].shape[:2]
    ch = OracleChainFromImages(O, K, cols, rows, orb_params, fix_map_points, map_order=map_order, init_params=init_params)
    history = []
    for i, img in enumerate(images):
        fr = ch.create_frame(i, img)
        ch.add_frame(fr)
        history.append(fr.T.copy())
    return ch, np.stack(history)
