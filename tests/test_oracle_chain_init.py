"""The oracle chain from images alone (tests/vo_chain_init.py): the reference's state machine (vo_addFrame.cpp:10-142) composed
from the CPU oracle and the restatements, on the 24 PNG-sized frames of synth.Scene3D that tests/test_gpu_run_vo.py uses.  No
product code runs here.  It establishes, before anything goes to a GPU, that this sequence with these thresholds is a fair test
of a run from images: frames are rejected first, the run initialises early enough through the E slot, everything after is
tracked and keyframes are inserted -- and that the chain's own trajectory follows the ground truth.

Thresholds: the reference's values (config/config.yaml:105-113: 1.0 / 20 / 15 / 50 / 2.0 / 0.8), none changed.  50 px of mean
displacement looked out of reach at 2 cm per frame, but at 517 px focal length and ~2 m depth a frame moves the image by about
5.5 px, so frame 9 passes (50.7 px; frame 8: 45.8 px).

Measured on the chain (ascending ids as the map's order): initialises at frame 9 through slot 0 with 703 points kept after 8
rejected frames, 14 frames tracked, keyframes at 14 and 20; against the ground truth after the scale alignment 0.024 m = 8.6 % of
the 0.283 m travelled since frame 9, 1.26 degrees."""
import numpy as np

import run_vo_init_body as B


def test_chain_rejects_initialises_through_e_and_tracks(O):
    ch, hist = B.chain_alone(O)
    n, f = B.N_FRAMES, ch.init_frame
    assert len(ch.frames) == n and f is not None
    states = [fr.rec["state"] for fr in ch.frames]
    assert states == ["BLANK"] + ["DOING_INITIALIZATION"] * f + ["DOING_TRACKING"] * (n - f - 1)
    rejected = ch.frames[1:f]
    assert len(rejected) >= 2                                             # at least two frames are rejected first
    assert f <= n - 12
    for fr in ch.frames[:f]:                                              # the first keyframe and every rejected frame: the identity
        assert np.array_equal(hist[fr.idx], np.eye(4))
    for fr in rejected:
        assert not fr.rec["init"]["good"] and "map_after" not in fr.rec and not fr.conn
    init = ch.frames[f].rec["init"]
    assert init["good"] and init["slot"] == 0 and init["scaled"]         # the chosen slot is 0 (E)
    assert len(ch.frames[f].rec["map_after"]) == init["n_kept"] >= 100
    later = ch.frames[f + 1:]
    assert all(fr.rec["good"] for fr in later)                            # every later frame tracks
    assert sum(fr.rec["is_keyframe"] for fr in later) >= 2                # at least two keyframes after f
    # reasons of the rejections: the small displacement (criteria_1) rejects every one of them
    assert all(not fr.rec["init"]["criteria"][1] for fr in rejected)
    print("oracle chain from images: initialised at frame %d, slot %d, n_kept %d, %d rejected, keyframes at %s"
          % (f, init["slot"], init["n_kept"], len(rejected), [fr.idx for fr in later if fr.rec["is_keyframe"]]))


def test_chain_trajectory_follows_the_ground_truth_up_to_scale(O):
    """The bound of test_run_vo_end_to_end_on_png_frames: 30 % of the distance travelled and 3 degrees, after the alignment
    initialisation leaves free (run_vo_init_body.aligned_errors: the scale only)."""
    ch, hist = B.chain_alone(O)
    gt, f = B.sequence()[2], ch.init_frame
    scale, err_t, err_r = B.aligned_errors(hist, gt, f)
    travelled = float(np.linalg.norm(gt[-1, :3, 3] - gt[f, :3, 3]))
    print("oracle chain from images: scale %.4f, %.4f m = %.1f %% of %.3f m travelled, %.2f deg" % (scale, err_t, 100 * err_t / travelled, travelled, err_r))
    # mean depth was set to 0.8 in front of a ~2 m deep scene: the scale is 2 to 4
    assert 2.0 < scale < 4.0
    assert err_t < 0.3 * travelled and err_r < 3.0
    assert np.linalg.norm(hist[-1, :3, 3] - hist[f, :3, 3]) * scale > 0.2   # it really moved


def test_chain_without_reachable_thresholds_never_initialises(O):
    """min_pixel_dist out of reach: every frame is rejected and keeps the identity (three frames suffice for the rule)."""
    import vo_chain_init
    scene, frames, _ = B.sequence()
    ch, hist = vo_chain_init.run_oracle_chain_from_images(O, frames[:1] + frames[9:11], scene.K, O.default_params(max_keypoints=B.MAX_KEYPOINTS),
                                                          dict(B.INIT_PARAMS, min_pixel_dist=1e6))
    assert ch.init_frame is None and not ch.map and np.array_equal(hist, np.tile(np.eye(4), (3, 1, 1)))
    assert [fr.rec["init"]["criteria"] for fr in ch.frames[1:]] == [[True, False, True]] * 2
