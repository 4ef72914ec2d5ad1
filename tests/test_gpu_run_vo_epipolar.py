"""run_vo with `triangulation_match_by_epipolar_line: 1` on the 24 rendered frames of tests/test_gpu_run_vo.py: every keyframe
inserted while tracking (and the seeding of the map, which goes through the same function) matches its reference keyframe along
the epipolar lines of the two estimated poses.  From the frame log alone the numpy transcription (tests/epipolar_numpy.py)
reproduces each keyframe's matches byte for byte: the logged keypoints and descriptors of the two frames, the logged F (EPIF);
and F is exactly what fundamental_from_poses makes of the two logged poses.

Which two poses: the current frame's POSE record and the reference keyframe's pose AS IT STOOD when the new keyframe was
inserted, which the run logs next to EPIF as EPIR.  The reference keyframe's own POSE record dates from its own frame, and the
sliding-window bundle adjustment of the frames in between rewrites the poses of the window in place (vo.cpp:384-478), the
reference keyframe's among them: on the MI355X, frame 7 of this run against keyframe 5, F of the two POSE records differs from
EPIF by 3.6e-5 in an entry of size 7e-5, while the seed keyframe (frame 5 against frame 0, no BA in between) is exact.  So the
exact comparison is made with EPIR; where nothing has touched the reference keyframe since its own frame, EPIR must equal
its POSE record bit for bit, and that is asserted for the seed."""
import subprocess

import numpy as np
import pytest

import epipolar_numpy as E
import vo_chain
from test_gpu_run_vo import EXE, _read_traj, _write_dataset

pytestmark = pytest.mark.gpu

KEYPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                     ("class_id", "<i4")])
MAX_LINE_DIST, LOWE_RATIO, MAX_HAMMING, SCALE_FACTOR = 2.0, 0.8, 64, 1.2


def octave_scales(octave):
    """(float)(scale_factor multiplied by itself `octave` times, starting from 1.0), as the mirror header computes it"""
    table, s = [], 1.0
    for _ in range(int(octave.max()) + 1 if len(octave) else 1):
        table.append(np.float32(s))
        s = s * SCALE_FACTOR
    return np.array(table, np.float32)[octave]


def test_run_vo_matches_keyframes_along_epipolar_lines(mvo, tmp_path):
    n, k1 = 24, 5
    log_path = tmp_path / "frames.log"
    scene, frames, truth, cfg = _write_dataset(
        mvo, tmp_path, n, k1, "save_frame_log_to: %s\ntriangulation_match_by_epipolar_line: 1\nepipolar_match_max_line_dist: %r\n"
        "epipolar_match_lowe_ratio: %r\nepipolar_match_max_hamming: %d\nscale_factor: %r\n"
        % (log_path, MAX_LINE_DIST, LOWE_RATIO, MAX_HAMMING, SCALE_FACTOR))
    r = subprocess.run([EXE, str(cfg)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "keyframes are matched along the epipolar lines" in r.stdout
    assert len(_read_traj(tmp_path / "cam_traj.txt")) == n                      # the trajectory file is written
    log = vo_chain.read_frame_log(log_path)
    assert len(log) == n
    by_id = {int(np.frombuffer(rec["FRAM"], "<i4")[1]): rec for rec in log}      # Frame::id_ -> its record
    n_tracking_keyframes = 0
    for i, rec in enumerate(log):
        if "MREF" not in rec:
            assert "EPIF" not in rec
            continue
        what = "frame %d: " % i
        assert "EPIF" in rec and len(rec["EPIF"]) == 80, what + "a keyframe without its EPIF record"
        ref_id, pad = np.frombuffer(rec["EPIF"], "<i4", 2)
        F = np.frombuffer(rec["EPIF"], "<f8", 9, 8).reshape(3, 3)
        assert pad == 0 and ref_id in by_id, what + "reference keyframe %d is not in the log" % ref_id
        ref = by_id[int(ref_id)]
        if "FLAG" in rec:
            assert np.frombuffer(rec["FLAG"], "<i4")[1] == 1
            n_tracking_keyframes += 1
        # F is the fundamental matrix of the two logged poses, exactly
        assert "EPIR" in rec and len(rec["EPIR"]) == 128, what + "a keyframe without its EPIR record"
        T_then, T_ref, T_cur = (np.frombuffer(x, "<f8").reshape(4, 4) for x in (ref["POSE"], rec["EPIR"], rec["POSE"]))
        F_poses = mvo.fundamental_from_poses(T_ref, T_cur, scene.K)
        print(what + "reference keyframe id %d, max |EPIF - F(EPIR, POSE)| = %g, the window BA moved the reference pose by %g since "
              "its own frame" % (ref_id, np.abs(F_poses - F).max(), np.abs(T_then - T_ref).max()))
        assert np.array_equal(F_poses, F), what + "EPIF is not fundamental_from_poses of the two logged poses"
        assert np.array_equal(T_ref[3], [0, 0, 0, 1]) and np.abs(T_ref[:3, :3] @ T_ref[:3, :3].T - np.eye(3)).max() < 1e-9
        if "FLAG" not in rec:                                 # the seed: its reference keyframe has not been in a BA window yet
            assert np.array_equal(T_then, T_ref), what + "EPIR differs from the untouched reference keyframe's POSE record"
        # the transcription reproduces the matches from the log alone
        k_ref, k_cur = (np.frombuffer(x["KPTS"], KEYPOINT) for x in (ref, rec))
        d_ref, d_cur = (np.frombuffer(x["DESC"], np.uint8).reshape(-1, 32) for x in (ref, rec))
        want = E.match_features(d_ref, np.stack([k_ref["x"], k_ref["y"]], 1), d_cur, np.stack([k_cur["x"], k_cur["y"]], 1), F,
                                MAX_LINE_DIST, LOWE_RATIO, MAX_HAMMING, octave_scales(k_cur["octave"]))
        n_mref, n_iref, n_i3dm = (len(rec[t]) // 16 for t in ("MREF", "IREF", "I3DM"))
        print(what + "MREF %d, IREF %d, I3DM %d" % (n_mref, n_iref, n_i3dm))
        assert len(want) > 50, what + "too few matches along the lines to mean anything"
        assert rec["MREF"] == want.tobytes(), what + "MREF (%d) differs from the transcription (%d)" % (n_mref, len(want))
    assert n_tracking_keyframes >= 1, "no keyframe was inserted while tracking:\n" + r.stdout
