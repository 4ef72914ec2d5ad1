"""host/tests/test_projection_match (its own makefile, host/tests/projection.mk): the mirror functions of
my_slam/vo/projection_match.h and the poseEstimationPnP of my_slam/vo/pnp_tracking.h on the tracking scene of
tests/projection_numpy.py, on the MI355X and, with the emulated build in front of the library search path, on the CPU.
  - predictPose / matchMapByProjection give what the C-ABI gives (and what the transcription gives);
  - with `tracking_match_by_projection: 1` poseEstimationPnP hands PnP exactly those matches, renumbered to its candidate list,
    and that list equals getMappointsInCurrentView's for the predicted pose;
  - with the key absent or 0 it hands PnP matchFeatures' result, as before."""
import os
import struct
import subprocess

import numpy as np
import pytest

import projection_numpy as P
import test_projection_sim as S
from conftest import ROOT

HOST_TESTS = os.path.join(ROOT, "monocular-visual-odometry_amd", "host", "tests")
BIN = os.path.join(HOST_TESTS, "test_projection_match")
PARAMS = dict(projection_match_max_pixel_dist=6.0, projection_match_lowe_ratio=0.8, projection_match_max_hamming=64)
SCALE_FACTOR = 1.2
PX = np.dtype([("x", "<f4"), ("y", "<f4")])


def scene_with_motion():
    """The tracking scene; the keypoints get octaves 0 .. 3 (seeded); T_prev2 = the keyframe's pose and T_prev half way to
    the scene's predicted pose (R_half^2 = R_pred, (R_half + I) t_half = t_pred), so that predict_pose lands on it up to
    rounding."""
    s = P.tracking_scene()
    octave = np.random.RandomState(5).randint(0, 4, len(s["t"])).astype(np.int32)
    rvec = np.array([0.03, -0.06, 0.02]) + [0.002, -0.0015, 0.001]
    R = P.rodrigues(rvec / 2)
    T_prev = np.eye(4)
    T_prev[:3, :3] = R
    T_prev[:3, 3] = np.linalg.solve(R + np.eye(3), s["T_pred"][:3, 3])
    return s, octave, np.eye(4), T_prev


def write_scene(path, s, octave, T_prev2, T_prev):
    K = s["K"]
    with open(path, "wb") as f:
        f.write(struct.pack("<iiii", len(s["pos"]), len(s["t"]), s["cols"], s["rows"]))
        f.write(np.array([K["fx"], K["fy"], K["cx"], K["cy"]], np.float64).tobytes())
        f.write(np.ascontiguousarray(T_prev2, np.float64).tobytes() + np.ascontiguousarray(T_prev, np.float64).tobytes())
        f.write(np.ascontiguousarray(s["pos"], np.float32).tobytes() + np.ascontiguousarray(s["desc"], np.uint8).tobytes())
        f.write(np.ascontiguousarray(s["txy"], np.float32).tobytes() + octave.tobytes() + np.ascontiguousarray(s["t"], np.uint8).tobytes())


def read_dump(path):
    raw = open(path, "rb").read()
    out, pos = [], 0
    for dt in (np.float64, np.int32, np.int32, PX, P.DMATCH, P.DMATCH, np.int32, PX, P.DMATCH, np.int32, P.DMATCH, P.DMATCH, np.float64):
        n = struct.unpack_from("<Q", raw, pos)[0]
        out.append(np.frombuffer(raw, dt, n, pos + 8))
        pos += 8 + n * np.dtype(dt).itemsize
    assert pos == len(raw)
    return out


def run(tmp_path, name, scene, extra, env):
    out = tmp_path / (name + ".bin")
    args = ["%s=%r" % kv for kv in list(PARAMS.items()) + [("scale_factor", SCALE_FACTOR)] + extra]
    r = subprocess.run([BIN, str(scene), str(out)] + args, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr
    return read_dump(out)


def host_program(mvo, tmp_path, env):
    subprocess.check_call(["make", "-C", HOST_TESTS, "-f", "projection.mk", "-s"])
    s, octave, T_prev2, T_prev = scene_with_motion()
    scene = tmp_path / "scene.bin"
    write_scene(scene, s, octave, T_prev2, T_prev)
    scale = np.array([np.float32(1.0), np.float32(SCALE_FACTOR), np.float32(SCALE_FACTOR * SCALE_FACTOR),
                      np.float32(SCALE_FACTOR * SCALE_FACTOR * SCALE_FACTOR)], np.float32)[octave]
    T_pred = P.predict_pose(T_prev2, T_prev)
    assert np.abs(T_pred - s["T_pred"]).max() < 1e-12
    b = (s["K"], s["cols"], s["rows"])
    want = P.match_features(s["pos"], s["desc"], T_pred, *b, s["t"], s["txy"], 6.0, 0.8, 64, scale)
    u, v, in_view = P.project_map(s["pos"], T_pred, *b)
    assert P.scene_score(s, want)[1:] == (343, 0) and in_view.sum() == 348

    pred, order, cand, cand_px, mirror, direct, cand0, cand0_px, blind, flags, handed, inliers, T_out = run(
        tmp_path, "on", scene, [("tracking_match_by_projection", 1)], env)
    assert pred.tobytes() == T_pred.tobytes() == mvo.predict_pose(T_prev2, T_prev).tobytes()
    assert sorted(order) == list(range(len(s["pos"])))
    # the transcription on the map in the order the program uploaded it
    want_o = P.match_features(s["pos"][order], s["desc"][order], T_pred, *b, s["t"], s["txy"], 6.0, 0.8, 64, scale)
    assert sorted(zip(order[want_o["queryIdx"]], want_o["trainIdx"])) == sorted(zip(want["queryIdx"], want["trainIdx"]))
    assert direct.tobytes() == want_o.tobytes()                           # C-ABI = transcription
    view_o = in_view[order]
    slot_o = np.cumsum(view_o) - 1
    want_r = want_o.copy()
    want_r["queryIdx"] = slot_o[want_o["queryIdx"]]
    assert mirror.tobytes() == want_r.tobytes()                           # mirror = the same, renumbered to the candidate list
    assert np.array_equal(cand, order[view_o])                            # all points in view, in map order
    assert cand_px.tobytes() == np.stack([u, v], 1)[order][view_o].tobytes()
    assert np.array_equal(cand0, cand) and cand0_px.tobytes() == cand_px.tobytes()   # = getMappointsInCurrentView for that pose
    assert flags.tolist() == [1, 1]
    assert handed.tobytes() == mirror.tobytes()                           # poseEstimationPnP handed PnP exactly those
    pairs = set(zip(handed["queryIdx"].tolist(), handed["trainIdx"].tolist()))
    assert len(inliers) > 300 and set(zip(inliers["queryIdx"].tolist(), inliers["trainIdx"].tolist())) <= pairs
    assert np.abs(T_out.reshape(4, 4) - s["T_true"]).max() < 5e-3         # and PnP on them finds the frame
    assert blind.tobytes() != mirror.tobytes()

    for name, extra in (("off", []), ("zero", [("tracking_match_by_projection", 0)])):
        pred0, order0, _, _, mirror0, direct0, cand00, _, blind0, flags0, handed0, inliers0, _ = run(tmp_path, name, scene, extra, env)
        assert pred0.tobytes() == pred.tobytes() and np.array_equal(order0, order)
        assert mirror0.tobytes() == mirror.tobytes() and direct0.tobytes() == direct.tobytes()
        assert len(handed0) == 0                                          # the matcher of the key did not run
        _, _, view_prev = P.project_map(s["pos"], T_prev, *b)
        assert np.array_equal(cand00, order[view_prev[order]])            # candidates under the last keyframe's pose, as before
        pairs0 = set(zip(blind0["queryIdx"].tolist(), blind0["trainIdx"].tolist()))
        if flags0[0]:                                                     # what PnP kept is a subset of matchFeatures' result
            assert set(zip(inliers0["queryIdx"].tolist(), inliers0["trainIdx"].tolist())) <= pairs0
        # (and matchFeatures finds the twins: none of its matches joins a point with its partner)
        found = np.zeros(len(blind0), P.DMATCH)
        found["queryIdx"], found["trainIdx"] = cand00[blind0["queryIdx"]], blind0["trainIdx"]
        assert P.scene_score(s, found)[1] == 0 and len(found) > 300


@pytest.mark.gpu
def test_host_program_on_the_gpu(mvo, tmp_path):
    host_program(mvo, tmp_path, dict(os.environ))


def test_host_program_on_the_emulated_build(mvo, tmp_path):
    """The C++ program links libmvo_hip.so by name: a directory in front of the search path that holds the emulated build under
    that name makes the same binary run on the CPU."""
    S.build_simlib()
    (tmp_path / "simlib").mkdir()
    os.symlink(S.SIM_PROJECTION_LIB, tmp_path / "simlib" / "libmvo_hip.so")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = str(tmp_path / "simlib") + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    host_program(mvo, tmp_path, env)
