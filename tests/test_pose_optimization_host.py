"""host/tests/test_pose_optimization (its own makefile, host/tests/pose_optimization.mk): the mirror function of
my_slam/vo/pose_optimization.h on a hand-built frame, on the MI355X and, with the emulated build in front of the library search
path, on the CPU.
  - optimizePoseFromMatches hands the matches' points and pixels and inv_sigma2 = (float)(1 / (scale scale)), scale the f32 of
    scale_factor multiplied octave times, to the library, and what it returns and records equals the transcription
    (tests/pose_optimize_numpy.py) with the weights computed here independently; on status 0 the inliers are the non-flagged
    matches in ascending order;
  - a status other than 0 returns no inliers and no pose (poseEstimationPnP then falls back to solvePnPRansac);
  - the keys: `tracking_pose_by_optimization` is off when absent or 0; `pose_optimization_rounds`, `_iterations`, `_min_inliers`,
    `_chi2_threshold` reach the call."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pose_optimize_numpy as R
import test_pose_optimize_sim as S
from conftest import ROOT

HOST_TESTS = os.path.join(ROOT, "monocular-visual-odometry_amd", "host", "tests")
BIN = os.path.join(HOST_TESTS, "test_pose_optimization")
N, NK, SCALE_FACTOR = 120, 150, 1.2
K = {k: float(np.float32(v)) for k, v in R.FR1_K.items()}


def scene(moved_every):
    rng = np.random.RandomState(31 + moved_every)
    p3, p2, T, moved, behind = R.scene(rng, N, 0.5, moved_every, 2)
    T_init = R.perturbed(T, 2.0, (0.1, -0.1, 0.15))
    train = rng.permutation(NK)[:N].astype(np.int32)          # match i -> keypoint train[i]
    kpt = rng.uniform(0, 480, (NK, 2)).astype(np.float32)
    kpt[train] = p2
    octave = rng.randint(0, 8, NK).astype(np.int32)
    return p3, p2, T_init, train, kpt, octave


def weights(octave):
    """(float)(1.0 / ((double)scale (double)scale)), scale = (float)(1.0 multiplied `octave` times by scale_factor)"""
    out = []
    for o in octave:
        s = 1.0
        for _ in range(int(o)):
            s = s * SCALE_FACTOR
        s = float(np.float32(s))
        out.append(np.float32(1.0 / (s * s)))
    return np.array(out, np.float32)


def read_dump(path):
    raw = open(path, "rb").read()
    out, p = [], 0
    for dt in (np.int32, np.int32, np.float64, np.float64, np.float64, np.float32, np.float32, np.float32, np.float64, np.float64,
               np.int32, np.float64, np.uint8):
        n = struct.unpack_from("<Q", raw, p)[0]
        out.append(np.frombuffer(raw, dt, n, p + 8))
        p += 8 + n * np.dtype(dt).itemsize
    assert p == len(raw)
    return out


def host_program(tmp_path, env):
    subprocess.check_call(["make", "-C", HOST_TESTS, "-f", "pose_optimization.mk", "-s"])
    for name, moved_every, extra, flag_want, params in (
            ("on", 5, [("tracking_pose_by_optimization", 1)], 1, {}), ("absent", 5, [], 0, {}),
            ("zero", 5, [("tracking_pose_by_optimization", 0)], 0, {}),
            ("keys", 5, [("pose_optimization_rounds", 2), ("pose_optimization_iterations", 3), ("pose_optimization_min_inliers", 20),
                         ("pose_optimization_chi2_threshold", 4.5)], 0, dict(rounds=2, iterations=3, min_inliers=20, chi2_threshold=4.5)),
            ("few", 2, [("pose_optimization_min_inliers", 100)], 0, dict(min_inliers=100))):
        p3, p2, T_init, train, kpt, octave = scene(moved_every)
        scene_path = tmp_path / (name + "_scene.bin")
        with open(scene_path, "wb") as f:
            f.write(struct.pack("<ii", N, NK) + struct.pack("<4d", K["fx"], K["fy"], K["cx"], K["cy"]))
            f.write(np.ascontiguousarray(T_init, np.float64).tobytes() + kpt.tobytes() + octave.tobytes() + p3.tobytes() + train.tobytes())
        out = tmp_path / (name + ".bin")
        r = subprocess.run([BIN, str(scene_path), str(out), "scale_factor=%r" % SCALE_FACTOR] + ["%s=%r" % kv for kv in extra],
                           capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr
        head, inliers, T_ret, setup, init, o_p3, o_p2, o_sig, Twc, Tcw, info, chi2, outlier = read_dump(out)
        P = dict(R.DEFAULTS, **params)
        sig = weights(octave[train])
        assert len(np.unique(sig)) == 8
        want = R.optimize_pose(p3, p2, sig, T_init, K, params)
        assert head.tolist() == [flag_want, P["min_inliers"], int(want[4][0])]
        assert setup.tolist() == [K["fx"], K["fy"], K["cx"], K["cy"], P["rounds"], P["iterations"], P["min_inliers"], P["chi2_threshold"],
                                  P["huber_delta"], P["rel_tolerance"]]
        assert init.tobytes() == np.ascontiguousarray(T_init, np.float64).tobytes()
        assert o_p3.tobytes() == p3.tobytes() and o_p2.tobytes() == p2.tobytes(), "the points and pixels of the matches"
        assert o_sig.tobytes() == sig.tobytes(), "inv_sigma2 is not (float)(1 / (scale scale))"
        assert Twc.tobytes() == want[0].tobytes() and Tcw.tobytes() == want[1].tobytes(), "the mirror against the transcription"
        assert outlier.tobytes() == want[2].tobytes() and chi2.tobytes() == want[3].tobytes() and info.tobytes() == want[4].tobytes()
        if name == "few":
            assert want[4][0] == R.FEW_INLIERS and len(inliers) == 0 and len(T_ret) == 0
        else:
            assert want[4][0] == R.OPTIMISED and want[4][1] == P["rounds"]
            assert inliers.tolist() == np.nonzero(want[2] == 0)[0].tolist() and 0 < len(inliers) < N
            assert T_ret.tobytes() == want[0].tobytes()


@pytest.mark.gpu
def test_host_program_on_the_gpu(tmp_path):
    host_program(tmp_path, dict(os.environ))


def test_host_program_on_the_emulated_build(tmp_path):
    """The C++ program links libmvo_hip.so by name: a directory in front of the search path that holds the emulated build under
    that name makes the same binary run on the CPU."""
    S.build_simlib()
    (tmp_path / "simlib").mkdir()
    os.symlink(S.SIM_POSE_OPTIMIZE_LIB, tmp_path / "simlib" / "libmvo_hip.so")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = str(tmp_path / "simlib") + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    host_program(tmp_path, env)
