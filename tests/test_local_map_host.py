"""host/tests/test_local_map (its own makefile, host/tests/local_map.mk): the mirror function of my_slam/vo/local_map.h on a
hand-built frame, on the MI355X and, with the emulated build in front of the library search path, on the CPU.
  - the masks: skip marks the map points connected in the frame, the level of a connected keypoint is -2 (also of one whose
    point has left the map), every other keypoint keeps its octave;
  - the search is the transcription's (tests/local_map_numpy.py) from the frame's pose with level_scale[l] = scale_factor
    multiplied l times;
  - the second optimisation (tests/pose_optimize_numpy.py) runs over the first pass's inlier matches in their order followed by
    the new matches in trainIdx order, weighted (float)(1 / (scale scale));
  - applied: the pose is replaced, the unflagged new matches are connected and counted in matched_times_, the flagged first-pass
    connections are erased, visible_times_ stays;
  - any other outcome (no new matches, not optimised, moved too far) leaves pose, connections and counters as they were;
  - the keys: `tracking_local_map` is off when absent or 0, the `local_map_*` keys reach the call."""
import os
import struct
import subprocess

import numpy as np
import pytest

import local_map_numpy as LM
import pose_optimize_numpy as R
from conftest import ROOT

HOST_TESTS = os.path.join(ROOT, "monocular-visual-odometry_amd", "host", "tests")
BIN = os.path.join(HOST_TESTS, "test_local_map")
SIM_DIR = os.path.join(ROOT, "tests", "sim")
SIM_LOCAL_MAP_VO_LIB = os.path.join(SIM_DIR, "_build", "libmvo_sim_local_map_vo.so")
N_MAP, NT, L = 257, 700, 8
GONE = 100000          # ids of map points that have left the map


def build_simlib_vo():
    subprocess.check_call(["make", "-C", SIM_DIR, "-f", "local_map_vo.mk", "-s", "-j8", "_build/libmvo_sim_local_map_vo.so"])
    return SIM_LOCAL_MAP_VO_LIB


def frame():
    """The shared scene as a frame after its first pass: the scene's skipped points that are in view are the first pass's inlier
    matches, each with a keypoint of its own near its projection (every fifth 3 px off: the second optimisation flags those); the
    scene's taken keypoints are connected to points that have left the map."""
    s = LM.scene(N_MAP, L)
    rng = np.random.RandomState(5)
    w = LM.view(s["pos"], s["normal"], s["max_dist"], s["T"], s["K"], s["cols"], s["rows"], s["level_scale"])
    first = np.nonzero((s["skip"] != 0) & w["in_view"])[0]
    first = first[rng.permutation(len(first))]                       # the matches' own order, not the map's
    noise = rng.normal(0, 0.3, (len(first), 2))
    noise[::5] += 3.0
    kp_first = (np.stack([w["u"], w["v"]], 1)[first].astype(np.float64) + noise).astype(np.float32)
    txy = np.concatenate([s["txy"][:NT], kp_first])
    octave = np.concatenate([s["octave"][:NT], rng.randint(0, L, len(first)).astype(np.int32)])
    kdesc = np.concatenate([s["t"][:NT], s["desc"][first]])
    taken = np.nonzero(s["taken"][:NT])[0]
    conn = [(int(j), GONE + int(j)) for j in taken] + [(NT + k, int(i)) for k, i in enumerate(first)]
    match = NT + np.arange(len(first), dtype=np.int32)
    return s, first, txy, octave, kdesc, np.array(conn, np.int32), match


def weights(octave):
    out = []
    for o in octave:
        sc = float(np.float32(LM.level_scales(LM.SCALE_FACTOR, int(o) + 1)[-1]))
        out.append(np.float32(1.0 / (sc * sc)))
    return np.array(out, np.float32)


def read_dump(path):
    raw = open(path, "rb").read()
    out, p = [], 0
    for dt in (np.int32, np.int32, np.float64, np.float64, np.uint8, np.int32, LM.DMATCH, np.float32, np.float32, np.float32, np.float64,
               np.int32, np.float64, np.uint8, np.float64, np.int32, np.int32, np.int32):
        n = struct.unpack_from("<Q", raw, p)[0]
        out.append(np.frombuffer(raw, dt, n, p + 8))
        p += 8 + n * np.dtype(dt).itemsize
    assert p == len(raw)
    return out


APPLIED, NO_NEW, NOT_OPTIMISED, TOO_FAR = 4, 0, 2, 3


def host_program(tmp_path, env):
    subprocess.check_call(["make", "-C", HOST_TESTS, "-f", "local_map.mk", "-s"])
    s, first, txy, octave, kdesc, conn, match = frame()
    K = s["K"]
    T_prev = np.array(s["T"])
    T_prev[:3, 3] += 0.01
    scene_path = tmp_path / "scene.bin"
    with open(scene_path, "wb") as f:
        f.write(struct.pack("<6i", N_MAP, len(txy), len(conn), len(match), s["cols"], s["rows"]))
        f.write(struct.pack("<4d", K["fx"], K["fy"], K["cx"], K["cy"]))
        f.write(np.ascontiguousarray(s["T"], np.float64).tobytes() + np.ascontiguousarray(T_prev, np.float64).tobytes())
        for i in range(N_MAP):
            f.write(s["pos"][i].tobytes() + s["normal"][i].tobytes() + s["max_dist"][i:i + 1].tobytes() + s["desc"][i].tobytes())
        f.write(txy.tobytes() + octave.tobytes() + kdesc.tobytes() + conn.tobytes() + match.tobytes())
    connected = dict(conn.tolist())
    n_outcomes = set()
    for name, extra, flag_want, params, opt, outcome_want in (
            ("on", [("tracking_local_map", 1)], 1, {}, {}, APPLIED), ("absent", [], 0, {}, {}, APPLIED),
            ("zero", [("tracking_local_map", 0)], 0, {}, {}, APPLIED),
            ("keys", [("local_map_min_view_cos", 0.3), ("local_map_radius_near", 3.0), ("local_map_radius_far", 6.0),
                      ("local_map_radius_scale", 1.5), ("local_map_lowe_ratio", 0.9), ("local_map_max_hamming", 64)], 0,
             dict(min_view_cos=0.3, radius_near=3.0, radius_far=6.0, radius_scale=1.5, lowe_ratio=0.9, max_hamming=64), {}, APPLIED),
            ("none", [("local_map_max_hamming", -1)], 0, dict(max_hamming=-1), {}, NO_NEW),
            ("few", [("pose_optimization_min_inliers", 4000)], 0, {}, dict(min_inliers=4000), NOT_OPTIMISED),
            ("far", [("max_possible_dist_to_prev_keyframe", 0.001)], 0, {}, {}, TOO_FAR)):
        out = tmp_path / (name + ".bin")
        r = subprocess.run([BIN, str(scene_path), str(out), "scale_factor=%r" % LM.SCALE_FACTOR, "level_pyramid=%d" % L]
                           + ["%s=%r" % kv for kv in extra], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr
        (head, order, setup, init, skip, t_level, found, p3, p2, sig, Twc, info, chi2, outlier, T_after, conn_after, kept,
         times) = read_dump(out)
        P = dict(LM.DEFAULTS, **params)
        # the map in the order of the resident copy
        assert sorted(order.tolist()) == list(range(N_MAP))
        pos, desc, normal, max_dist = (s[k][order] for k in ("pos", "desc", "normal", "max_dist"))
        row_of_id = {int(i): r_ for r_, i in enumerate(order)}
        # the masks
        skip_want = np.zeros(N_MAP, np.uint8)
        skip_want[[row_of_id[int(i)] for i in first]] = 1
        level_want = np.array(octave)
        level_want[conn[:, 0]] = -2
        assert skip.tobytes() == skip_want.tobytes() and t_level.tobytes() == level_want.tobytes(), name
        assert (level_want[:NT] == -2).sum() == s["taken"][:NT].sum() > 0
        ls = LM.level_scales(LM.SCALE_FACTOR, L)
        assert setup.tolist() == [K["fx"], K["fy"], K["cx"], K["cy"], s["cols"], s["rows"], L] + [
            P[k] for k in ("min_view_cos", "radius_near", "radius_far", "near_cos", "radius_scale", "lowe_ratio", "max_hamming")] + ls.tolist()
        assert init.tobytes() == np.ascontiguousarray(s["T"], np.float64).tobytes()
        # the search
        want = LM.match_features(pos, desc, normal, max_dist, s["T"], K, s["cols"], s["rows"], kdesc, txy, level_want, ls, skip_want, params)
        assert found.tobytes() == want.tobytes(), name + ": the new matches against the transcription"
        assert head[0] == flag_want and head[2] == outcome_want and head[1] == (outcome_want == APPLIED), (name, head)
        n_outcomes.add(int(head[2]))
        before = sorted(connected.items())
        times_want = np.ones((N_MAP, 2), np.int32)
        if outcome_want == NO_NEW:
            assert len(want) == 0 and len(info) == 0 and len(p3) == 0
        else:
            # the pairs: the first pass's inlier matches in their order, then the new matches in trainIdx order
            assert len(want) > 20 and (np.diff(want["trainIdx"]) > 0).all()
            rows = np.concatenate([[row_of_id[int(i)] for i in first], want["queryIdx"]])
            kps = np.concatenate([match, want["trainIdx"]])
            assert p3.tobytes() == pos[rows].tobytes() and p2.tobytes() == txy[kps].tobytes(), name + ": the order of the pairs"
            sig_want = weights(octave[kps])
            assert sig.tobytes() == sig_want.tobytes(), name + ": inv_sigma2 is not (float)(1 / (scale scale))"
            res = R.optimize_pose(pos[rows], txy[kps], sig_want, s["T"], K, opt)
            assert Twc.tobytes() == res[0].tobytes() and outlier.tobytes() == res[2].tobytes(), name + ": the second optimisation"
            assert chi2.tobytes() == res[3].tobytes() and info.tobytes() == res[4].tobytes()
            assert (info[0] == R.OPTIMISED) == (outcome_want in (APPLIED, TOO_FAR))
        if outcome_want == APPLIED:
            nf = len(first)
            assert outlier[:nf].any() and not outlier[:nf].all() and outlier[nf:].any() and not outlier[nf:].all()
            assert T_after.tobytes() == Twc.tobytes() and T_after.tobytes() != init.tobytes()
            after = dict(connected)
            for k in range(nf):
                if outlier[k]:
                    del after[int(match[k])]
            for k in range(len(want)):
                if not outlier[nf + k]:
                    after[int(want["trainIdx"][k])] = int(order[want["queryIdx"][k]])
                    times_want[order[want["queryIdx"][k]], 0] += 1
            assert conn_after.reshape(-1, 2).tolist() == [list(c) for c in sorted(after.items())], name + ": the connections"
            assert kept.tolist() == match[outlier[:nf] == 0].tolist()
        else:
            assert T_after.tobytes() == init.tobytes(), name + ": the pose changed"
            assert conn_after.reshape(-1, 2).tolist() == [list(c) for c in before], name + ": the connections changed"
            assert kept.tolist() == match.tolist()
        assert times.reshape(-1, 2).tolist() == times_want.tolist(), name + ": matched_times_ / visible_times_"
    assert n_outcomes == {APPLIED, NO_NEW, NOT_OPTIMISED, TOO_FAR}


@pytest.mark.gpu
def test_host_program_on_the_gpu(tmp_path):
    host_program(tmp_path, dict(os.environ))


def test_host_program_on_the_emulated_build(tmp_path):
    """The C++ program links libmvo_hip.so by name: a directory in front of the search path that holds the emulated build under
    that name makes the same binary run on the CPU."""
    (tmp_path / "simlib").mkdir()
    os.symlink(build_simlib_vo(), tmp_path / "simlib" / "libmvo_hip.so")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = str(tmp_path / "simlib") + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    host_program(tmp_path, env)
