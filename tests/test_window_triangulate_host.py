"""host/tests/test_window_triangulate (its own makefile, host/tests/window_triangulate.mk): the mirror function of
my_slam/vo/window_triangulate.h on a hand-built window of 20 frames, on the MI355X and, with the emulated build in front of the
library search path, on the CPU.
  - createMapPointsFromWindow hands the newest frame of the buffer to the library as curr and the others, oldest first, as the
    frames, with the connections and scales collectFuseFrames makes, and reports what the transcription
    (tests/window_triangulate_numpy.py) gives on the same arrays: points, pairs, counts;
  - for every point a MapPoint exists afterwards as pushCurrPointsToMap would have made it (world position, descriptor and colour
    of the keyframe's keypoint, unit normal from the keyframe's centre), with consecutive ids; both keypoints are connected to it
    with PtConn{-1, id}; every other connection, every other map point and the resident map are as they were;
  - the key `map_point_create_from_window` is off when absent or 0: trackFrame then calls nothing; the five parameter keys reach
    the call, and ratio_factor is 1.5 scale_factor."""
import os
import struct
import subprocess

import numpy as np
import pytest

import test_window_triangulate_sim as S
import window_triangulate_numpy as W
from conftest import ROOT

HOST_TESTS = os.path.join(ROOT, "monocular-visual-odometry_amd", "host", "tests")
BIN = os.path.join(HOST_TESTS, "test_window_triangulate")
N_PTS, N_FRAMES, N_CURR, COLS, ROWS = 20, 20, 150, 640, 480
K = W.FR1_K
SETUP = ("max_line_px", "lowe_ratio", "max_hamming", "max_cos_parallax", "max_reproj_chi2", "ratio_factor", "min_baseline")


def scene():
    rng = np.random.RandomState(23)
    s = W.scene(rng, N_CURR, [int(x) for x in rng.randint(30, 201, N_FRAMES - 1)], K=K, cols=COLS, rows=ROWS)
    frames = []
    for fr in s["frames"] + [s["curr"]]:
        octave = rng.randint(0, 4, len(fr["desc"])).astype(np.int32)
        scale = np.ones(len(octave))
        for o in range(1, 4):                                    # the mirror's product: 1.0 * 1.2 * 1.2 ... in double, then float
            scale[octave >= o] = scale[octave >= o] * 1.2
        frames.append(dict(fr, scale=scale.astype(np.float32), octave=octave))
    pos = rng.uniform([-1, -1, 2], [1, 1, 6], (N_PTS, 3)).astype(np.float32)
    desc = rng.randint(0, 256, (N_PTS, 32)).astype(np.uint8)
    return pos, desc, frames


def write_scene(path, pos, desc, frames):
    with open(path, "wb") as f:
        f.write(struct.pack("<iiii", N_PTS, N_FRAMES, COLS, ROWS))
        f.write(struct.pack("<4d", K["fx"], K["fy"], K["cx"], K["cy"]))
        f.write(pos.tobytes() + desc.tobytes())
        for fr in frames:
            f.write(struct.pack("<i", len(fr["desc"])) + np.ascontiguousarray(fr["T"], np.float64).tobytes() + fr["xy"].tobytes()
                    + fr["desc"].tobytes() + fr["octave"].tobytes() + fr["conn"].tobytes())


DUMP = (np.int32, np.float64, np.int32, np.int32, np.float32, np.int32, np.float32, np.float64, np.int32, np.float32, np.float64, np.int32,
        np.int32, np.float32, np.int32, np.float32, np.uint8, np.float64, np.uint8, np.int32, np.int32)


def read_dump(path):
    raw = open(path, "rb").read()
    out, p = [], 0
    for dt in DUMP:
        n = struct.unpack_from("<Q", raw, p)[0]
        out.append(np.frombuffer(raw, dt, n, p + 8))
        p += 8 + n * np.dtype(dt).itemsize
    assert p == len(raw)
    return out


def run(tmp_path, name, scene_path, extra, env):
    out = tmp_path / (name + ".bin")
    r = subprocess.run([BIN, str(scene_path), str(out), "scale_factor=1.2"] + ["%s=%r" % kv for kv in extra], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stderr
    return read_dump(out)


def world_position(p_curr, T):
    """preTranslatePoint3f: (float)(T p) with every row summed j = 0..3 in double from 0."""
    p = p_curr.astype(np.float64)
    out = np.zeros((len(p), 3), np.float32)
    for r in range(3):
        acc = 0.0 + T[r, 0] * p[:, 0]
        acc = acc + T[r, 1] * p[:, 1]
        acc = acc + T[r, 2] * p[:, 2]
        acc = acc + T[r, 3] * 1.0
        out[:, r] = acc.astype(np.float32)
    return out


def host_program(tmp_path, env):
    subprocess.check_call(["make", "-C", HOST_TESTS, "-f", "window_triangulate.mk", "-s"])
    pos, desc, frames = scene()
    scene_path = tmp_path / "scene.bin"
    write_scene(scene_path, pos, desc, frames)
    kp = [len(fr["desc"]) for fr in frames]
    first = np.r_[0, np.cumsum(kp)]
    conn_in = np.concatenate([fr["conn"] for fr in frames])
    keys = dict(max_line_px=3.0, lowe_ratio=0.7, max_hamming=50, max_cos_parallax=0.9995, min_baseline=0.2)
    for name, extra, flag_want, params in (("on", [("map_point_create_from_window", 1)], 1, {}), ("absent", [], 0, {}),
                                           ("zero", [("map_point_create_from_window", 0)], 0, {}),
                                           ("keys", [("map_point_create_" + k, v) for k, v in keys.items()], 0, keys)):
        (flag, setup, n_kp, conn_rows, scale, pts_i, pts_p, pts_c, prs_i, prs_p, prs_c, counts, ids, world, map_size, n_pos, n_desc, n_norm,
         n_rgb, conn_after, tail) = run(tmp_path, name, scene_path, extra, env)
        assert flag.tolist() == [flag_want]                                     # the key: absent or 0 -> trackFrame calls nothing
        P = dict(W.DEFAULTS, ratio_factor=1.5 * 1.2, **params)
        assert setup.tolist() == [K["fx"], K["fy"], K["cx"], K["cy"]] + [float(P[k]) for k in SETUP]
        # what the library was handed: the frames in buffer order, the keyframe last
        assert n_kp.tolist() == kp
        assert np.array_equal(conn_rows == -1, conn_in == -1) and np.array_equal(conn_rows == -2, conn_in == -2)
        assert (conn_rows[conn_in >= 0] >= 0).all() and (conn_in == -2).any() and (conn_in >= 0).any()
        assert scale.tobytes() == np.concatenate([fr["scale"] for fr in frames]).tobytes()
        # the transcription on the same arrays
        t_frames = [dict(fr, conn=conn_rows[first[f]:first[f + 1]]) for f, fr in enumerate(frames)]
        curr, others = t_frames[-1], t_frames[:-1]
        w_points, w_pairs, w_counts, _ = W.window_triangulate(curr, others, K, **P)
        assert len(w_points) >= 20 and w_counts[5] > 0 and (params or w_counts[6] > 0) and len(np.unique(w_points["frame"])) >= 3, w_counts
        assert counts.tobytes() == w_counts.tobytes()
        want_i = np.stack([w_points[k] for k in ("keypoint", "frame", "train", "hamming")], 1).astype(np.int32)
        assert pts_i.tobytes() == want_i.tobytes() and pts_p.tobytes() == w_points["p_curr"].tobytes()
        assert pts_c.tobytes() == w_points["cos2"].tobytes()
        want_i = np.stack([w_pairs[k] for k in ("frame", "keypoint", "train", "hamming", "status")], 1).astype(np.int32)
        assert prs_i.tobytes() == want_i.tobytes() and prs_c.tobytes() == w_pairs["cos2"].tobytes()
        assert prs_p.tobytes() == np.concatenate([w_pairs["p_curr"], w_pairs["p_frame"]], 1).tobytes()
        # the new map points
        n_new = len(w_points)
        assert len(ids) == n_new and (np.diff(ids) == 1).all() and map_size.tolist() == [N_PTS, N_PTS + n_new]
        want_world = world_position(w_points["p_curr"], np.asarray(curr["T"], np.float64))
        assert world.tobytes() == want_world.tobytes() and n_pos.tobytes() == want_world.tobytes()
        assert n_desc.tobytes() == curr["desc"][w_points["keypoint"]].tobytes()
        d = want_world.astype(np.float64) - np.asarray(curr["T"], np.float64)[:3, 3][None, :]
        length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        assert n_norm.tobytes() == (d / length[:, None]).tobytes()
        kpt = w_points["keypoint"].astype(np.int64)
        assert n_rgb.tobytes() == np.stack([kpt % 256, 2 * kpt % 256, 3 * kpt % 256], 1).astype(np.uint8).tobytes()
        # the connections: both keypoints of every point name it, nothing else changed
        want_after = conn_in.copy()
        for k, p in enumerate(w_points):
            for slot in (first[-2] + p["keypoint"], first[p["frame"]] + p["train"]):
                assert want_after[slot] == -1
                want_after[slot] = 1000000 + k
        assert np.array_equal(conn_after, want_after)
        assert tail.tolist() == [N_PTS, N_PTS, N_PTS]                           # the old points, the resident map before and after


@pytest.mark.gpu
def test_host_program_on_the_gpu(tmp_path):
    host_program(tmp_path, dict(os.environ))


def test_host_program_on_the_emulated_build(tmp_path):
    """The C++ program links libmvo_hip.so by name: a directory in front of the search path that holds the emulated build under
    that name makes the same binary run on the CPU."""
    S.build_simlib()
    (tmp_path / "simlib").mkdir()
    os.symlink(S.SIM_WINDOW_LIB, tmp_path / "simlib" / "libmvo_hip.so")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = str(tmp_path / "simlib") + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    host_program(tmp_path, env)
