"""host/tests/test_map_refresh (its own makefile, host/tests/map_refresh.mk): the mirror functions of my_slam/vo/map_refresh.h
on a hand-built window of 20 frames, on the MI355X and, with the emulated build in front of the library search path, on the CPU.
  - collectObservations gives the declared order -- frames oldest first, then keypoint index -- although every frame's
    connection map is filled in a scrambled order; a point with 70 observations keeps the newest 64; connections to points
    that left the map are ignored;
  - refreshMapPoints leaves MapPoint::descriptor_, MapPoint::norm_ (kept where the new one is not finite), MapOnDevice's host
    copy and the resident arrays equal to the transcription (tests/map_refresh_numpy.py);
  - the key `map_point_refresh` is off when absent or 0: trackFrame then calls nothing (tests/run_vo_map_refresh_body.py shows
    the same end to end: the log of such a run equals the log of a run without the key, byte for byte)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import map_refresh_numpy as R
import test_map_refresh_sim as S
from conftest import ROOT

HOST_TESTS = os.path.join(ROOT, "monocular-visual-odometry_amd", "host", "tests")
BIN = os.path.join(HOST_TESTS, "test_map_refresh")
N_PTS, N_FRAMES, NK = 9, 20, 40
NAN_POINT, UNSEEN_POINT, CROWDED_POINT = 3, 8, 0


def scene():
    rng = np.random.RandomState(11)
    pos = np.stack([rng.uniform(-1, 1, N_PTS), rng.uniform(-1, 1, N_PTS), rng.uniform(3, 6, N_PTS)], 1).astype(np.float32)
    desc = rng.randint(0, 256, (N_PTS, 32)).astype(np.uint8)
    base = rng.randint(0, 2, (N_PTS, 256)).astype(np.uint8)
    frames = []
    for f in range(N_FRAMES):
        T = np.eye(4)
        T[:3, 3] = rng.uniform(-0.5, 0.5, 3)
        if f == 7:
            T[:3, 3] = pos[NAN_POINT].astype(np.float64)       # this frame looked at NAN_POINT from the point itself
        # keypoints: -1 no connection, -2 a point that left the map, else a point 1 .. 7 (never UNSEEN_POINT)
        conn = rng.choice(np.r_[-1, -1, -2, np.arange(1, 8)], NK).astype(np.int32)
        crowd = 1 + rng.choice(NK - 1, 4 if f < 17 else (2 if f == 17 else 0), replace=False)     # 17 x 4 + 2 = 70 observations
        conn[crowd] = CROWDED_POINT
        if f == 7:
            conn[0] = NAN_POINT
        elif conn[0] == CROWDED_POINT:
            conn[0] = -1
        kdesc = np.zeros((NK, 32), np.uint8)
        for k in range(NK):
            b = base[conn[k]] if conn[k] >= 0 else rng.randint(0, 2, 256).astype(np.uint8)
            kdesc[k] = np.packbits(b ^ (rng.uniform(size=256) < 0.08).astype(np.uint8))
        frames.append((T, kdesc, conn))
    assert sum(int((c == CROWDED_POINT).sum()) for _, _, c in frames) == 70
    return pos, desc, frames


def write_scene(path, pos, desc, frames):
    with open(path, "wb") as f:
        f.write(struct.pack("<iii", N_PTS, N_FRAMES, NK))
        f.write(pos.tobytes() + desc.tobytes())
        for T, kdesc, conn in frames:
            f.write(np.ascontiguousarray(T, np.float64).tobytes() + kdesc.tobytes() + conn.tobytes())


def declared_observations(order, frames):
    """The declared order, written down independently of the header: (frame oldest first, keypoint index), the newest 64."""
    start, obs_desc, obs_cam = [0], [], []
    for i in order:
        rows = [(f, k) for f, (_, _, conn) in enumerate(frames) for k in range(NK) if conn[k] == i][-64:]
        obs_desc += [frames[f][1][k] for f, k in rows]
        obs_cam += [frames[f][0][:3, 3] for f, _ in rows]
        start.append(start[-1] + len(rows))
    return np.array(start, np.int32), np.array(obs_desc, np.uint8).reshape(-1, 32), np.array(obs_cam, np.float64).reshape(-1, 3)


def read_dump(path):
    raw = open(path, "rb").read()
    out, p = [], 0
    for dt in (np.int32, np.int32, np.int32, np.uint8, np.float64, np.int32, np.float64, np.uint8, np.float64, np.uint8, np.float32, np.uint8):
        n = struct.unpack_from("<Q", raw, p)[0]
        out.append(np.frombuffer(raw, dt, n, p + 8))
        p += 8 + n * np.dtype(dt).itemsize
    assert p == len(raw)
    return out


def run(tmp_path, name, scene_path, extra, env):
    out = tmp_path / (name + ".bin")
    r = subprocess.run([BIN, str(scene_path), str(out)] + ["%s=%r" % kv for kv in extra], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr
    return read_dump(out)


def host_program(tmp_path, env):
    subprocess.check_call(["make", "-C", HOST_TESTS, "-f", "map_refresh.mk", "-s"])
    pos, desc, frames = scene()
    scene_path = tmp_path / "scene.bin"
    write_scene(scene_path, pos, desc, frames)
    for name, extra, flag_want in (("on", [("map_point_refresh", 1)], 1), ("absent", [], 0), ("zero", [("map_point_refresh", 0)], 0)):
        flag, order, start, obs_desc, obs_cam, choice, norm, pdesc, pnorm, host_desc, rpos, rdesc = run(tmp_path, name, scene_path, extra, env)
        assert flag.tolist() == [flag_want]                                     # the key: absent or 0 -> trackFrame calls nothing
        assert sorted(order) == list(range(N_PTS))
        w_start, w_desc, w_cam = declared_observations(order, frames)
        m_i = np.diff(w_start)
        assert m_i[list(order).index(CROWDED_POINT)] == 64 and m_i[list(order).index(UNSEEN_POINT)] == 0 and (m_i >= 3).sum() >= 6
        assert np.array_equal(start, w_start), "collectObservations: the starts differ"
        assert obs_desc.tobytes() == w_desc.tobytes(), "collectObservations: not the declared order"
        assert obs_cam.tobytes() == w_cam.tobytes()
        # (the newest 64 of the crowded point: its oldest six observations, all in frames 0 and 1, are gone)
        a = w_start[list(order).index(CROWDED_POINT)]
        crowd_rows = [(f, k) for f, (_, _, conn) in enumerate(frames) for k in range(NK) if conn[k] == CROWDED_POINT]
        assert obs_desc.reshape(-1, 32)[a].tobytes() == frames[crowd_rows[6][0]][1][crowd_rows[6][1]].tobytes()
        want = R.refresh(pos[order], desc[order], w_desc, w_cam, w_start)
        assert np.array_equal(choice, want[0]) and (want[0] > 0).any()
        assert R.same_f64(norm.reshape(-1, 3), want[2])
        assert pdesc.tobytes() == want[1].tobytes(), "MapPoint::descriptor_"
        assert host_desc.tobytes() == want[1].tobytes(), "MapOnDevice's host copy"
        assert rdesc.tobytes() == want[1].tobytes(), "the resident descriptors"
        assert rpos.tobytes() == pos[order].tobytes(), "the resident positions"
        # MapPoint::norm_: the new one where it is finite and the point was observed, else what it held (0, 0, 1)
        i_nan, i_unseen = list(order).index(NAN_POINT), list(order).index(UNSEEN_POINT)
        assert np.isnan(want[2][i_nan]).all() and want[0][i_nan] >= 0 and want[0][i_unseen] == -1
        w_norm = want[2].copy()
        w_norm[[i_nan, i_unseen]] = [0, 0, 1]
        assert pnorm.tobytes() == w_norm.tobytes(), "MapPoint::norm_"


@pytest.mark.gpu
def test_host_program_on_the_gpu(tmp_path):
    host_program(tmp_path, dict(os.environ))


def test_host_program_on_the_emulated_build(tmp_path):
    """The C++ program links libmvo_hip.so by name: a directory in front of the search path that holds the emulated build under
    that name makes the same binary run on the CPU."""
    S.build_simlib()
    (tmp_path / "simlib").mkdir()
    os.symlink(S.SIM_MAP_REFRESH_LIB, tmp_path / "simlib" / "libmvo_hip.so")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = str(tmp_path / "simlib") + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    host_program(tmp_path, env)
