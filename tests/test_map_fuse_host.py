"""host/tests/test_map_fuse (its own makefile, host/tests/map_fuse.mk): the mirror functions of my_slam/vo/map_fuse.h on a
hand-built window of 20 frames, on the MI355X and, with the emulated build in front of the library search path, on the CPU.
  - collectFuseFrames gives every keypoint the row of the map point its connection names, -1 without one, -2 for a point that
    left the map, although every frame's connection map is filled in a scrambled order; the scale is scale_factor^octave;
  - fuseMapPoints reports what the transcription (tests/map_fuse_numpy.py) gives on the same arrays, and leaves the state as
    declared: the connections of a replaced point rewritten in every buffered frame, its counters added to its survivor's, the
    point gone from map_ and from the resident map, the added observations connected, connections to departed points untouched;
  - the key `map_point_fuse` is off when absent or 0: trackFrame then calls nothing; `map_point_fuse_max_px` and
    `map_point_fuse_max_hamming` reach the call."""
import os
import struct
import subprocess

import numpy as np
import pytest

import map_fuse_numpy as M
import test_map_fuse_sim as S
from conftest import ROOT

HOST_TESTS = os.path.join(ROOT, "monocular-visual-odometry_amd", "host", "tests")
BIN = os.path.join(HOST_TESTS, "test_map_fuse")
N_PTS, N_FRAMES, COLS, ROWS = 90, 20, 640, 480
K = M.FR1_K


def scene():
    rng = np.random.RandomState(19)
    s = M.scene(rng, N_PTS, [int(x) for x in rng.randint(30, 121, N_FRAMES)], K=K, cols=COLS, rows=ROWS)
    frames = []
    for fr in s["frames"]:
        octave = rng.randint(0, 4, len(fr["desc"])).astype(np.int32)
        scale = np.ones(len(octave))
        for o in range(1, 4):                                    # the mirror's product: 1.0 * 1.2 * 1.2 ... in double, then float
            scale[octave >= o] = scale[octave >= o] * 1.2
        frames.append(dict(fr, scale=scale.astype(np.float32), octave=octave))
    matched, visible = rng.randint(1, 9, N_PTS).astype(np.int32), rng.randint(9, 30, N_PTS).astype(np.int32)
    return s["pos"], s["desc"], frames, matched, visible


def write_scene(path, pos, desc, frames, matched, visible):
    with open(path, "wb") as f:
        f.write(struct.pack("<iiii", N_PTS, N_FRAMES, COLS, ROWS))
        f.write(struct.pack("<4d", K["fx"], K["fy"], K["cx"], K["cy"]))
        f.write(pos.tobytes() + desc.tobytes() + matched.tobytes() + visible.tobytes())
        for fr in frames:
            f.write(struct.pack("<i", len(fr["desc"])) + np.ascontiguousarray(fr["T"], np.float64).tobytes() + fr["xy"].tobytes()
                    + fr["desc"].tobytes() + fr["octave"].tobytes() + fr["conn"].tobytes())


def read_dump(path):
    raw = open(path, "rb").read()
    out, p = [], 0
    for dt in (np.int32, np.int32, np.int32, np.int32, np.float32, np.float64) + (np.int32,) * 9:
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


def host_program(tmp_path, env):
    subprocess.check_call(["make", "-C", HOST_TESTS, "-f", "map_fuse.mk", "-s"])
    pos, desc, frames, matched, visible = scene()
    scene_path = tmp_path / "scene.bin"
    write_scene(scene_path, pos, desc, frames, matched, visible)
    kp = [len(fr["desc"]) for fr in frames]
    first = np.r_[0, np.cumsum(kp)]
    for name, extra, flag_want, params in (("on", [("map_point_fuse", 1)], 1, {}), ("absent", [], 0, {}), ("zero", [("map_point_fuse", 0)], 0, {}),
                                           ("keys", [("map_point_fuse_max_px", 1.5), ("map_point_fuse_max_hamming", 35)], 0,
                                            dict(max_px=1.5, max_hamming=35))):
        (flag, order, n_kp, conn_rows, scale, setup, replaced_by, added, counts, after, in_map, conn_after, m_after, v_after,
         resident) = run(tmp_path, name, scene_path, extra, env)
        assert flag.tolist() == [flag_want]                                     # the key: absent or 0 -> trackFrame calls nothing
        assert sorted(order) == list(range(N_PTS))
        row_of = np.empty(N_PTS, np.int64)
        row_of[order] = np.arange(N_PTS)
        # collectFuseFrames, written down independently of the header
        assert n_kp.tolist() == kp
        want_conn = np.concatenate([np.where(fr["conn"] >= 0, row_of[np.maximum(fr["conn"], 0)], fr["conn"]) for fr in frames]).astype(np.int32)
        assert (want_conn == -2).any() and (want_conn == -1).any() and (want_conn >= 0).any()
        assert np.array_equal(conn_rows, want_conn), "collectFuseFrames: the connections"
        assert scale.tobytes() == np.concatenate([fr["scale"] for fr in frames]).tobytes(), "collectFuseFrames: the scales"
        P = dict(dict(max_px=M.DEFAULT_MAX_PX, max_hamming=M.DEFAULT_MAX_HAMMING), **params)
        assert setup.tolist() == [K["fx"], K["fy"], K["cx"], K["cy"], COLS, ROWS, P["max_px"], P["max_hamming"]]
        # the transcription on the arrays in map order
        t_frames = [dict(fr, conn=want_conn[first[f]:first[f + 1]]) for f, fr in enumerate(frames)]
        trace = {}
        w_rep, w_added, w_counts = M.fuse(pos[order], desc[order], t_frames, K, COLS, ROWS, P["max_px"], P["max_hamming"], trace=trace)
        assert w_counts[1] >= 5 and w_counts[2] >= 1 and w_counts[3] >= 50 and trace["sizes"][-1] == 3, w_counts
        assert replaced_by.tobytes() == w_rep.tobytes() and added.tobytes() == w_added.tobytes() and counts.tobytes() == w_counts.tobytes()
        # the state after the call
        gone = np.nonzero(w_rep != np.arange(N_PTS))[0]                          # rows
        kept_scene = sorted(int(order[i]) for i in range(N_PTS) if w_rep[i] == i)
        assert in_map.tolist() == kept_scene, "replaced points are gone from map_, and only they"
        assert sorted(after.tolist()) == kept_scene and resident.tolist() == [N_PTS - len(gone)], "the resident map follows"
        want_after = want_conn.copy()
        live = want_after >= 0
        want_after[live] = w_rep[want_after[live]]                               # connections rewritten in every buffered frame
        for f, j, p in w_added.tolist():
            assert want_after[first[f] + j] == -1
            want_after[first[f] + j] = p                                         # added observations connected to the survivor
        want_scene = np.where(want_after >= 0, np.asarray(order)[np.maximum(want_after, 0)], want_after)
        assert np.array_equal(conn_after, want_scene), "the connection maps after the call"
        assert not (conn_after == -3).any() and ((conn_after == -2) == (want_conn == -2)).all()      # departed points untouched
        assert not np.isin(conn_after, np.asarray(order)[gone]).any(), "a connection names a replaced point"
        want_m, want_v = np.full(N_PTS, -1, np.int64), np.full(N_PTS, -1, np.int64)
        for i in range(N_PTS):
            if w_rep[i] == i:
                group = np.asarray(order)[w_rep == i]
                want_m[order[i]], want_v[order[i]] = matched[group].sum(), visible[group].sum()
        assert np.array_equal(m_after, want_m) and np.array_equal(v_after, want_v), "the counters are summed"


@pytest.mark.gpu
def test_host_program_on_the_gpu(tmp_path):
    host_program(tmp_path, dict(os.environ))


def test_host_program_on_the_emulated_build(tmp_path):
    """The C++ program links libmvo_hip.so by name: a directory in front of the search path that holds the emulated build under
    that name makes the same binary run on the CPU."""
    S.build_simlib()
    (tmp_path / "simlib").mkdir()
    os.symlink(S.SIM_MAP_FUSE_LIB, tmp_path / "simlib" / "libmvo_hip.so")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = str(tmp_path / "simlib") + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    host_program(tmp_path, env)
