"""my_slam::vo::VisualOdometry (host/include/my_slam/vo/vo.h = the reference's class, vo.h:36-54 / vo_addFrame.cpp:10-142) driven
by host/tests/test_vo_state_machine.cpp over feature-level frames, on the emulated build of the kernels (CPU) and on the MI355X:
BLANK -> DOING_INITIALIZATION with the identity and one keyframe; a tiny baseline is rejected (the first keyframe's pose bit for
bit, one keyframe, an empty map); a wide baseline initialises (two keyframes, map size = n_kept, pose and points exactly
mvo_init_two_view's on the same matches); two further views are tracked; points on a plane initialise through a homography
slot; 30 rejected frames leave 20 in the frame buffer, and every frame enters the buffer exactly once."""
import os
import re
import subprocess

import numpy as np
import pytest

import h_restate as HR
from conftest import ROOT
from test_host_initialization import seen_by, view
from test_init_finish_sim import sim_init_as_the_library, simlib_init  # noqa: F401  (fixtures)

VO_BIN = os.path.join(ROOT, "monocular-visual-odometry_amd", "host", "tests", "test_vo_state_machine")


def test_state_machine_binary_is_built_and_links_only_the_hip_library():
    assert os.path.exists(VO_BIN), "run __graft_entry__.build()"
    ldd = subprocess.run(["ldd", VO_BIN], capture_output=True, text=True).stdout
    assert "libmvo_hip.so" in ldd and "liboracle" not in ldd and "opencv" not in ldd.lower()


def write_scene(path):
    rng = np.random.RandomState(7)
    K, n = HR.K_DEFAULT, 400
    uv = rng.uniform([40, 40], [600, 440], (n, 2))
    rays = np.linalg.solve(K, np.c_[uv, np.ones(n)].T).T
    X1 = rays * rng.uniform(2.5, 8.0, n)[:, None]
    d_ref = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    frames = [(uv.astype(np.float32), d_ref),
              seen_by(view(X1, K, 0.1, [0.005, 0.001, 0.0], rng), d_ref, rng),          # tiny
              seen_by(view(X1, K, 6.0, [0.3, 0.05, 0.02], rng), d_ref, rng),            # wide
              seen_by(view(X1, K, 6.3, [0.33, 0.05, 0.03], rng), d_ref, rng),           # two further views, close to the wide one
              seen_by(view(X1, K, 6.6, [0.36, 0.06, 0.04], rng), d_ref, rng)]
    # points on a tilted plane, z = 4 + 0.3 x - 0.2 y
    uvp = rng.uniform([40, 40], [600, 440], (n, 2))
    r = np.linalg.solve(K, np.c_[uvp, np.ones(n)].T).T
    Xp = r * (4.0 / (1.0 - 0.3 * r[:, 0] + 0.2 * r[:, 1]))[:, None]
    d_p = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    frames += [(uvp.astype(np.float32), d_p), seen_by(view(Xp, K, 6.0, [0.3, 0.05, 0.02], rng), d_p, rng)]
    with open(path, "wb") as f:
        f.write(np.array([640, 480], "<i4").tobytes())
        f.write(np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], "<f8").tobytes())
        f.write(np.array([len(xy) for xy, _ in frames], "<i4").tobytes())
        for xy, desc in frames:
            f.write(np.ascontiguousarray(xy, "<f4").tobytes())
            f.write(np.ascontiguousarray(desc).tobytes())


def run_program(tmp_path):
    scene = tmp_path / "vo_scene.bin"
    write_scene(scene)
    r = subprocess.run([VO_BIN, str(scene)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "VO-OK" in r.stdout, r.stdout + r.stderr
    c = {k: int(v) for k, v in re.findall(r"(\w+) (-?\d+)", r.stdout)}
    assert c["tiny_matches"] > 300 and c["matches"] > 300 and c["slot"] == 0 and c["kept"] > 200 and c["map"] == c["kept"], c
    assert c["tracked0"] > 150 and c["tracked1"] > 150 and c["plane_slot"] >= 1 and c["plane_kept"] > 200 and c["buffer"] == 20, c


def test_cpp_state_machine_on_the_emulated_build(tmp_path, sim_init_as_the_library):
    run_program(tmp_path)


@pytest.mark.gpu
def test_cpp_state_machine(tmp_path):
    run_program(tmp_path)
