"""The C++ mirror of the DOING_INITIALIZATION branch (host/include/my_slam/vo/initialization.h) driven like
vo_addFrame.cpp:36-69 by host/tests/test_initialization.cpp, on the emulated build of the kernels (CPU) and on the
MI355X: a frame with a tiny baseline does not initialise and takes the first keyframe's pose, a frame with a large
baseline does, fills the map, is held as the second keyframe and carries exactly mvo_init_two_view's pose and points."""
import os
import re
import subprocess

import numpy as np
import pytest

import h_restate as HR
from conftest import ROOT
from test_init_finish_sim import sim_init_as_the_library, simlib_init  # noqa: F401  (fixtures)

INIT_BIN = os.path.join(ROOT, "monocular-visual-odometry_amd", "host", "tests", "test_initialization")


def test_initialization_binary_is_built_and_links_only_the_hip_library():
    assert os.path.exists(INIT_BIN), "run __graft_entry__.build()"
    ldd = subprocess.run(["ldd", INIT_BIN], capture_output=True, text=True).stdout
    assert "libmvo_hip.so" in ldd and "liboracle" not in ldd and "opencv" not in ldd.lower()


def view(X1, K, rot_deg, t, rng, noise=0.3):
    X2 = X1 @ HR.rot([0.2, 1.0, 0.1], rot_deg).T + np.asarray(t, float)
    p = X2 @ K.T
    return (p[:, :2] / p[:, 2:] + rng.normal(0, noise, (len(X1), 2))).astype(np.float32)


def seen_by(kp, d_ref, rng, frac=0.85, clutter=60):
    """A later frame: `frac` of the points (descriptors with a few flipped bits, shuffled) plus clutter."""
    n = len(kp)
    seen = rng.permutation(n)[: int(frac * n)]
    bits = np.unpackbits(d_ref[seen], axis=1)
    bits ^= (rng.uniform(size=bits.shape) < 0.03).astype(np.uint8)
    desc = np.concatenate([np.packbits(bits, axis=1), rng.randint(0, 256, (clutter, 32)).astype(np.uint8)])
    xy = np.concatenate([kp[seen], rng.uniform(40, 440, (clutter, 2)).astype(np.float32)]).astype(np.float32)
    return xy, desc


def write_scene(path):
    rng = np.random.RandomState(7)
    K, n = HR.K_DEFAULT, 400
    uv = rng.uniform([40, 40], [600, 440], (n, 2))
    rays = np.linalg.solve(K, np.c_[uv, np.ones(n)].T).T
    X1 = rays * rng.uniform(2.5, 8.0, n)[:, None]
    d_ref = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    T_ref = np.eye(4)
    T_ref[:3, :3] = HR.rot([0.3, -0.5, 1.0], 25.0)
    T_ref[:3, 3] = [0.7, -1.3, 2.1]
    tiny = seen_by(view(X1, K, 0.1, [0.005, 0.001, 0.0], rng), d_ref, rng)
    wide = seen_by(view(X1, K, 6.0, [0.3, 0.05, 0.02], rng), d_ref, rng)
    with open(path, "wb") as f:
        f.write(np.array([n, len(tiny[0]), len(wide[0])], "<i4").tobytes())
        f.write(np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], "<f8").tobytes())
        f.write(np.ascontiguousarray(T_ref, "<f8").tobytes())
        for xy, desc in ((uv.astype(np.float32), d_ref), tiny, wide):
            f.write(xy.tobytes())
            f.write(desc.tobytes())


def run_program(tmp_path):
    scene = tmp_path / "init_scene.bin"
    write_scene(scene)
    r = subprocess.run([INIT_BIN, str(scene)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "INIT-OK" in r.stdout, r.stdout + r.stderr
    c = {k: int(v) for k, v in re.findall(r"(\w+) (-?\d+)", r.stdout)}
    assert c["matches"] > 300 and c["slot"] == 0 and c["kept"] > 200 and c["map"] == c["kept"], c
    assert c["tiny_matches"] > 300, c


def test_cpp_initialization_mirror_on_the_emulated_build(tmp_path, sim_init_as_the_library):
    run_program(tmp_path)


@pytest.mark.gpu
def test_cpp_initialization_mirror(tmp_path):
    run_program(tmp_path)
