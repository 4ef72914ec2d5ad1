"""host/tests/test_orb_distribute (its own makefile, host/tests/orb_distribute.mk): Frame::calcKeyPoints / calcDescriptors of
the mirror (my_slam/vo/frame.h, my_slam/geometry/orb_distribute.h) on one small image, on the MI355X and, with the emulated
build in front of the library search path, on the CPU.
  - with `orb_distribute_keypoints: 1` the frame holds what mvo_calc_keypoints_distributed gives, which is what the numpy
    transcription gives, with the per-level counts; the descriptors are cv::ORB::compute's for those key points;
  - with the key absent or 0 it holds what mvo_calc_keypoints gives, as before, and records no counts;
  - the optional parameter keys reach the library."""
import os
import struct
import subprocess

import numpy as np
import pytest

import orb_distribute_numpy as D
import orb_numpy as N
import test_orb_distribute_sim as S
from conftest import ROOT

HOST_TESTS = os.path.join(ROOT, "monocular-visual-odometry_amd", "host", "tests")
BIN = os.path.join(HOST_TESTS, "test_orb_distribute")
# config/config.yaml's extraction keys, a smaller number of key points
CONFIG = dict(number_of_keypoints_to_extract=300, scale_factor=1.2, level_pyramid=4, score_threshold=20, max_number_of_keypoints=250,
              kpts_uniform_selection_grid_size=16, kpts_uniform_selection_max_pts_per_grid=8)
ORB = dict(nfeatures=300, scale_factor=1.2, nlevels=4, fast_threshold=20, max_keypoints=250, grid_size=16, grid_max_per_cell=8)


def read_dump(path):
    raw = open(path, "rb").read()
    out, pos = [], 0
    for dt in (N.KEYPOINT_DTYPE, np.int32, np.int32, N.KEYPOINT_DTYPE, np.uint8, N.KEYPOINT_DTYPE, N.KEYPOINT_DTYPE):
        n = struct.unpack_from("<Q", raw, pos)[0]
        out.append(np.frombuffer(raw, dt, n, pos + 8))
        pos += 8 + n * np.dtype(dt).itemsize
    assert pos == len(raw)
    return out


def run(tmp_path, name, image, extra, env):
    out = tmp_path / (name + ".bin")
    args = ["%s=%r" % kv for kv in list(CONFIG.items()) + extra]
    r = subprocess.run([BIN, str(image), str(out)] + args, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr
    return read_dump(out)


def host_program(mvo, tmp_path, env):
    subprocess.check_call(["make", "-C", HOST_TESTS, "-f", "orb_distribute.mk", "-s"])
    img = mvo.synth.small_test_image(3, 160, 120)
    image = tmp_path / "image.bin"
    with open(image, "wb") as f:
        f.write(struct.pack("<iii", 160, 120, 3) + img.tobytes())
    ref = D.OrbDistribute(**ORB)
    pyr = ref.pyramid(img)
    cand = ref.candidates(img, pyr)
    want = ref.detect(img, pyr, cand)
    want_all = ref.detect(img, pyr, cand, grid=False)
    want_k, want_d = N.Orb(**ORB).compute(img, want)
    assert 0 < len(want_k) < len(want) < len(want_all)       # the grid cap and the 31-px filter both bite

    kp, ncand, nkp, kp2, desc, direct, plain = run(tmp_path, "on", image, [("orb_distribute_keypoints", 1)], env)
    assert kp.tobytes() == want.tobytes() == direct.tobytes()
    assert ncand.tolist() == np.bincount(cand[:, 2], minlength=4).tolist()
    assert nkp.tolist() == np.bincount(want["octave"], minlength=4).tolist()
    assert kp2.tobytes() == want_k.tobytes() and np.array_equal(desc.reshape(-1, 32), want_d)

    for name, extra in (("off", []), ("zero", [("orb_distribute_keypoints", 0)])):
        kp0, ncand0, nkp0, kp20, desc0, direct0, plain0 = run(tmp_path, name, image, extra, env)
        assert kp0.tobytes() == plain0.tobytes() == plain.tobytes() and len(kp0) > 0
        assert kp0.tobytes() != kp.tobytes() and len(ncand0) == 0 and len(nkp0) == 0
        k0, d0 = N.Orb(**ORB).compute(img, kp0)
        assert kp20.tobytes() == k0.tobytes() and np.array_equal(desc0.reshape(-1, 32), d0)

    # the optional parameter keys
    par = dict(ini_threshold=30, min_threshold=5, cell_size=24, edge_threshold=25)
    kp, _, _, _, _, direct, _ = run(tmp_path, "params", image,
                                    [("orb_distribute_keypoints", 1)] + [("orb_distribute_" + k, v) for k, v in par.items()], env)
    want_p = D.OrbDistribute(**ORB, **par).detect(img, pyr)
    assert kp.tobytes() == want_p.tobytes() == direct.tobytes() and want_p.tobytes() != want.tobytes()


@pytest.mark.gpu
def test_host_program_on_the_gpu(mvo, tmp_path):
    host_program(mvo, tmp_path, dict(os.environ))


def test_host_program_on_the_emulated_build(mvo, tmp_path):
    """The C++ program links libmvo_hip.so by name: a directory in front of the search path that holds the emulated build under
    that name makes the same binary run on the CPU."""
    S.build_simlib()
    (tmp_path / "simlib").mkdir()
    os.symlink(S.SIM_LIB, tmp_path / "simlib" / "libmvo_hip.so")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = str(tmp_path / "simlib") + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    host_program(mvo, tmp_path, env)
