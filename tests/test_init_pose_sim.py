"""The homography decomposition, the visibility filter, the solution table and the E / H choice of the monocular
initialisation (k_h_decompose and k_init_triangulate in track_kernels.hip, csrc/hd_wave.h) with their host side,
compiled for x86 against tests/sim/hip_emu (libmvo_sim.so) and run thread for thread on the CPU: the MI355X
comparisons of tests/test_gpu_init_pose.py with the restatement, bit for bit, without a GPU."""
import pytest

import test_gpu_init_pose as T
from test_kernels_sim import simctx, simlib, simmvo  # noqa: F401  (fixtures)


@pytest.fixture(scope="module")
def P():
    return T.PR.Restatement()


@pytest.mark.parametrize("kind,n,seed,frac", [T.POSE_CASES[i] for i in (0, 1, 3, 4, 5, 11, 12, 13, 14)])
def test_relative_poses_on_the_emulated_build(simctx, P, O, kind, n, seed, frac):
    pr = T.scene(kind, n, seed, frac)
    T.check_poses(simctx, P, O, pr["src"], pr["dst"], pr["K"])
    T.check_homography(simctx, P, pr["src"], pr["dst"], pr["K"])


def test_relative_poses_cam1_to_cam2_on_the_emulated_build(simctx, P, O):
    pr = T.scene("planar", 300, 41, 0.2)
    T.check_poses(simctx, P, O, pr["src"], pr["dst"], pr["K"], motion_cam2_to_cam1=False)


def test_deviation_cases_on_the_emulated_build(simctx, P, O):
    T.deviation_cases(simctx, P, O)
