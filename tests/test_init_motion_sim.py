"""recoverPose and the E / H scores of the monocular initialisation (k_recover_pose and k_init_scores in
track_kernels.hip, csrc/em_wave.h) with their host side, compiled for x86 against tests/sim/hip_emu (libmvo_sim.so) and
run thread for thread on the CPU: the MI355X comparisons of tests/test_gpu_init_motion.py with the restatement, bit for
bit, without a GPU."""
import pytest

import test_gpu_init_motion as T
from test_kernels_sim import simctx, simlib, simmvo  # noqa: F401  (fixtures)


@pytest.fixture(scope="module")
def R():
    return T.IR.Restatement()


@pytest.mark.parametrize("kind,n,seed,frac", [T.CASES[i] for i in (0, 1, 2, 3, 4, 5, 6)])
def test_esti_motion_and_scores_on_the_emulated_build(simctx, R, O, kind, n, seed, frac):
    pr = T.scene(kind, n, seed, frac)
    T.check_pipeline(simctx, R, O, pr["src"], pr["dst"], pr["K"])


def test_degenerate_inputs_on_the_emulated_build(simctx, R, O):
    T.degenerate_cases(simctx, R, O)
