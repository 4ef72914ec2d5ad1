"""The homography kernels of the monocular initialisation (csrc/h_wave.h in track_kernels.hip) and their host side
(track_host.cpp), compiled for x86 against tests/sim/hip_emu (libmvo_sim.so) and run thread for thread on the CPU:
the MI355X comparisons of tests/test_gpu_init.py with the restatement, bit for bit, without a GPU."""
import pytest

import h_restate as HR
import test_gpu_init as T_init
import test_gpu_regrow as T_regrow
from test_kernels_sim import simctx, simlib, simmvo  # noqa: F401  (fixtures)


@pytest.fixture(scope="module")
def R():
    return HR.Restatement()


@pytest.mark.parametrize("n,seed,kw", [T_init.CASES[i] for i in (0, 1, 2, 3, 4)])
def test_find_homography_on_the_emulated_build(simctx, R, n, seed, kw):
    T_init.test_find_homography_matches_the_restatement(simctx, R, n, seed, kw)


def test_degenerate_inputs_on_the_emulated_build(simctx, R):
    T_init.degenerate_cases(simctx, R)


def test_homography_buffers_regrow_on_the_emulated_build(simmvo, R):
    T_regrow.homography_steps(simmvo, R)


def test_outlier_heavy_input_on_the_emulated_build(simctx, R):
    pr = HR.two_view(200, 13, planar=True, noise=0.5, outlier_frac=0.6)
    got, dbg, ref = T_init.check_find_homography(simctx, R, pr["src"], pr["dst"])
    assert got["H"] is not None and ref["iters_run"] > 10
