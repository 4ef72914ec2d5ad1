"""The finish of the monocular initialisation (k_init_finish in track_kernels.hip, csrc/init_wave.h) with its host
tail (csrc/init_host.cpp), compiled for x86 against tests/sim/hip_emu and run thread for thread on the CPU: the MI355X
comparisons of tests/test_gpu_init_finish.py with the restatement, bit for bit, without a GPU.  The emulated build is
libmvo_sim_init.so (tests/sim/init_finish.mk): the objects of libmvo_sim.so plus init_host.cpp."""
import ctypes as C
import os
import subprocess

import pytest

import test_gpu_init_finish as T
import test_gpu_regrow as T_regrow
from conftest import ROOT

SIM_DIR = os.path.join(ROOT, "tests", "sim")
SIM_INIT_LIB = os.path.join(SIM_DIR, "_build", "libmvo_sim_init.so")


@pytest.fixture(scope="module")
def simlib_init():
    subprocess.check_call(["make", "-C", SIM_DIR, "-f", "init_finish.mk", "-s", "-j8", "_build/libmvo_sim_init.so"])
    lib = C.CDLL(SIM_INIT_LIB)
    lib.mvo_last_error.restype = C.c_char_p
    lib.mvo_destroy.restype = None
    return lib


@pytest.fixture()
def simctx(mvo, simlib_init, monkeypatch):
    """A context of the product's Python mirror with its library handle pointing at the emulated build."""
    monkeypatch.setattr(mvo, "load_library", lambda: simlib_init)
    c = mvo.Context(0)
    yield c
    c.close()


@pytest.fixture()
def sim_init_as_the_library(simlib_init, tmp_path, monkeypatch):
    """The C++ test programs link libmvo_hip.so by name (DT_RUNPATH): a directory in front of the search path that holds
    the emulated build under that name makes the same binary run on the CPU."""
    d = tmp_path / "simlib"
    d.mkdir()
    os.symlink(SIM_INIT_LIB, d / "libmvo_hip.so")
    monkeypatch.setenv("LD_LIBRARY_PATH", str(d) + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    return d


@pytest.fixture(scope="module")
def F():
    return T.FR.Restatement()


@pytest.mark.parametrize("n,seed,planar", T.COUNT_CASES)
def test_inlier_counts_on_the_emulated_build(simctx, F, O, n, seed, planar):
    T.test_inlier_counts_around_the_wave_and_the_workgroup(simctx, F, O, n, seed, planar)


def test_four_matches_on_the_emulated_build(simctx, F, O):
    T.test_four_matches_choose_the_homography(simctx, F, O)


@pytest.mark.parametrize("kind,n,seed,frac,h_slot", T.SCENE_CASES)
def test_init_two_view_on_the_emulated_build(simctx, F, O, kind, n, seed, frac, h_slot):
    T.test_init_two_view_matches_the_restatement(simctx, F, O, kind, n, seed, frac, h_slot)


def test_initialisation_buffers_regrow_on_the_emulated_build(mvo, simctx, F, O):
    T_regrow.init_chain_steps(mvo, F, O)  # (simctx has pointed the package at the emulated build)


def test_parameters_boundary_and_no_solution_on_the_emulated_build(simctx, F, O):
    T.test_identity_reference_pose_and_other_parameters(simctx, F, O)
    T.boundary_cases(simctx, F, O)
    T.no_solution_cases(simctx, F, O)
