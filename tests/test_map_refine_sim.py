"""The map-point position refinement (csrc/map_refine_kernels.hip with its host side csrc/map_refine_host.cpp) compiled for x86
against tests/sim/hip_emu and run thread for thread on the CPU: the MI355X comparisons of tests/test_gpu_map_refine.py with the
numpy transcription, bit for bit, without a GPU.  The emulated build is libmvo_sim_map_refine.so (tests/sim/map_refine.mk): the
objects of libmvo_sim_map_refresh.so plus the two new sources."""
import ctypes as C
import os
import subprocess

import pytest

import test_gpu_map_refine as T
from conftest import ROOT

SIM_DIR = os.path.join(ROOT, "tests", "sim")
SIM_MAP_REFINE_LIB = os.path.join(SIM_DIR, "_build", "libmvo_sim_map_refine.so")


def build_simlib():
    subprocess.check_call(["make", "-C", SIM_DIR, "-f", "map_refine.mk", "-s", "-j8", "_build/libmvo_sim_map_refine.so"])
    lib = C.CDLL(SIM_MAP_REFINE_LIB)
    lib.mvo_last_error.restype = C.c_char_p
    lib.mvo_destroy.restype = None
    return lib


@pytest.fixture(scope="module")
def simlib_map_refine():
    return build_simlib()


@pytest.fixture()
def simmvo(mvo, simlib_map_refine, monkeypatch):
    """The product's Python mirror with its library handle pointing at the emulated build."""
    monkeypatch.setattr(mvo, "load_library", lambda: simlib_map_refine)
    return mvo


@pytest.fixture()
def simctx(simmvo):
    c = simmvo.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("n,n_frames", T.CASES)
def test_refine_on_the_emulated_build(simctx, n, n_frames):
    T.test_refine_bit_exact(simctx, n, n_frames)


@pytest.mark.parametrize("m_obs", [2, 64])
def test_a_single_point_on_the_emulated_build(simctx, m_obs):
    T.test_a_single_point_with_2_and_64_observations(simctx, m_obs)


def test_parameters_on_the_emulated_build(simctx):
    T.test_parameters_other_than_the_defaults(simctx)


def test_a_second_call_and_moved_positions_on_the_emulated_build(simctx):
    T.test_a_second_call_starts_from_the_refined_positions(simctx)
    T.test_moved_positions_are_what_the_next_call_starts_from(simctx)


def test_the_projection_matcher_on_the_emulated_build(simctx):
    T.test_the_projection_matcher_projects_the_refined_positions(simctx)


def test_errors_on_the_emulated_build(simmvo, simctx):
    T.test_errors(simmvo, simctx)
