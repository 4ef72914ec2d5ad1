"""The map-point refresh (csrc/map_refresh_kernels.hip with its host side csrc/map_refresh_host.cpp) compiled for x86 against
tests/sim/hip_emu and run thread for thread on the CPU: the MI355X comparisons of tests/test_gpu_map_refresh.py with the numpy
transcription, bit for bit, without a GPU.  The emulated build is libmvo_sim_map_refresh.so (tests/sim/map_refresh.mk): the
objects of libmvo_sim_orb_distribute.so plus the two new sources."""
import ctypes as C
import os
import subprocess

import pytest

import test_gpu_map_refresh as T
from conftest import ROOT

SIM_DIR = os.path.join(ROOT, "tests", "sim")
SIM_MAP_REFRESH_LIB = os.path.join(SIM_DIR, "_build", "libmvo_sim_map_refresh.so")


def build_simlib():
    subprocess.check_call(["make", "-C", SIM_DIR, "-f", "map_refresh.mk", "-s", "-j8", "_build/libmvo_sim_map_refresh.so"])
    lib = C.CDLL(SIM_MAP_REFRESH_LIB)
    lib.mvo_last_error.restype = C.c_char_p
    lib.mvo_destroy.restype = None
    return lib


@pytest.fixture(scope="module")
def simlib_map_refresh():
    return build_simlib()


@pytest.fixture()
def simmvo(mvo, simlib_map_refresh, monkeypatch):
    """The product's Python mirror with its library handle pointing at the emulated build."""
    monkeypatch.setattr(mvo, "load_library", lambda: simlib_map_refresh)
    return mvo


@pytest.fixture()
def simctx(simmvo):
    c = simmvo.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("flip", T.FLIP_RATES)
@pytest.mark.parametrize("n", T.MAP_SIZES)
def test_refresh_on_the_emulated_build(simctx, n, flip):
    T.test_refresh_bit_exact(simctx, n, flip)


@pytest.mark.parametrize("m_obs", [1, 2, 64])
def test_a_single_point_on_the_emulated_build(simctx, m_obs):
    T.test_a_single_point_with_1_2_64_observations(simctx, m_obs)


def test_a_camera_at_the_point_on_the_emulated_build(simctx):
    T.test_a_camera_at_the_point_gives_nan_written_as_it_comes(simctx)


def test_moved_positions_and_a_second_refresh_on_the_emulated_build(simctx):
    T.test_moved_positions_are_what_the_next_refresh_uses(simctx)
    T.test_a_second_refresh_with_the_same_observations_changes_nothing(simctx)


def test_the_projection_matcher_on_the_emulated_build(simctx):
    T.test_the_projection_matcher_finds_the_chosen_descriptors_at_distance_0(simctx)


def test_errors_on_the_emulated_build(simmvo, simctx):
    T.test_errors(simmvo, simctx)
