"""Tracking the local map (csrc/local_map_kernels.hip with its host side csrc/local_map_host.cpp) compiled for x86 against
tests/sim/hip_emu and run thread for thread on the CPU: the MI355X comparisons of tests/test_gpu_local_map.py with the numpy
transcription, bit for bit, without a GPU.  The emulated build is libmvo_sim_local_map.so (tests/sim/local_map.mk): the objects
of libmvo_sim_projection.so plus the two new sources."""
import ctypes as C
import os
import subprocess

import pytest

import test_gpu_local_map as T
from conftest import ROOT
from test_projection_sim import HostTensor

SIM_DIR = os.path.join(ROOT, "tests", "sim")
SIM_LOCAL_MAP_LIB = os.path.join(SIM_DIR, "_build", "libmvo_sim_local_map.so")


def build_simlib():
    subprocess.check_call(["make", "-C", SIM_DIR, "-f", "local_map.mk", "-s", "-j8", "_build/libmvo_sim_local_map.so"])
    lib = C.CDLL(SIM_LOCAL_MAP_LIB)
    lib.mvo_last_error.restype = C.c_char_p
    lib.mvo_destroy.restype = None
    return lib


@pytest.fixture(scope="module")
def simlib_local_map():
    return build_simlib()


@pytest.fixture()
def simmvo(mvo, simlib_local_map, monkeypatch):
    """The product's Python mirror with its library handle pointing at the emulated build."""
    monkeypatch.setattr(mvo, "load_library", lambda: simlib_local_map)
    monkeypatch.setattr(T, "_to_device", HostTensor)
    return mvo


@pytest.fixture()
def simctx(simmvo):
    c = simmvo.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("L", T.LEVELS)
@pytest.mark.parametrize("n_map", T.MAP_SIZES)
def test_scenes_on_the_emulated_build(simctx, n_map, L):
    T.test_scenes_bit_exact(simctx, n_map, L)


def test_every_large_scene_makes_every_clause_decide():
    for L in T.LEVELS:
        for n_map in (257, 700):
            for nt in (255, 256, 257, 1100):
                T.check_guard(n_map, L, nt)


def test_hand_worked_cases_on_the_emulated_build(simctx):
    T.test_hand_worked_cases(simctx)


def test_idle_wave_other_params_and_the_device_pointer_form_on_the_emulated_build(simctx):
    T.test_idle_wave_other_params_and_the_device_pointer_form(simctx)


def test_a_smaller_map_and_a_reupload_on_the_emulated_build(simmvo):
    T.test_a_smaller_map_on_the_same_ctx_and_a_reupload(simmvo)


def test_errors_on_the_emulated_build(simmvo, simctx):
    T.test_errors_write_nothing(simmvo, simctx)
