"""The fusion of duplicate map points (csrc/map_fuse_kernels.hip with its host side csrc/map_fuse_host.cpp) compiled for x86
against tests/sim/hip_emu and run thread for thread on the CPU: the MI355X comparisons of tests/test_gpu_map_fuse.py with the
numpy transcription, bit for bit, without a GPU.  The emulated build is libmvo_sim_map_fuse.so (tests/sim/map_fuse.mk): the
objects of libmvo_sim_map_refine.so plus the two new sources."""
import ctypes as C
import os
import subprocess

import pytest

import test_gpu_map_fuse as T
from conftest import ROOT

SIM_DIR = os.path.join(ROOT, "tests", "sim")
SIM_MAP_FUSE_LIB = os.path.join(SIM_DIR, "_build", "libmvo_sim_map_fuse.so")


def build_simlib():
    subprocess.check_call(["make", "-C", SIM_DIR, "-f", "map_fuse.mk", "-s", "-j8", "_build/libmvo_sim_map_fuse.so"])
    lib = C.CDLL(SIM_MAP_FUSE_LIB)
    lib.mvo_last_error.restype = C.c_char_p
    lib.mvo_destroy.restype = None
    return lib


@pytest.fixture(scope="module")
def simlib_map_fuse():
    return build_simlib()


@pytest.fixture()
def simmvo(mvo, simlib_map_fuse, monkeypatch):
    """The product's Python mirror with its library handle pointing at the emulated build."""
    monkeypatch.setattr(mvo, "load_library", lambda: simlib_map_fuse)
    return mvo


@pytest.fixture()
def simctx(simmvo):
    c = simmvo.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("n,F", T.CASES)
def test_search_on_the_emulated_build(simctx, n, F):
    T.test_search_bit_exact(simctx, n, F)


@pytest.mark.parametrize("n,F", T.CASES)
def test_fuse_on_the_emulated_build(simctx, n, F):
    T.test_fuse_bit_exact(simctx, n, F)


def test_repeated_and_alternating_calls_on_the_emulated_build(simctx):
    T.test_a_repeated_call_gives_the_same_bytes(simctx)
    T.test_a_smaller_call_after_a_larger_one(simctx)


def test_scales_on_the_emulated_build(simctx):
    T.test_scales(simctx)


@pytest.mark.parametrize("max_px,max_hamming", [(5.5, 30), (3.0, 0), (3.0, 256), (0.0, 50), (1.25, 40)])
def test_parameters_on_the_emulated_build(simctx, max_px, max_hamming):
    T.test_parameters_other_than_the_defaults(simctx, max_px, max_hamming)
    T.test_explicit_defaults_are_the_defaults(simctx)


def test_errors_on_the_emulated_build(simmvo, simctx):
    T.test_errors(simmvo, simctx)
