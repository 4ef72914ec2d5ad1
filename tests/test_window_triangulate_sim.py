"""The triangulation of new map points against every buffered frame (csrc/window_triangulate_kernels.hip with its host side
csrc/window_triangulate_host.cpp) compiled for x86 against tests/sim/hip_emu and run thread for thread on the CPU: the MI355X
comparisons of tests/test_gpu_window_triangulate.py with the numpy transcription, bit for bit, without a GPU.  The emulated build is
libmvo_sim_window_triangulate.so (tests/sim/window_triangulate.mk): the objects of libmvo_sim_map_fuse.so plus the two new sources."""
import ctypes as C
import os
import subprocess

import pytest

import test_gpu_window_triangulate as T
from conftest import ROOT

SIM_DIR = os.path.join(ROOT, "tests", "sim")
SIM_WINDOW_LIB = os.path.join(SIM_DIR, "_build", "libmvo_sim_window_triangulate.so")


def build_simlib():
    subprocess.check_call(["make", "-C", SIM_DIR, "-f", "window_triangulate.mk", "-s", "-j8", "_build/libmvo_sim_window_triangulate.so"])
    lib = C.CDLL(SIM_WINDOW_LIB)
    lib.mvo_last_error.restype = C.c_char_p
    lib.mvo_destroy.restype = None
    return lib


@pytest.fixture(scope="module")
def simlib_window():
    return build_simlib()


@pytest.fixture()
def simmvo(mvo, simlib_window, monkeypatch):
    """The product's Python mirror with its library handle pointing at the emulated build."""
    monkeypatch.setattr(mvo, "load_library", lambda: simlib_window)
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
def test_window_triangulate_on_the_emulated_build(simctx, O, n, F):
    T.test_window_triangulate_bit_exact(simctx, O, n, F)


def test_every_status_bit_occurs_over_the_set():
    T.test_every_status_bit_occurs_over_the_set()


def test_a_pair_that_is_not_finite_on_the_emulated_build(simctx):
    T.test_a_pair_that_is_not_finite(simctx)


@pytest.mark.parametrize("n_pairs", [0, 1, 256, 257])
def test_pair_counts_on_the_emulated_build(simctx, n_pairs):
    T.test_pair_counts_around_the_verification_launch(simctx, n_pairs)


def test_repeated_and_alternating_calls_on_the_emulated_build(simctx):
    T.test_a_repeated_call_gives_the_same_bytes(simctx)
    T.test_a_smaller_call_between_two_larger_ones(simctx)


def test_scales_on_the_emulated_build(simctx):
    T.test_scales(simctx)


@pytest.mark.parametrize("k", range(len(T.PARAMS)))
def test_parameters_on_the_emulated_build(simctx, k):
    T.test_parameters_other_than_the_defaults(simctx, k)
    T.test_explicit_defaults_are_the_defaults(simctx)


def test_the_resident_map_is_left_alone_on_the_emulated_build(simctx):
    T.test_the_resident_map_is_left_alone(simctx)


def test_errors_on_the_emulated_build(simmvo, simctx):
    T.test_errors(simmvo, simctx)
