"""The robust motion-only pose optimisation (csrc/pose_optimize_kernels.hip with its host side csrc/pose_optimize_host.cpp) compiled
for x86 against tests/sim/hip_emu and run thread for thread on the CPU: the MI355X comparisons of tests/test_gpu_pose_optimize.py
with the numpy transcription, bit for bit, without a GPU.  The emulated build is libmvo_sim_pose_optimize.so
(tests/sim/pose_optimize.mk): the objects of libmvo_sim_window_triangulate.so plus the two new sources."""
import ctypes as C
import os
import subprocess

import pytest

import test_gpu_pose_optimize as T
from conftest import ROOT

SIM_DIR = os.path.join(ROOT, "tests", "sim")
SIM_POSE_OPTIMIZE_LIB = os.path.join(SIM_DIR, "_build", "libmvo_sim_pose_optimize.so")


def build_simlib():
    subprocess.check_call(["make", "-C", SIM_DIR, "-f", "pose_optimize.mk", "-s", "-j8", "_build/libmvo_sim_pose_optimize.so"])
    lib = C.CDLL(SIM_POSE_OPTIMIZE_LIB)
    lib.mvo_last_error.restype = C.c_char_p
    lib.mvo_destroy.restype = None
    return lib


@pytest.fixture(scope="module")
def simlib_pose_optimize():
    return build_simlib()


@pytest.fixture()
def simmvo(mvo, simlib_pose_optimize, monkeypatch):
    """The product's Python mirror with its library handle pointing at the emulated build."""
    monkeypatch.setattr(mvo, "load_library", lambda: simlib_pose_optimize)
    return mvo


@pytest.fixture()
def simctx(simmvo):
    c = simmvo.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("n", T.SHAPES)
def test_shapes_on_the_emulated_build(simctx, n):
    T.test_shapes_bit_exact(simctx, n)


@pytest.mark.parametrize("params", T.PARAMS, ids=lambda p: "-".join("%s=%g" % kv for kv in sorted(p.items())))
def test_parameters_on_the_emulated_build(simctx, params):
    T.test_parameters_other_than_the_defaults(simctx, params)


def test_every_status_on_the_emulated_build(simctx):
    T.test_every_status(simctx)


def test_a_second_call_on_the_emulated_build(simctx):
    T.test_a_second_call_with_fewer_observations(simctx)


def test_errors_on_the_emulated_build(simmvo, simctx):
    T.test_errors(simmvo, simctx)


def test_the_debug_getter_on_the_emulated_build(simmvo):
    T.test_the_debug_getter_before_the_first_call(simmvo)


@pytest.mark.parametrize("order", ["reverse", "shuffle"])
def test_the_fiber_order_does_not_matter(simmvo, monkeypatch, order):
    """A missing barrier in k_pose_optimize would show as a result that depends on the order the fibers of a workgroup run in."""
    monkeypatch.setenv("EMU_ORDER", order)
    c = simmvo.Context(0)
    try:
        T.test_shapes_bit_exact(c, 513)
    finally:
        c.close()
