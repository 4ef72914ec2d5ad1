"""The pose-guided matcher (csrc/epipolar_kernels.hip with its host side csrc/epipolar_host.cpp) compiled for x86 against
tests/sim/hip_emu and run thread for thread on the CPU: the MI355X comparisons of tests/test_gpu_epipolar_match.py with the
numpy transcription, bit for bit, without a GPU.  The emulated build is libmvo_sim_epipolar.so (tests/sim/epipolar.mk): the
objects of libmvo_sim_undistort.so plus the two new sources."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_gpu_epipolar_match as T
from conftest import ROOT

SIM_DIR = os.path.join(ROOT, "tests", "sim")
SIM_EPIPOLAR_LIB = os.path.join(SIM_DIR, "_build", "libmvo_sim_epipolar.so")


def build_simlib():
    subprocess.check_call(["make", "-C", SIM_DIR, "-f", "epipolar.mk", "-s", "-j8", "_build/libmvo_sim_epipolar.so"])
    lib = C.CDLL(SIM_EPIPOLAR_LIB)
    lib.mvo_last_error.restype = C.c_char_p
    lib.mvo_destroy.restype = None
    return lib


@pytest.fixture(scope="module")
def simlib_epipolar():
    return build_simlib()


class HostTensor:  # "device memory" of the emulated runtime is host memory: stands in for torch's .cuda() tensors
    def __init__(self, a):
        self.a = np.array(a)

    def data_ptr(self):
        return self.a.ctypes.data


@pytest.fixture()
def simmvo(mvo, simlib_epipolar, monkeypatch):
    """The product's Python mirror with its library handle pointing at the emulated build."""
    monkeypatch.setattr(mvo, "load_library", lambda: simlib_epipolar)
    monkeypatch.setattr(T, "_to_device", HostTensor)
    return mvo


@pytest.fixture()
def simctx(simmvo):
    c = simmvo.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("kind", ["perturbed", "ties"])
@pytest.mark.parametrize("nq,nt", T.SHAPES)
def test_raw_call_on_the_emulated_build(simmvo, simctx, nq, nt, kind, scaled):
    T.test_raw_call_bit_exact(simmvo, simctx, nq, nt, kind, scaled)


def test_gate_scene_and_filter_on_the_emulated_build(simctx):
    T.test_exact_gate_and_zero_f(simctx)
    T.test_filter_ceiling_ratio_single_candidate_and_one_query_per_train(simctx)


def test_two_view_scene_on_the_emulated_build(simctx):
    T.test_two_view_scene_every_partner_found(simctx)


def test_device_pointer_form_and_the_largest_train_set_on_the_emulated_build(simmvo, simctx):
    T.test_device_pointer_form_equals_the_host_form(simmvo, simctx)
    T.test_the_largest_train_set(simmvo, simctx)


def test_partial_scratch_regrow_on_the_emulated_build(simmvo):
    T.test_partial_scratch_regrows_between_calls(simmvo)


def test_errors_and_fundamental_from_poses_on_the_emulated_build(simmvo, simctx):
    T.test_errors(simmvo, simctx)
    T.test_fundamental_from_poses(simmvo)
