"""The ORB-SLAM style detector (csrc/orb_distribute_kernels.hip with its host side csrc/orb_distribute_host.cpp) compiled for
x86 against tests/sim/hip_emu and run thread for thread on the CPU: the MI355X comparisons of
tests/test_gpu_orb_distribute.py with the numpy transcription, bit for bit, without a GPU.  The emulated build is
libmvo_sim_orb_distribute.so (tests/sim/orb_distribute.mk): the objects of libmvo_sim_projection.so plus the two new sources."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_gpu_orb_distribute as T
from conftest import ROOT

SIM_DIR = os.path.join(ROOT, "tests", "sim")
SIM_LIB = os.path.join(SIM_DIR, "_build", "libmvo_sim_orb_distribute.so")


def build_simlib():
    subprocess.check_call(["make", "-C", SIM_DIR, "-f", "orb_distribute.mk", "-s", "-j8", "_build/libmvo_sim_orb_distribute.so"])
    lib = C.CDLL(SIM_LIB)
    lib.mvo_last_error.restype = C.c_char_p
    lib.mvo_destroy.restype = None
    return lib


@pytest.fixture(scope="module")
def simlib_orb_distribute():
    return build_simlib()


class HostTensor:  # "device memory" of the emulated runtime is host memory: stands in for torch's .cuda() tensors
    def __init__(self, a):
        self.a = np.array(a)

    def data_ptr(self):
        return self.a.ctypes.data


@pytest.fixture()
def simmvo(mvo, simlib_orb_distribute, monkeypatch):
    """The product's Python mirror with its library handle pointing at the emulated build."""
    monkeypatch.setattr(mvo, "load_library", lambda: simlib_orb_distribute)
    monkeypatch.setattr(T, "_to_device", HostTensor)
    return mvo


@pytest.fixture()
def simctx(simmvo):
    c = simmvo.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_candidates_and_keypoints_on_the_emulated_build(simmvo, simctx, name):
    T.test_candidates_and_keypoints_bit_exact(simmvo, simctx, name)


def test_descriptors_on_the_emulated_build(simmvo, simctx):
    T.test_descriptors_of_the_distributed_keypoints(simmvo, simctx)


def test_padded_stride_bgra_and_the_device_pointer_form_on_the_emulated_build(simmvo, simctx):
    T.test_padded_stride_bgra_and_the_device_pointer_form(simmvo, simctx)


@pytest.mark.parametrize("mode", ["latency", "throughput"])
def test_latency_and_throughput_contexts_on_the_emulated_build(simmvo, mode):
    T.test_latency_and_throughput_contexts(simmvo, mode)


def test_existing_detector_reconfiguration_and_errors_on_the_emulated_build(simmvo, simctx):
    T.test_the_existing_detector_is_untouched_by_a_distributed_call(simmvo)
    T.test_reconfiguration_and_errors(simmvo, simctx)
