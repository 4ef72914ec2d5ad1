"""The undistortion kernels (csrc/undistort_kernels.hip) with their host side (csrc/undistort_host.cpp), compiled for x86
against tests/sim/hip_emu and run thread for thread on the CPU: the MI355X comparisons of tests/test_gpu_undistort.py with the
numpy transcription, bit for bit, without a GPU.  The emulated build is libmvo_sim_undistort.so (tests/sim/undistort.mk): the
objects of libmvo_sim.so plus init_host.cpp (run_vo's start from images) and the two new sources.  Case D runs in full here as
well, map and 640 x 480 x 3 remap: one fiber per pixel takes about a second."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_gpu_undistort as T
from conftest import ROOT

SIM_DIR = os.path.join(ROOT, "tests", "sim")
SIM_UNDISTORT_LIB = os.path.join(SIM_DIR, "_build", "libmvo_sim_undistort.so")


@pytest.fixture(scope="module")
def simlib_undistort():
    subprocess.check_call(["make", "-C", SIM_DIR, "-f", "undistort.mk", "-s", "-j8", "_build/libmvo_sim_undistort.so"])
    lib = C.CDLL(SIM_UNDISTORT_LIB)
    lib.mvo_last_error.restype = C.c_char_p
    lib.mvo_destroy.restype = None
    return lib


class HostTensor:  # "device memory" of the emulated runtime is host memory: stands in for torch's .cuda() tensors
    def __init__(self, a):
        self.a = np.array(a)

    def data_ptr(self):
        return self.a.ctypes.data


@pytest.fixture()
def simmvo(mvo, simlib_undistort, monkeypatch):
    """The product's Python mirror with its library handle pointing at the emulated build."""
    monkeypatch.setattr(mvo, "load_library", lambda: simlib_undistort)
    monkeypatch.setattr(T, "_to_device", HostTensor)
    monkeypatch.setattr(T, "_to_host", lambda t: t.a)
    return mvo


@pytest.fixture()
def simctx(simmvo):
    c = simmvo.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name,ch", [("A", 1), ("A", 3), ("B", 1), ("D", 3)])
def test_map_and_image_on_the_emulated_build(simctx, name, ch):
    T.test_map_and_image_equal_the_transcription(simctx, name, ch)


def test_strides_and_the_device_pointer_form_on_the_emulated_build(simctx):
    T.test_four_channels_with_padded_rows(simctx)
    T.test_device_pointer_form_equals_the_host_form(simctx)


def test_configurations_on_the_emulated_build(simctx):
    T.test_eight_coefficients_map(simctx)
    T.test_zero_coefficients_return_the_input(simctx)
    T.test_configure_again_replaces_the_map(simctx)


def test_errors_on_the_emulated_build(simmvo):
    T.test_errors(simmvo)


def test_run_vo_undistorts_on_the_emulated_build(simmvo, tmp_path, monkeypatch):
    """The C++ program links libmvo_hip.so by name (DT_RUNPATH): a directory in front of the search path that holds the
    emulated build under that name makes the same binary run on the CPU.  The three runs are started together."""
    (tmp_path / "simlib").mkdir()
    os.symlink(SIM_UNDISTORT_LIB, tmp_path / "simlib" / "libmvo_hip.so")
    monkeypatch.setenv("LD_LIBRARY_PATH", str(tmp_path / "simlib") + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    data = T.write_run_images(tmp_path)
    runs = T.start_runs(tmp_path, data, timeout=1200)
    try:
        T.run_vo_wiring(simmvo, runs, data)
    finally:
        for r in runs.values():
            if r.proc.poll() is None:
                r.proc.kill()
                r.proc.communicate()
