"""The stand-alone sanitizer programs of tests/sim (each with its own main, linked with hip_emu/emu_runtime.cpp, built with
-fsanitize=address,undefined): DevBuf of csrc/mvo_internal.h, the host tail of the pose-gated matchers,
and the staged call of csrc/staged_call.h with the scratch of the launches over every buffered frame.  A failed build is a
failure, not a skip; a sanitizer report (a leaked emulated allocation included) ends the program non-zero."""
import os
import subprocess

import pytest

from conftest import ROOT

SIM_DIR = os.path.join(ROOT, "tests", "sim")


@pytest.mark.parametrize("name", ["dev_buf_check", "guided_host_check", "staged_call_check"])
def test_sanitizer_program(name):
    r = subprocess.run(["make", "-C", SIM_DIR, "-f", name + ".mk", "check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and name + " ok" in r.stdout.splitlines(), r.stdout[-3000:] + r.stderr[-3000:]
