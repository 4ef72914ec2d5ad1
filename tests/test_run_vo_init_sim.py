"""host/driver/run_vo under `init_from_images: 1` on the emulated build of the kernels (tests/sim: every GPU thread a fiber on the
CPU), against the oracle chain from images: the body of tests/test_gpu_run_vo_init.py (tests/run_vo_init_body.py) without a GPU.
The emulation takes about two seconds per frame, so the four runs of the module (two from images, one with the thresholds out of
reach, one seeded from the ground truth without the key) are started together and checked one after the other; the byte
comparison of `init_from_images: 0` with the absent key is left to the MI355X test."""
import pytest

import run_vo_init_body as B
from test_init_finish_sim import SIM_INIT_LIB, simlib_init  # noqa: F401  (fixture)


@pytest.fixture(scope="module")
def runs(simlib_init, tmp_path_factory):
    """The C++ programs link libmvo_hip.so by name (DT_RUNPATH): a directory in front of the search path that holds the emulated
    build under that name makes the same binary run on the CPU (as tests/test_init_finish_sim.py's sim_init_as_the_library)."""
    import os
    tmp = tmp_path_factory.mktemp("run_vo_init_sim")
    (tmp / "simlib").mkdir()
    os.symlink(SIM_INIT_LIB, tmp / "simlib" / "libmvo_hip.so")
    mp = pytest.MonkeyPatch()
    mp.setenv("LD_LIBRARY_PATH", str(tmp / "simlib") + os.pathsep + os.environ.get("LD_LIBRARY_PATH", ""))
    try:
        data = B.write_images(tmp)
        (tmp / "images_only").mkdir()
        (tmp / "seeded").mkdir()
        started = dict(init=B.start_runs_from_images(tmp / "images_only", data, timeout=1200),
                       never=B.start_run_out_of_reach(tmp / "images_only", data, timeout=1200),
                       seeded=B.start_seeded_runs(tmp / "seeded", data, with_key_zero=False, timeout=1200))
    finally:
        mp.undo()
    yield started
    for r in started["init"] + [started["never"]] + started["seeded"]:
        if r.proc.poll() is None:
            r.proc.kill()
            r.proc.communicate()


def test_run_vo_from_images_equals_the_oracle_chain_on_the_emulated_build(O, runs):
    B.run_equals_the_chain(O, runs["init"])


def test_run_vo_never_initialises_with_thresholds_out_of_reach_on_the_emulated_build(runs):
    B.never_initialises(runs["never"])


def test_run_vo_without_the_key_is_the_seeded_run_on_the_emulated_build(O, runs):
    B.seeded_run_is_unchanged(O, runs["seeded"])
