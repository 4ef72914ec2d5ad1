"""run_vo with `map_point_fuse: 1` on the emulated build (tests/sim/map_fuse.mk in front of the library search path):
tests/run_vo_map_fuse_body.py, without a GPU."""
import os

import pytest

import run_vo_map_fuse_body as B
import test_map_fuse_sim as S


def sim_env(tmp_path):
    S.build_simlib()
    d = os.path.join(S.SIM_DIR, "_build", "as_libmvo_hip_map_fuse")      # the emulated build under the product's name
    os.makedirs(d, exist_ok=True)
    if not os.path.islink(os.path.join(d, "libmvo_hip.so")):
        os.symlink(S.SIM_MAP_FUSE_LIB, os.path.join(d, "libmvo_hip.so"))
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = d + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    return env


def test_run_vo_with_the_key_off_on_the_emulated_build(mvo, tmp_path):
    B.check_off(mvo, tmp_path, sim_env(tmp_path))


@pytest.mark.parametrize("others", [False, True])
def test_run_vo_fuses_duplicate_map_points_on_the_emulated_build(mvo, tmp_path, others):
    B.check_fuse(mvo, tmp_path, sim_env(tmp_path), others)


def test_a_library_without_the_entry_point_answers_the_key_with_an_error(mvo, tmp_path):
    """libmvo_sim_map_refine.so (tests/sim/map_refine.mk) is the emulated build WITHOUT the two fusion sources: run_vo asked for
    `map_point_fuse: 1` stops with an error instead of tracking without the fusion."""
    import subprocess

    import test_map_refine_sim as D
    from test_gpu_run_vo import EXE, _write_dataset

    D.build_simlib()
    (tmp_path / "simlib").mkdir()
    os.symlink(D.SIM_MAP_REFINE_LIB, tmp_path / "simlib" / "libmvo_hip.so")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = str(tmp_path / "simlib") + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    cfg = _write_dataset(mvo, tmp_path, 7, 5, "map_point_fuse: 1\n")[3]
    r = subprocess.run([EXE, str(cfg)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 1 and "has no mvo_map_fuse" in r.stderr and "map points fused" not in r.stdout
