"""run_vo with `map_point_create_from_window: 1` on the emulated build (tests/sim/window_triangulate.mk in front of the library search
path): tests/run_vo_window_triangulate_body.py, without a GPU."""
import os

import pytest

import run_vo_window_triangulate_body as B
import test_window_triangulate_sim as S


def sim_env(tmp_path):
    S.build_simlib()
    d = os.path.join(S.SIM_DIR, "_build", "as_libmvo_hip_window_triangulate")      # the emulated build under the product's name
    os.makedirs(d, exist_ok=True)
    if not os.path.islink(os.path.join(d, "libmvo_hip.so")):
        os.symlink(S.SIM_WINDOW_LIB, os.path.join(d, "libmvo_hip.so"))
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = d + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    return env


def test_run_vo_with_the_key_off_on_the_emulated_build(mvo, tmp_path):
    B.check_off(mvo, tmp_path, sim_env(tmp_path))


@pytest.mark.parametrize("others", [False, True])
def test_run_vo_creates_map_points_from_the_window_on_the_emulated_build(mvo, tmp_path, others):
    B.check_window(mvo, tmp_path, sim_env(tmp_path), others)


def test_a_library_without_the_entry_point_answers_the_key_with_an_error(mvo, tmp_path):
    """libmvo_sim_map_fuse.so (tests/sim/map_fuse.mk) is the emulated build WITHOUT the two new sources: run_vo asked for
    `map_point_create_from_window: 1` stops with an error instead of tracking without the step."""
    import subprocess

    import test_map_fuse_sim as D
    from test_gpu_run_vo import EXE, _write_dataset

    D.build_simlib()
    (tmp_path / "simlib").mkdir()
    os.symlink(D.SIM_MAP_FUSE_LIB, tmp_path / "simlib" / "libmvo_hip.so")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = str(tmp_path / "simlib") + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    cfg = _write_dataset(mvo, tmp_path, 7, 5, "map_point_create_from_window: 1\n")[3]
    r = subprocess.run([EXE, str(cfg)], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 1 and "has no mvo_window_triangulate" in r.stderr and "from the window" not in r.stdout
