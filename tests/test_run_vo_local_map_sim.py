"""run_vo with `tracking_local_map: 1` on the emulated build (tests/sim/local_map_vo.mk in front of the library search path):
tests/run_vo_local_map_body.py, without a GPU."""
import os

import run_vo_local_map_body as B
import test_local_map_host as S


def test_run_vo_tracks_the_local_map_on_the_emulated_build(mvo, tmp_path):
    (tmp_path / "simlib").mkdir()
    os.symlink(S.build_simlib_vo(), tmp_path / "simlib" / "libmvo_hip.so")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = str(tmp_path / "simlib") + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    B.check_off(mvo, tmp_path, env)
    B.check_tracked(mvo, tmp_path, env)
    B.check_alone(mvo, tmp_path, env)
