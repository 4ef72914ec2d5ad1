"""run_vo with `tracking_match_by_projection: 1` on the emulated build (tests/sim/projection.mk in front of the library search
path): tests/run_vo_projection_body.py, without a GPU."""
import os

import run_vo_projection_body as B
import test_projection_sim as S


def test_run_vo_tracks_by_projection_on_the_emulated_build(mvo, tmp_path):
    S.build_simlib()
    (tmp_path / "simlib").mkdir()
    os.symlink(S.SIM_PROJECTION_LIB, tmp_path / "simlib" / "libmvo_hip.so")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = str(tmp_path / "simlib") + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    B.check(mvo, B.run(mvo, tmp_path / "on", True, env), B.run(mvo, tmp_path / "off", False, env))
