"""run_vo with `orb_distribute_keypoints: 1` on the emulated build (tests/sim/orb_distribute.mk in front of the library search
path): tests/run_vo_orb_distribute_body.py, without a GPU."""
import os

import run_vo_orb_distribute_body as B
import test_orb_distribute_sim as S


def test_run_vo_extracts_the_orb_slam_way_on_the_emulated_build(mvo, tmp_path):
    S.build_simlib()
    (tmp_path / "simlib").mkdir()
    os.symlink(S.SIM_LIB, tmp_path / "simlib" / "libmvo_hip.so")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = str(tmp_path / "simlib") + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    B.check(B.run(mvo, tmp_path / "on", True, env), B.run(mvo, tmp_path / "off", False, env))
