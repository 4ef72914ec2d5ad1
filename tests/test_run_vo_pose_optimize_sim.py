"""run_vo with `tracking_pose_by_optimization: 1` on the emulated build (tests/sim/pose_optimize.mk in front of the library search
path): tests/run_vo_pose_optimize_body.py, without a GPU."""
import os

import run_vo_pose_optimize_body as B
import test_pose_optimize_sim as S


def test_run_vo_takes_its_pose_from_the_optimisation_on_the_emulated_build(mvo, tmp_path):
    S.build_simlib()
    (tmp_path / "simlib").mkdir()
    os.symlink(S.SIM_POSE_OPTIMIZE_LIB, tmp_path / "simlib" / "libmvo_hip.so")
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = str(tmp_path / "simlib") + os.pathsep + env.get("LD_LIBRARY_PATH", "")
    B.check_off(mvo, tmp_path, env)
    B.check_optimised(mvo, tmp_path, env)
    B.check_alone(mvo, tmp_path, env)
