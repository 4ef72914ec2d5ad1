"""run_vo with `orb_distribute_keypoints: 1` on the MI355X: tests/run_vo_orb_distribute_body.py."""
import os

import pytest

import run_vo_orb_distribute_body as B

pytestmark = pytest.mark.gpu


def test_run_vo_extracts_the_orb_slam_way(mvo, tmp_path):
    env = dict(os.environ)
    B.check(B.run(mvo, tmp_path / "on", True, env), B.run(mvo, tmp_path / "off", False, env))
