"""run_vo with `tracking_match_by_projection: 1` on the MI355X: tests/run_vo_projection_body.py."""
import os

import pytest

import run_vo_projection_body as B

pytestmark = pytest.mark.gpu


def test_run_vo_tracks_by_projection(mvo, tmp_path):
    env = dict(os.environ)
    B.check(mvo, B.run(mvo, tmp_path / "on", True, env), B.run(mvo, tmp_path / "off", False, env))
