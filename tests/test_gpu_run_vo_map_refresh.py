"""run_vo with `map_point_refresh: 1` on the MI355X: tests/run_vo_map_refresh_body.py."""
import os

import pytest

import run_vo_map_refresh_body as B

pytestmark = pytest.mark.gpu


def test_run_vo_with_the_key_off_is_the_run_without_the_key(mvo, tmp_path):
    B.check_off(mvo, tmp_path, dict(os.environ))


@pytest.mark.parametrize("projection", [False, True])
def test_run_vo_refreshes_the_map_points(mvo, tmp_path, projection):
    B.check_refresh(mvo, tmp_path, dict(os.environ), projection)
