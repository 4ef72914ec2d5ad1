"""run_vo with `map_point_create_from_window: 1` on the MI355X: tests/run_vo_window_triangulate_body.py."""
import os

import pytest

import run_vo_window_triangulate_body as B

pytestmark = pytest.mark.gpu


def test_run_vo_with_the_key_off_is_the_run_without_the_key(mvo, tmp_path):
    B.check_off(mvo, tmp_path, dict(os.environ))


@pytest.mark.parametrize("others", [False, True])
def test_run_vo_creates_map_points_from_the_window(mvo, tmp_path, others):
    B.check_window(mvo, tmp_path, dict(os.environ), others)
