"""run_vo with `map_point_refine_positions: 1` on the MI355X: tests/run_vo_map_refine_body.py."""
import os

import pytest

import run_vo_map_refine_body as B

pytestmark = pytest.mark.gpu


def test_run_vo_with_the_key_off_is_the_run_without_the_key(mvo, tmp_path):
    B.check_off(mvo, tmp_path, dict(os.environ))


@pytest.mark.parametrize("refresh", [False, True])
def test_run_vo_refines_the_map_point_positions(mvo, tmp_path, refresh):
    B.check_refine(mvo, tmp_path, dict(os.environ), refresh)
