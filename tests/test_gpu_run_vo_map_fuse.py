"""run_vo with `map_point_fuse: 1` on the MI355X: tests/run_vo_map_fuse_body.py."""
import os

import pytest

import run_vo_map_fuse_body as B

pytestmark = pytest.mark.gpu


def test_run_vo_with_the_key_off_is_the_run_without_the_key(mvo, tmp_path):
    B.check_off(mvo, tmp_path, dict(os.environ))


@pytest.mark.parametrize("others", [False, True])
def test_run_vo_fuses_duplicate_map_points(mvo, tmp_path, others):
    B.check_fuse(mvo, tmp_path, dict(os.environ), others)
