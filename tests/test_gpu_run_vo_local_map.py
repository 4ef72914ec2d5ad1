"""run_vo with `tracking_local_map: 1` on the MI355X: tests/run_vo_local_map_body.py."""
import os

import pytest

import run_vo_local_map_body as B

pytestmark = pytest.mark.gpu


def test_run_vo_with_the_key_off_is_the_run_without_the_key(mvo, tmp_path):
    B.check_off(mvo, tmp_path, dict(os.environ))


def test_run_vo_tracks_the_local_map(mvo, tmp_path):
    B.check_tracked(mvo, tmp_path, dict(os.environ))


def test_run_vo_with_the_key_alone_fails_with_the_message(mvo, tmp_path):
    B.check_alone(mvo, tmp_path, dict(os.environ))
