"""host/driver/run_vo under `init_from_images: 1` on the MI355X: a folder of PNG frames and a config.yaml without any ground truth,
against the oracle chain from images (tests/vo_chain_init.py).  The body is tests/run_vo_init_body.py, shared with
tests/test_run_vo_init_sim.py.  Every frame: keypoints and descriptors bit for bit.  Every initialisation frame: the matches with
the first keyframe, every integer of the INIT record, the slot's inliers, the kept matches, the f32 points and the pose bit for
bit (the finish is declared arithmetic, tests/test_gpu_init_finish.py).  After initialisation: what
test_run_vo_equals_the_oracle_chain compares, with its tolerances."""
import pytest

import run_vo_init_body as B

pytestmark = pytest.mark.gpu


def test_run_vo_from_images_equals_the_oracle_chain(mvo, O, tmp_path):
    runs = B.start_runs_from_images(tmp_path, B.write_images(tmp_path))
    B.run_equals_the_chain(O, runs)


def test_run_vo_never_initialises_with_thresholds_out_of_reach(mvo, tmp_path):
    B.never_initialises(B.start_run_out_of_reach(tmp_path, B.write_images(tmp_path)))


def test_run_vo_without_the_key_is_the_seeded_run(mvo, O, tmp_path):
    B.seeded_run_is_unchanged(O, B.start_seeded_runs(tmp_path, B.write_images(tmp_path)))
