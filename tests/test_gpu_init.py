"""cv::findHomography of the monocular initialisation on the MI355X (k_h_hypotheses, k_h_mask, k_h_refine through
mvo_find_homography) against the test-side restatement (tests/homography_restatement.cpp), bit for bit: every
evaluated hypothesis' inlier count, the selected iteration, the loop length, the inlier list and the refined H.
tests/test_init_sim.py runs the same functions through the emulated build of the kernels."""
import numpy as np
import pytest

import h_restate as HR


@pytest.fixture(scope="module")
def R():
    return HR.Restatement()


def check_find_homography(ctx, R, src, dst, threshold=3.0, confidence=0.995):
    got = ctx.find_homography(src, dst, threshold, confidence)
    dbg = ctx.debug_homography()
    ref = R.find_homography(src, dst, threshold, confidence)
    assert (got["H"] is None) == (ref["H"] is None)
    assert np.array_equal(got["inliers"], ref["inliers"])
    n = len(src)
    if n < 4 or ref["n_subsets"] == 0:
        return got, dbg, ref
    run = ref["iters_run"]
    assert dbg["n_subsets"] == ref["n_subsets"]
    assert dbg["iters_run"] == run and dbg["evaluated"] >= run
    assert np.array_equal(dbg["counts"][:run], ref["counts"][:run])
    assert dbg["best_iter"] == ref["best_iter"]
    if ref["H"] is not None:
        assert np.array_equal(got["H"], ref["H"]), np.abs(got["H"] - ref["H"]).max()
        assert (dbg["lm_iters"], dbg["dlt"]) == (ref["lm_iters"], ref["dlt"])
    return got, dbg, ref


CASES = [  # (n, seed, two_view keywords)
    (4, 1, dict(planar=True, noise=0.0)),
    (5, 2, dict(planar=True, noise=0.5)),
    (60, 3, dict(planar=True, noise=0.5, outlier_frac=0.3)),
    (300, 4, dict(planar=True, noise=0.5)),
    (500, 5, dict(planar=False, noise=0.3)),
    (500, 6, dict(planar=False, noise=0.3, rotation_only=True)),
    (1000, 7, dict(planar=True, noise=0.7, outlier_frac=0.5)),
    (2000, 8, dict(planar=True, noise=0.5, outlier_frac=0.7)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed,kw", CASES)
def test_find_homography_matches_the_restatement(ctx, R, n, seed, kw):
    pr = HR.two_view(n, seed, **kw)
    got, dbg, ref = check_find_homography(ctx, R, pr["src"], pr["dst"])
    assert got["H"] is not None
    if kw.get("planar") and n >= 300:
        assert pr["inlier_gt"][got["inliers"]].all()


def full_loop_case(ctx, R):
    """Wrong matches only: no hypothesis ever gathers enough inliers to shorten the loop, all 2000 iterations run."""
    rng = np.random.RandomState(11)
    src = rng.uniform(0, 640, (300, 2)).astype(np.float32)
    dst = rng.uniform(0, 640, (300, 2)).astype(np.float32)
    _, dbg, ref = check_find_homography(ctx, R, src, dst, threshold=1.0)
    assert ref["iters_run"] == 2000 and dbg["evaluated"] == 2000


def degenerate_cases(ctx, R):
    pr = HR.two_view(40, 3, planar=True, noise=0.0)
    s, d = pr["src"], pr["dst"]
    for k in (0, 1, 3, 4):
        check_find_homography(ctx, R, s[:k], d[:k])
    x = np.arange(10, 250, 8.0)
    line = np.c_[x, 2 * x + 7].astype(np.float32)
    got, dbg, _ = check_find_homography(ctx, R, line, line + 3)
    assert got["H"] is None and dbg["n_subsets"] == 0 and len(dbg["counts"]) == 0
    same = np.tile(np.float32([[5, 5]]), (4, 1))
    assert check_find_homography(ctx, R, same, same)[0]["H"] is None
    for thr, conf in [(1.0, 0.999), (0.0, 0.5), (5.0, 0.9999999)]:
        check_find_homography(ctx, R, s, d + 0.25, thr, conf)


@pytest.mark.gpu
def test_find_homography_full_loop(ctx, R):
    full_loop_case(ctx, R)


@pytest.mark.gpu
def test_find_homography_degenerate_inputs(mvo, ctx, R):
    degenerate_cases(ctx, R)
    with pytest.raises(mvo.MvoError):
        ctx.find_homography(np.zeros((8, 2), np.float32), np.zeros((8, 2), np.float32), confidence=1.0)


@pytest.mark.gpu
def test_find_homography_leaves_the_essential_path_alone(mvo, O, ctx):
    """The E RANSAC shares the chunked loop with the homography: its outputs stay the oracle's."""
    kf = mvo.synth.keyframe_problem(n=400, seed=8)
    HR_ = HR.two_view(200, 2, planar=True)
    ctx.find_homography(HR_["src"], HR_["dst"])
    got = ctx.find_essential_inliers(kf["kp_ref"], kf["kp_cur"], kf["K"], 0.999, 1.0)
    ref = O.find_essential_inliers(kf["kp_ref"], kf["kp_cur"], kf["K"], 0.999, 1.0)
    dbg = ctx.debug_essential()
    assert np.array_equal(got, ref["inliers"]) and dbg["iters_run"] == ref["iters_run"]
