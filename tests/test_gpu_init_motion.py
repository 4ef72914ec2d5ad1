"""The essential-matrix branch of the monocular initialisation and the ORB-SLAM E / H scores on the MI355X
(k_em_hypotheses, k_em_mask, k_recover_pose through mvo_esti_motion_by_essential; k_init_scores through
mvo_check_init_scores) against the test-side restatement (tests/init_motion_restatement.cpp on the oracle's RANSAC),
bit for bit: the scaled E, the four recoverPose counts, the chosen combination, R, t, the decomposition, the per-match
masks, the inlier list, both scores and both kept lists.  tests/test_init_motion_sim.py runs the same functions through
the emulated build of the kernels."""
import numpy as np
import pytest

import h_restate as HR
import init_restate as IR


@pytest.fixture(scope="module")
def R():
    return IR.Restatement()


def far_view(n, seed, outlier_frac=0.0, noise=0.3):
    """A thick scene with depths from 3 to 40 (the baseline is 0.3): the points past 50 baselines fail recoverPose's
    distance threshold."""
    rng = np.random.RandomState(seed)
    K = HR.K_DEFAULT
    Rt = HR.rot([0.2, 1.0, 0.1], 4.0)
    t = np.array([0.3, 0.0, 0.0])
    uv = rng.uniform([40, 40], [600, 440], (n, 2))
    rays = np.linalg.solve(K, np.c_[uv, np.ones(n)].T).T
    X1 = rays * rng.uniform(3.0, 40.0, n)[:, None]
    X2 = X1 @ Rt.T + t
    p2 = X2 @ K.T
    uv2 = p2[:, :2] / p2[:, 2:] + (rng.normal(0, noise, (n, 2)) if noise else 0)
    n_out = int(round(outlier_frac * n))
    if n_out:
        idx = rng.choice(n, n_out, replace=False)
        uv2[idx] = rng.uniform([0, 0], [640, 480], (n_out, 2))
    return dict(src=uv.astype(np.float32), dst=uv2.astype(np.float32), R=Rt, t=t, K=K, X1=X1, X2=X2)


def scene(kind, n, seed, outlier_frac):
    if kind == "far":
        return far_view(n, seed, outlier_frac)
    kw = dict(planar=kind == "planar", rotation_only=kind == "rotation", noise=0.5, outlier_frac=outlier_frac)
    return HR.two_view(n, seed, **kw)


def same_float(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def check_esti(ctx, R, O, kp1, kp2, K, prob=0.999, threshold=1.0):
    got = ctx.esti_motion_by_essential(kp1, kp2, IR.kdict(K), prob, threshold)
    dbg = ctx.debug_recover_pose()
    ref = R.esti_motion_by_essential(O, kp1, kp2, K, prob, threshold)
    assert got["found"] == ref["found"]
    assert np.array_equal(got["inliers"], ref["inliers"])
    if not ref["found"]:
        assert dbg["chosen"] == -1 and not dbg["good"].any() and len(dbg["masks"]) == 0
        return got, dbg, ref
    rp = ref["rp"]
    assert np.array_equal(dbg["masks"], rp["masks"]), np.nonzero(dbg["masks"] != rp["masks"])[0][:10]
    assert np.array_equal(dbg["good"], rp["good"]) and dbg["chosen"] == rp["chosen"]
    for k in ("R1", "R2"):
        assert np.array_equal(dbg[k], rp[k], equal_nan=True), k
    assert np.array_equal(dbg["t"], rp["tdec"], equal_nan=True)
    for k in ("E", "R", "t"):
        assert np.array_equal(got[k], ref[k], equal_nan=True), (k, got[k], ref[k])
    return got, dbg, ref


def check_scores(ctx, R, kp1, kp2, K, E, inl_e, H, inl_h, sigma=1.0):
    got = ctx.check_init_scores(kp1, kp2, IR.kdict(K), E, inl_e, H, inl_h, sigma)
    ref = R.check_init_scores(kp1, kp2, K, E, inl_e, H, inl_h, sigma)
    assert same_float(got["score_e"], ref["score_e"]), (got["score_e"], ref["score_e"])
    assert same_float(got["score_h"], ref["score_h"]), (got["score_h"], ref["score_h"])
    assert np.array_equal(got["kept_e"], ref["kept_e"]) and np.array_equal(got["kept_h"], ref["kept_h"])
    return got, ref


def check_pipeline(ctx, R, O, kp1, kp2, K):
    """Both models as the reference computes them, then both scores from the device outputs."""
    got, _, _ = check_esti(ctx, R, O, kp1, kp2, K)
    h = ctx.find_homography(kp1, kp2)
    H = None if h["H"] is None else IR.scale_by_22(h["H"])
    E = got["E"] if got["found"] else None
    return check_scores(ctx, R, kp1, kp2, K, E, got["inliers"], H, h["inliers"])


CASES = [  # (scene kind, n, seed, wrong-match fraction)
    ("thick", 5, 21, 0.0),
    ("thick", 60, 22, 0.3),
    ("thick", 500, 23, 0.0),
    ("planar", 500, 24, 0.5),
    ("rotation", 500, 25, 0.0),
    ("far", 1000, 26, 0.3),
    ("thick", 1000, 27, 0.5),
    ("thick", 2000, 28, 0.7),
    ("planar", 2000, 29, 0.0),
    ("far", 2000, 30, 0.0),
    ("rotation", 1000, 31, 0.3),
    ("planar", 60, 32, 0.7),
]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,seed,frac", CASES)
def test_esti_motion_and_scores_match_the_restatement(ctx, R, O, kind, n, seed, frac):
    pr = scene(kind, n, seed, frac)
    check_pipeline(ctx, R, O, pr["src"], pr["dst"], pr["K"])


def degenerate_cases(ctx, R, O):
    pr = HR.two_view(60, 33, planar=False, noise=0.3)
    a, b, K = pr["src"], pr["dst"], pr["K"]
    for m in (0, 3, 4):
        got, dbg, _ = check_esti(ctx, R, O, a[:m], b[:m], K)
        assert not got["found"]
    # five matches whose five-point system has several real solutions: no model (deviation 7)
    seed = several_candidate_seed(O)
    p5 = HR.two_view(5, seed, planar=False, noise=0.0)
    got, _, _ = check_esti(ctx, R, O, p5["src"], p5["dst"], p5["K"])
    assert not got["found"]
    # identical views: degenerate five-point systems
    check_esti(ctx, R, O, a, a, K)
    # a NULL model scores 0 and keeps nothing; an empty list scores 0
    g = check_esti(ctx, R, O, a, b, K)[0]
    out, _ = check_scores(ctx, R, a, b, K, None, g["inliers"], None, g["inliers"])
    assert out["score_e"] == 0 and out["score_h"] == 0 and len(out["kept_e"]) == 0 and len(out["kept_h"]) == 0
    check_scores(ctx, R, a, b, K, g["E"], [], np.eye(3), np.arange(60))
    # a match on the epipole: NaN, as the reference's loop gives it
    ep = epipole_case(g["E"], K)
    check_scores(ctx, R, ep[0], ep[1], K, g["E"], np.arange(len(ep[0])), None, None)
    # sigma other than 1, repeated list entries, a singular H
    check_scores(ctx, R, a, b, K, g["E"], np.r_[g["inliers"], g["inliers"][:7]], np.ones((3, 3)), np.arange(60), sigma=0.7)


def several_candidate_seed(O):
    for seed in range(200):
        p5 = HR.two_view(5, seed, planar=False, noise=0.0)
        if O.find_essential_inliers(p5["src"], p5["dst"], IR.kdict(p5["K"]))["n_models"] > 1:
            return seed
    raise AssertionError("no five-match scene with several candidates")


def epipole_case(E, K):
    """Matches whose first point is the right null vector of F21 (a2 = b2 = 0 there up to rounding)."""
    F = np.linalg.inv(K).T @ E @ np.linalg.inv(K)
    _, _, Vt = np.linalg.svd(F)
    e = Vt[2] / Vt[2][2]
    p1 = np.array([[e[0], e[1]], [100.0, 120.0], [e[0], e[1]]], np.float32)
    p2 = np.array([[300.0, 200.0], [310.0, 205.0], [e[0] + 1, e[1]]], np.float32)
    return p1, p2


@pytest.mark.gpu
def test_degenerate_inputs(ctx, R, O):
    degenerate_cases(ctx, R, O)


@pytest.mark.gpu
def test_argument_errors(mvo, ctx):
    pr = HR.two_view(60, 34, planar=False)
    K = IR.kdict(pr["K"])
    with pytest.raises(mvo.MvoError):
        ctx.esti_motion_by_essential(pr["src"], pr["dst"], K, prob=1.0)
    with pytest.raises(mvo.MvoError):
        ctx.check_init_scores(pr["src"], pr["dst"], K, np.eye(3), [0, 60], None, None)
    with pytest.raises(mvo.MvoError):
        ctx.check_init_scores(pr["src"], pr["dst"], K, None, None, np.eye(3), [-1])
