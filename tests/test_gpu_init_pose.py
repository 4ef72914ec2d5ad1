"""The homography branch and the E / H choice of the monocular initialisation on the MI355X (k_h_decompose through
mvo_esti_motion_by_homography; k_h_decompose and k_init_triangulate through mvo_estimate_possible_relative_poses)
against the sequential restatement (tests/init_pose_restatement.cpp composed with the existing restatements by
tests/pose_restate.py), bit for bit: H, the raw decomposition, the rejection counts, the survivors, the solution
table, every slot's points, both scores, the ratio and the choice.  The composed call must also give what the three
single calls give on the same matches.  tests/test_init_pose_sim.py runs the same functions through the emulated
build of the kernels."""
import numpy as np
import pytest

import h_restate as HR
import init_restate as IR
import pose_restate as PR
from test_gpu_init_motion import CASES, same_float, scene, several_candidate_seed


@pytest.fixture(scope="module")
def P():
    return PR.Restatement()


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def check_decomposition(dbg, dec):
    assert dbg["count"] == dec["count"]
    assert dbg["rotation_only"] == dec["rotation_only"] and dbg["index"] == dec["index"]
    for k in ("Hn", "w", "Rs", "ts", "normals"):
        assert same(dbg[k], dec[k]), (k, dbg[k], dec[k])


def check_homography(ctx, P, kp1, kp2, K, threshold=3.0, confidence=0.995):
    got = ctx.esti_motion_by_homography(kp1, kp2, IR.kdict(K), threshold, confidence)
    dbg = ctx.debug_homography_decomposition()
    ref = P.esti_motion_by_homography(kp1, kp2, K, threshold, confidence)
    assert got["found"] == ref["found"]
    assert np.array_equal(got["inliers"], ref["inliers"])
    if not ref["found"]:
        assert got["H"] is None and got["Rs"] == [] and dbg["count"] == 0
        return got, ref
    assert same(got["H"], ref["H"])
    check_decomposition(dbg, ref["dec"])
    assert np.array_equal(dbg["rejected"], ref["rejected"]), (dbg["rejected"], ref["rejected"])
    assert len(got["Rs"]) == len(ref["survivors"])
    for k in ("Rs", "ts", "normals"):
        for x, y in zip(got[k], ref[k]):
            assert same(x, y), k
    return got, ref


def check_poses(ctx, P, O, kp1, kp2, K, motion_cam2_to_cam1=True, singles=True):
    kd = IR.kdict(K)
    got = ctx.estimate_possible_relative_poses(kp1, kp2, kd, motion_cam2_to_cam1=motion_cam2_to_cam1)
    dbg = ctx.debug_homography_decomposition()
    ref = P.estimate_possible_relative_poses(O, kp1, kp2, K, motion_cam2_to_cam1=motion_cam2_to_cam1)
    assert got["best"] == ref["best"], (got["best"], ref["best"], got["ratio"], ref["ratio"])
    for k in ("ratio", "score_e", "score_h"):
        assert same_float(got[k], ref[k]), (k, got[k], ref[k])
    for k in ("E", "H"):
        assert (got[k] is None) == (ref[k] is None) and (got[k] is None or same(got[k], ref[k])), k
    assert np.array_equal(got["inliers_e"], ref["inliers_e"]) and np.array_equal(got["inliers_h"], ref["inliers_h"])
    if ref["H"] is not None:
        check_decomposition(dbg, ref["h"]["dec"])
        assert np.array_equal(dbg["rejected"], ref["h"]["rejected"])
    else:
        assert dbg["count"] == 0
    assert len(got["solutions"]) == len(ref["solutions"])
    for g, r in zip(got["solutions"], ref["solutions"]):
        assert (g is None) == (r is None)
        if r is None:
            continue
        assert g["kind"] == r["kind"] and g["candidate"] == r["candidate"]
        for k in ("R", "t"):
            assert same(g[k], r[k]), (k, g[k], r[k])
        assert (g["normal"] is None) == (r["normal"] is None) and (r["normal"] is None or same(g["normal"], r["normal"]))
        assert np.array_equal(g["inliers"], r["inliers"])
        assert g["pts3d"].dtype == np.float32 and same(g["pts3d"], r["pts3d"])
    if singles:  # the composed call computes what the single calls compute
        e = ctx.esti_motion_by_essential(kp1, kp2, kd)
        h = ctx.find_homography(kp1, kp2)
        assert np.array_equal(e["inliers"], got["inliers_e"]) and np.array_equal(h["inliers"], got["inliers_h"])
        assert (e["E"] is None and got["E"] is None) or same(e["E"], got["E"])
        H = None if h["H"] is None else IR.scale_by_22(h["H"])
        assert (H is None and got["H"] is None) or same(H, got["H"])
        if e["found"]:
            s0 = got["solutions"][0]
            if motion_cam2_to_cam1:
                assert same(e["R"], s0["R"]) and same(e["t"], s0["t"])
            tri = ctx.triangulate_points(kp1[e["inliers"]], kp2[e["inliers"]], kd, e["R"], e["t"])
            assert same(tri[0], s0["pts3d"])
        sc = ctx.check_init_scores(kp1, kp2, kd, got["E"], got["inliers_e"], got["H"], got["inliers_h"])
        assert same_float(sc["score_e"], got["score_e"]) and same_float(sc["score_h"], got["score_h"])
    return got, ref


POSE_CASES = CASES + [("planar", 4, 40, 0.0), ("planar", 300, 41, 0.2), ("rotation", 60, 42, 0.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,seed,frac", POSE_CASES)
def test_relative_poses_match_the_restatement(ctx, P, O, kind, n, seed, frac):
    pr = scene(kind, n, seed, frac)
    check_poses(ctx, P, O, pr["src"], pr["dst"], pr["K"])
    check_homography(ctx, P, pr["src"], pr["dst"], pr["K"])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,seed,frac", [("planar", 500, 24, 0.5), ("thick", 1000, 27, 0.5), ("planar", 60, 32, 0.7)])
def test_relative_poses_cam1_to_cam2(ctx, P, O, kind, n, seed, frac):
    pr = scene(kind, n, seed, frac)
    check_poses(ctx, P, O, pr["src"], pr["dst"], pr["K"], motion_cam2_to_cam1=False)


def deviation_cases(ctx, P, O):
    """The three declared deviations and the empty input."""
    pr = HR.two_view(60, 33, planar=True, noise=0.3)
    a, b, K = pr["src"], pr["dst"], pr["K"]
    # 9: E has no model (n == 4: H only; five matches with several five-point candidates)
    got, _ = check_poses(ctx, P, O, a[:4], b[:4], K)
    assert got["solutions"][0] is None and got["score_e"] == 0 and got["H"] is not None
    p5 = HR.two_view(5, several_candidate_seed(O), planar=False, noise=0.0)
    got, _ = check_poses(ctx, P, O, p5["src"], p5["dst"], p5["K"])
    assert got["solutions"][0] is None and got["score_e"] == 0
    # 10: H has no model (n < 4) -- and with E absent too, NaN ratio: best = -1
    for m in (0, 3):
        got, _ = check_poses(ctx, P, O, a[:m], b[:m], K)
        assert got["H"] is None and got["score_h"] == 0 and len(got["solutions"]) == 1 and got["best"] == -1
        assert np.isnan(got["ratio"])
    # 11: ratio > 0.5 with zero H survivors: a rotation-only H (its candidate has a zero normal)
    rot = HR.two_view(200, 34, planar=False, rotation_only=True, noise=0.0)
    got, _ = check_poses(ctx, P, O, rot["src"], rot["dst"], rot["K"])
    dbg = ctx.debug_homography_decomposition()
    assert dbg["count"] == 1 and dbg["rotation_only"] and len(got["solutions"]) == 1
    if got["ratio"] > 0.5:
        assert got["best"] == -1


@pytest.mark.gpu
def test_deviation_cases(ctx, P, O):
    deviation_cases(ctx, P, O)


@pytest.mark.gpu
def test_argument_errors(mvo, ctx):
    pr = HR.two_view(60, 35)
    K = IR.kdict(pr["K"])
    with pytest.raises(mvo.MvoError):
        ctx.esti_motion_by_homography(pr["src"], pr["dst"], K, confidence=1.0)
    with pytest.raises(mvo.MvoError):
        ctx.estimate_possible_relative_poses(pr["src"], pr["dst"], K, prob=0.0)
