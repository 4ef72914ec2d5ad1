"""The finish of the monocular initialisation on the MI355X (k_init_finish through mvo_init_two_view, with the host
tail of csrc/init_host.cpp) against the sequential restatement (tests/init_finish_restatement.cpp composed with
tests/pose_restate.py by tests/finish_restate.py), bit for bit and without tolerances: what the kernel wrote per inlier
of the chosen slot (p_curr, the cosine, the pixel distance), every field of mvo_init_result, and `poses` equal to what
mvo_estimate_possible_relative_poses returns on its own.  tests/test_init_finish_sim.py runs the same functions through
the emulated build of the kernels.

Inlier counts of the chosen slot: 4 and 5 (the fewest a RANSAC model can have: the H of four matches, the E of five
-- a count of 1 cannot be reached through the call, findHomography / findEssentialMat return no model below their
sample size), 63 / 64 / 65 (one wave), 255 / 256 / 257 (one workgroup), about 1800 (n = 2000, several workgroups)."""
import numpy as np
import pytest

import finish_restate as FR
import h_restate as HR
import init_restate as IR
from test_gpu_init_motion import CASES, same_float, scene
from test_gpu_init_pose import same

T_REF = np.eye(4)
T_REF[:3, :3] = HR.rot([0.3, -0.5, 1.0], 25.0)
T_REF[:3, 3] = [0.7, -1.3, 2.1]


@pytest.fixture(scope="module")
def F():
    return FR.Restatement()


def exact_scene(n, seed, planar=False, baseline=0.3):
    """n noise-free matches (every one an inlier of the model RANSAC finds) of a thick or planar scene."""
    pr = HR.two_view(n, seed, planar=planar, noise=0.0)
    if baseline != 0.3:
        pr = scaled_baseline(pr, n, seed, baseline)
    return pr


def scaled_baseline(pr, n, seed, baseline):
    """The thick scene of HR.two_view(n, seed, planar=False) seen with the translation scaled to |t| ~ baseline and a
    rotation scaled with it."""
    rng = np.random.RandomState(seed)
    K = pr["K"]
    uv = rng.uniform([40, 40], [600, 440], (n, 2))
    rays = np.linalg.solve(K, np.c_[uv, np.ones(n)].T).T
    X1 = rays * rng.uniform(2.5, 8.0, n)[:, None]
    f = baseline / 0.3
    R = HR.rot([0.2, 1.0, 0.1], 6.0 * f)
    t = pr["t"] * f
    p2 = (X1 @ R.T + t) @ K.T
    return dict(pr, src=uv.astype(np.float32), dst=(p2[:, :2] / p2[:, 2:]).astype(np.float32), R=R, t=t)


def check_init(ctx, F, O, kp1, kp2, K, T_ref=T_REF, poses_alone=True, **params):
    kd = IR.kdict(K)
    got = ctx.init_two_view(kp1, kp2, kd, T_ref, **params)
    dbg = ctx.debug_init_finish()
    ref = F.init_two_view(O, kp1, kp2, K, T_ref, **params)
    # what k_init_finish wrote
    for k in ("p_curr", "cosang", "pixdist"):
        assert dbg[k].dtype == ref["finish"][k].dtype and np.array_equal(dbg[k], ref["finish"][k]), k
    # every field of mvo_init_result
    for k in ("slot", "n_slot_inliers", "n_kept", "scaled", "criteria", "good"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    for k in ("matches_for_3d", "pts3d_in_curr", "angles", "R", "t", "T_w_c"):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    for k in ("mean_depth", "scale", "mean_pixel_dist", "mean_angle", "median_angle", "min_angle", "max_angle"):
        assert same_float(got[k], ref[k]), (k, got[k], ref[k])
    # poses: the restatement's, and what the composed call returns on its own for the same matches
    check_same_poses(got["poses"], ref["poses"])
    if poses_alone:
        check_same_poses(got["poses"], ctx.estimate_possible_relative_poses(kp1, kp2, kd))
    return got, ref


def check_same_poses(g, r):
    assert g["best"] == r["best"]
    for k in ("ratio", "score_e", "score_h"):
        assert same_float(g[k], r[k]), k
    for k in ("E", "H"):
        assert (g[k] is None) == (r[k] is None) and (g[k] is None or same(g[k], r[k])), k
    assert np.array_equal(g["inliers_e"], r["inliers_e"]) and np.array_equal(g["inliers_h"], r["inliers_h"])
    assert len(g["solutions"]) == len(r["solutions"])
    for a, b in zip(g["solutions"], r["solutions"]):
        assert (a is None) == (b is None)
        if a is None:
            continue
        assert a["kind"] == b["kind"] and a["candidate"] == b["candidate"]
        assert same(a["R"], b["R"]) and same(a["t"], b["t"]) and same(a["pts3d"], b["pts3d"])
        assert np.array_equal(a["inliers"], b["inliers"])


# (n, seed, planar): noise-free scenes, every match an inlier of the chosen slot.  Five matches of this thick scene
# give several five-point candidates, so E has no model (deviation 7) and the H of the five matches is chosen.
COUNT_CASES = [(5, 1, False), (63, 61, False), (64, 62, False), (65, 63, False), (255, 64, False), (256, 65, True),
               (257, 66, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,seed,planar", COUNT_CASES)
def test_inlier_counts_around_the_wave_and_the_workgroup(ctx, F, O, n, seed, planar):
    pr = exact_scene(n, seed, planar)
    got, _ = check_init(ctx, F, O, pr["src"], pr["dst"], pr["K"])
    assert got["n_slot_inliers"] == n and (got["slot"] >= 1) == (planar or n == 5)


@pytest.mark.gpu
def test_four_matches_choose_the_homography(ctx, F, O):
    """n = 4: E has no model (deviation 9), the H of the four matches has four inliers."""
    pr = exact_scene(60, 33, planar=True)
    got, _ = check_init(ctx, F, O, pr["src"][:4], pr["dst"][:4], pr["K"])
    assert got["slot"] >= 1 and got["n_slot_inliers"] == 4 and got["poses"]["solutions"][0] is None


# (scene kind, n, seed, wrong-match fraction, an H slot is chosen): scenes of tests/test_gpu_init_motion.py.  The thick
# scenes choose slot 0; the noise-free plane chooses an H slot behind a present E slot (the slot's points do not start
# the table, the motion comes from k_h_decompose); the noisy plane with 50 % wrong matches scores E higher and
# triangulates badly with it (the keep rule drops nine tenths of the slot).
SCENE_CASES = [CASES[2] + (False,), CASES[3] + (False,), CASES[6] + (False,), CASES[8] + (True,),
               ("thick", 2000, 36, 0.1, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,seed,frac,h_slot", SCENE_CASES)
def test_init_two_view_matches_the_restatement(ctx, F, O, kind, n, seed, frac, h_slot):
    pr = scene(kind, n, seed, frac)
    got, _ = check_init(ctx, F, O, pr["src"], pr["dst"], pr["K"])
    assert (got["slot"] >= 1) == h_slot and got["poses"]["solutions"][0] is not None
    if kind == "planar" and not h_slot:
        assert got["n_kept"] < got["n_slot_inliers"] // 5
    if n == 2000 and kind == "thick":
        assert 1700 <= got["n_slot_inliers"] <= 1900


@pytest.mark.gpu
def test_identity_reference_pose_and_other_parameters(ctx, F, O):
    pr = scene("thick", 500, 23, 0.0)
    check_init(ctx, F, O, pr["src"], pr["dst"], pr["K"], T_ref=None)
    check_init(ctx, F, O, pr["src"], pr["dst"], pr["K"], min_triang_angle=3.0, max_ratio_to_median=1.5,
               assumed_mean_depth=2.0, min_inlier_matches=400, min_pixel_dist=10.0, min_median_triangulation_angle=1.0)


def boundary_cases(ctx, F, O):
    """19 kept: no scaling, t stays a unit vector, criteria_0 still holds (19 >= 15); 20 kept: scaled."""
    for n, seed in ((19, 71), (20, 72)):
        pr = exact_scene(n, seed)
        got, _ = check_init(ctx, F, O, pr["src"], pr["dst"], pr["K"])
        assert got["slot"] == 0 and got["n_kept"] == n and got["criteria"][0]
        assert got["scaled"] == (n == 20)
        if n == 19:
            assert got["scale"] == 0 and same(got["t"], got["poses"]["solutions"][0]["t"])
        else:
            assert got["scale"] > 0 and not same(got["t"], got["poses"]["solutions"][0]["t"])


@pytest.mark.gpu
def test_the_19_20_boundary(ctx, F, O):
    boundary_cases(ctx, F, O)


def no_solution_cases(ctx, F, O):
    """best == -1 (deviation 12): nothing launched, the reference pose, no criterion holds."""
    pr = exact_scene(60, 33)
    for m in (0, 3):
        got, _ = check_init(ctx, F, O, pr["src"][:m], pr["dst"][:m], pr["K"])
        assert got["poses"]["best"] == -1 and got["slot"] == -1 and got["n_kept"] == 0 and not got["good"]
        assert not any(got["criteria"]) and same(got["T_w_c"], T_REF)
        assert len(ctx.debug_init_finish()["cosang"]) == 0


@pytest.mark.gpu
def test_no_solution(ctx, F, O):
    no_solution_cases(ctx, F, O)


@pytest.mark.gpu
def test_argument_errors(mvo, ctx):
    pr = exact_scene(60, 35)
    with pytest.raises(mvo.MvoError):
        ctx.init_two_view(pr["src"], pr["dst"], IR.kdict(pr["K"]), prob=0.0)
