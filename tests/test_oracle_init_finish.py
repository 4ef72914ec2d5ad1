"""Known answers for the restatement of the finish of the monocular initialisation (tests/init_finish_restatement.cpp
via tests/finish_restate.py), on the CPU: the true pose up to the monocular scale and the assumed mean depth on a
noise-free scene, the kept set against analytic angles, every per-point quantity against a float64 numpy transcription
of the reference's loops fed the same float32 inputs, the keep list against the existing
mvo_retain_good_triangulation, the 19 / 20 boundary, each criterion on its own and deviation 12.

Tolerances: the transcription differs from the restatement only in the association of three- and four-term sums
(numpy's matrix products) and in preTranslatePoint3f's rounding to float, which the transcription repeats; every test
scene keeps its angles above 0.5 degrees, so acos is well conditioned and 1e-12 relative holds.  The analytic angles
are computed from the exact points; the restatement sees them rounded to float32 (relative 6e-8, a few 1e-6 degrees
at these depths), so the scenes are required to keep every analytic angle 1e-4 degrees away from a threshold."""
import numpy as np
import pytest

import finish_restate as FR
import h_restate as HR

DEG = 180.0 / 3.1415926   # vo.cpp:210


@pytest.fixture(scope="module")
def F(mvo):
    """The restatement of the product's entry points, which the library must export (dlsym, no GPU needed)."""
    lib = mvo.load_library()
    for sym in ("mvo_init_two_view", "mvo_debug_get_init_finish"):
        assert getattr(lib, sym) is not None
    assert all(hasattr(mvo.Context, m) for m in ("init_two_view", "debug_init_finish"))
    return FR.Restatement()


T_REF = np.eye(4)
T_REF[:3, :3] = HR.rot([0.3, -0.5, 1.0], 25.0)
T_REF[:3, 3] = [0.7, -1.3, 2.1]


def make(n, seed, rot_deg=6.0, t=(0.3, 0.05, 0.02), depth=(2.5, 8.0)):
    """A noise-free thick scene with its true motion in the form the E branch returns it: x2 = R x1 + t, |t| = 1 and
    the points of camera 1 in units of the baseline (float32), the pixels float32."""
    rng = np.random.RandomState(seed)
    K = HR.K_DEFAULT
    R = HR.rot([0.2, 1.0, 0.1], rot_deg)
    t = np.asarray(t, float)
    uv = rng.uniform([40, 40], [600, 440], (n, 2))
    rays = np.linalg.solve(K, np.c_[uv, np.ones(n)].T).T
    X1 = rays * rng.uniform(depth[0], depth[1], n)[:, None]
    p2 = (X1 @ R.T + t) @ K.T
    b = np.linalg.norm(t)
    return dict(p1=(X1 / b).astype(np.float32), X1=X1 / b, px1=uv.astype(np.float32),
                px2=(p2[:, :2] / p2[:, 2:]).astype(np.float32), R=R, t=t / b)


def analytic_angles(X1, R, t):
    """Angle at every exact point between the rays to the two camera centres (camera 1 frame), in the reference's degrees."""
    c2 = -R.T @ t
    a, b = -X1, c2 - X1
    cos = (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    return np.arccos(cos) * DEG


def transcription(p1, px1, px2, R, t, T_ref, prm):
    """vo.cpp:83-109, 126-166, 203-242 in float64 numpy on the same float32 inputs."""
    T = T_ref @ np.linalg.inv(np.block([[R, t[:, None]], [np.zeros((1, 3)), np.ones((1, 1))]]))
    pc = (p1.astype(np.float64) @ R.T + t).astype(np.float32)
    pw = (np.c_[pc.astype(np.float64), np.ones(len(pc))] @ T[:3].T).astype(np.float32).astype(np.float64)
    a, b = T[:3, 3] - pw, T_ref[:3, 3] - pw
    ang = np.arccos((a * b).sum(1) / (np.sqrt((a * a).sum(1)) * np.sqrt((b * b).sum(1)))) / 3.1415926 * 180.0
    med = np.sort(ang)[len(ang) // 2]
    keep = np.nonzero(~((ang < prm["min_triang_angle"]) | (ang / med > prm["max_ratio_to_median"])))[0]
    d = (px1 - px2).astype(np.float64)   # float differences, widened
    dist = np.sqrt((d * d).sum(1))
    pts = pc[keep]
    out = dict(angle=ang, pixdist=dist, keep=keep, mean_pixel_dist=dist[keep].mean(), mean_angle=ang[keep].mean(),
               median_angle=np.sort(ang[keep])[len(keep) // 2], min_angle=ang[keep].min(), max_angle=ang[keep].max())
    if len(keep) >= 20:
        out["mean_depth"] = pts[:, 2].astype(np.float64).mean()
        out["scale"] = prm["assumed_mean_depth"] / out["mean_depth"]
        out["pts"] = (pts.astype(np.float64) * out["scale"]).astype(np.float32)
        out["T"] = T_ref @ np.linalg.inv(np.block([[R, (t * out["scale"])[:, None]], [np.zeros((1, 3)), np.ones((1, 1))]]))
    return out


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if a.size else 0.0


STRICT = dict(min_triang_angle=3.0, max_ratio_to_median=1.5)


def test_true_pose_mean_depth_and_the_analytic_keep_set(F):
    s = make(300, 81)
    prm = dict(FR.DEFAULTS, **STRICT)
    f = F.finish(s["p1"], s["px1"], s["px2"], s["R"], s["t"], T_REF, **STRICT)
    ang = analytic_angles(s["X1"], s["R"], s["t"])
    med = np.sort(ang)[len(ang) // 2]
    margin = min(np.abs(ang - prm["min_triang_angle"]).min(), np.abs(ang - prm["max_ratio_to_median"] * med).min())
    assert margin > 1e-4, "the scene has an angle on a threshold: pick another seed"
    want = np.nonzero((ang >= prm["min_triang_angle"]) & (ang / med <= prm["max_ratio_to_median"]))[0]
    assert 20 <= len(want) < len(ang) and (ang < 3.0).any() and (ang / med > 1.5).any()
    assert np.array_equal(f["kept"], want)
    assert f["scaled"] and abs(f["pts3d_in_curr"][:, 2].astype(np.float64).mean() - 0.8) < 0.8 * 2.0 ** -22
    # the true pose of camera 2 up to the monocular scale: rotation T_ref R^T, centre T_ref (-R^T t) * scale
    T = f["T_w_c"]
    assert np.abs(T[:3, :3] - T_REF[:3, :3] @ s["R"].T).max() < 1e-12 and np.array_equal(T[3], [0, 0, 0, 1])
    c = T_REF[:3, :3] @ (-s["R"].T @ s["t"]) * f["scale"] + T_REF[:3, 3]
    assert np.abs(T[:3, 3] - c).max() < 1e-12
    assert np.abs(f["t"] - s["t"] * f["scale"]).max() < 1e-15


@pytest.mark.parametrize("n,seed,params", [(300, 81, STRICT), (257, 82, {}), (40, 83, dict(assumed_mean_depth=2.5))])
def test_against_the_float64_numpy_transcription(F, n, seed, params):
    s = make(n, seed)
    prm = dict(FR.DEFAULTS, **params)
    f = F.finish(s["p1"], s["px1"], s["px2"], s["R"], s["t"], T_REF, **params)
    ref = transcription(s["p1"], s["px1"], s["px2"], s["R"], s["t"], T_REF, prm)
    assert ref["angle"].min() >= 0.5
    assert np.array_equal(f["kept"], ref["keep"])
    assert rel(f["angle"], ref["angle"]) < 1e-12 and rel(f["pixdist"], ref["pixdist"]) < 1e-12
    assert rel(f["angles"], ref["angle"][ref["keep"]]) < 1e-12
    for k in ("mean_pixel_dist", "mean_angle", "median_angle", "min_angle", "max_angle", "mean_depth", "scale"):
        assert rel(f[k], ref[k]) < 1e-12, k
    assert np.abs(f["T_w_c"] - ref["T"]).max() < 1e-12
    # the scaled points: float32 roundings of products that agree to 1e-12
    assert np.abs(f["pts3d_in_curr"].astype(np.float64) - ref["pts"]).max() <= 2.0 ** -23 * np.abs(ref["pts"]).max()


def test_keep_list_and_angles_equal_retain_good_triangulation(mvo, F):
    """The finish keeps what the existing mvo_retain_good_triangulation keeps on the same p_curr and poses."""
    for n, seed, params in [(300, 81, STRICT), (257, 82, {})]:
        s = make(n, seed)
        prm = dict(FR.DEFAULTS, **params)
        f = F.finish(s["p1"], s["px1"], s["px2"], s["R"], s["t"], T_REF, **params)
        T_unscaled = F.compose(T_REF, s["R"], s["t"])
        keep, ang = mvo.retain_good_triangulation(f["p_curr"], T_unscaled, T_REF, prm["min_triang_angle"],
                                                  prm["max_ratio_to_median"])
        assert np.array_equal(keep, f["kept"]) and np.array_equal(ang, f["angle"])
        assert np.array_equal(ang[keep], f["angles"])


def test_the_19_20_boundary(F):
    for n in (19, 20):
        s = make(n, 84 + n)
        f = F.finish(s["p1"], s["px1"], s["px2"], s["R"], s["t"], T_REF)
        assert f["n_kept"] == n and f["criteria"][0]   # 19 >= min_inlier_matches = 15
        if n == 19:
            assert not f["scaled"] and np.array_equal(f["t"], s["t"]) and np.array_equal(f["pts3d_in_curr"], f["p_curr"])
            assert np.array_equal(f["T_w_c"], F.compose(T_REF, s["R"], s["t"]))
        else:
            assert f["scaled"] and f["scale"] > 0 and np.array_equal(f["t"], s["t"] * f["scale"])


def test_each_criterion_flips_on_its_own(F):
    good = make(100, 91)
    f = F.finish(good["p1"], good["px1"], good["px2"], good["R"], good["t"], T_REF)
    assert f["criteria"] == [True, True, True] and f["good"]
    few = make(10, 92)                                   # too few kept
    f = F.finish(few["p1"], few["px1"], few["px2"], few["R"], few["t"], T_REF)
    assert f["n_kept"] == 10 and f["criteria"] == [False, True, True] and not f["good"]
    short = make(100, 93, rot_deg=0.0)                   # no rotation: the parallax alone moves the pixels < 50
    f = F.finish(short["p1"], short["px1"], short["px2"], short["R"], short["t"], T_REF)
    assert f["mean_pixel_dist"] < 50 and f["criteria"] == [True, False, True] and not f["good"]
    far = make(100, 94, depth=(9.5, 16.0))               # every angle below 2 degrees, most of them above 1
    f = F.finish(far["p1"], far["px1"], far["px2"], far["R"], far["t"], T_REF)
    assert f["n_kept"] >= 50 and f["max_angle"] < 2 and f["median_angle"] < 2 and f["criteria"] == [True, True, False] and not f["good"]


def test_no_solution_is_deviation_12(F, O):
    s = make(3, 95)
    out = F.init_two_view(O, s["px1"], s["px2"], HR.K_DEFAULT, T_REF)
    assert out["poses"]["best"] == -1 and out["slot"] == -1 and out["n_kept"] == 0
    assert out["criteria"] == [False, False, False] and not out["good"] and np.array_equal(out["T_w_c"], T_REF)
