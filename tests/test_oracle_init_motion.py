"""Known answers for the restatement of estiMotionByEssential's recoverPose and of the ORB-SLAM E / H scores
(tests/init_motion_restatement.cpp via tests/init_restate.py), on the CPU: the true motion from the true E, the
distance threshold on a far scene, recoverPose's counts against an independent numpy restatement (numpy.linalg.svd),
both scores against a float64 numpy transcription of the reference's loops, and the degenerate inputs."""
import numpy as np
import pytest

import h_restate as HR
import init_restate as IR
from test_gpu_init_motion import epipole_case, far_view, several_candidate_seed


@pytest.fixture(scope="module")
def R():
    return IR.Restatement()


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def normalised(kp, K):
    """(p - pp) / focal with focal = (fx + fy) / 2 and pp the float copy of (cx, cy), as recoverPose sees the points."""
    f = (K[0, 0] + K[1, 1]) / 2
    pp = np.array([K[0, 2], K[1, 2]], np.float32).astype(np.float64)
    return (np.asarray(kp, np.float32).astype(np.float64) - pp) / f


def numpy_recover_pose(kp1, kp2, K, E, mask=None, margin=1e-9):
    """recoverPose restated with numpy.linalg.svd: per combination (R, t) the pass flags of every match and the flags
    of the matches within `margin` (relative) of a threshold."""
    q1, q2 = normalised(kp1, K), normalised(kp2, K)
    n = len(q1)
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1.0]])
    R1, R2, t = U @ W @ Vt, U @ W.T @ Vt, U[:, 2]
    out = []
    for Rc, tc in ((R1, t), (R2, t), (R1, -t), (R2, -t)):
        P = np.c_[Rc, tc]
        P0 = np.c_[np.eye(3), np.zeros(3)]
        A = np.stack([q1[:, :1] * P0[2] - P0[0], q1[:, 1:] * P0[2] - P0[1], q2[:, :1] * P[2] - P[0],
                      q2[:, 1:] * P[2] - P[1]], axis=1)
        Q = np.linalg.svd(A)[2][:, 3, :]
        X = Q / Q[:, 3:]
        z = X @ P[2]
        ok = (Q[:, 2] * Q[:, 3] > 0) & (X[:, 2] < 50) & (z > 0) & (z < 50)
        if mask is not None:
            ok &= mask.astype(bool)
        near = (np.abs(X[:, 2] - 50) < 50 * margin) | (np.abs(z) < margin) | (np.abs(z - 50) < 50 * margin) | \
               (np.abs(X[:, 2]) < margin)
        out.append(dict(R=Rc, t=tc, ok=ok, near=near))
    return out


def test_true_essential_matrix_gives_the_true_motion(R):
    for seed in (41, 42, 43):
        pr = HR.two_view(300, seed, planar=False, noise=0.0)
        Et = skew(pr["t"]) @ pr["R"]
        rp = R.recover_pose(pr["src"], pr["dst"], pr["K"], Et * 3.7)
        assert np.abs(rp["R"] - pr["R"]).max() < 1e-9
        assert np.abs(rp["t"] - pr["t"] / np.linalg.norm(pr["t"])).max() < 1e-9
        assert np.abs(rp["E"] - Et / Et[2, 2]).max() < 1e-12 * np.abs(Et / Et[2, 2]).max()
        c = rp["chosen"]
        assert rp["good"][c] == 300 and all(rp["good"][k] < 300 for k in range(4) if k != c)
        assert np.array_equal(rp["masks"] >> c & 1, np.ones(300, np.uint8))
        # the RANSAC mask is ANDed in
        mask = np.arange(300) % 3 != 0
        rp2 = R.recover_pose(pr["src"], pr["dst"], pr["K"], Et, mask.astype(np.uint8))
        assert rp2["good"][c] == mask.sum() and not (rp2["masks"][~mask]).any()


def test_ransac_essential_matrix_on_noise_free_thick_scenes(R, O):
    for seed in (44, 45):
        pr = HR.two_view(400, seed, planar=False, noise=0.0)
        ref = R.esti_motion_by_essential(O, pr["src"], pr["dst"], pr["K"])
        assert ref["found"] and len(ref["inliers"]) == 400
        # the pixels are float32: the fitted E carries their rounding (about 1e-7 of the normalised coordinates)
        assert np.abs(ref["R"] - pr["R"]).max() < 1e-5
        assert np.abs(ref["t"] - pr["t"] / np.linalg.norm(pr["t"])).max() < 1e-4
        assert ref["E"][2, 2] == ref["E_raw"][2, 2] * (1.0 / ref["E_raw"][2, 2])
        rp = ref["rp"]
        c = rp["chosen"]
        assert rp["good"][c] == 400 and all(rp["good"][k] < 400 for k in range(4) if k != c)


def test_distance_threshold_on_a_far_scene(R):
    pr = far_view(800, 46, noise=0.0)
    Et = skew(pr["t"]) @ pr["R"]
    rp = R.recover_pose(pr["src"], pr["dst"], pr["K"], Et)
    base = np.linalg.norm(pr["t"])
    d1, d2 = pr["X1"][:, 2] / base, pr["X2"][:, 2] / base
    far = (d1 >= 50) | (d2 >= 50)
    clear = (np.abs(d1 - 50) > 1e-3) & (np.abs(d2 - 50) > 1e-3)
    c = rp["chosen"]
    assert np.abs(rp["R"] - pr["R"]).max() < 1e-9
    assert 100 < far.sum() < 700
    bit = (rp["masks"] >> c & 1).astype(bool)
    assert np.array_equal(bit[clear], ~far[clear])
    assert rp["good"][c] == bit.sum() < 800


@pytest.mark.parametrize("kind,n,seed,frac", [("thick", 200, 47, 0.0), ("thick", 500, 48, 0.3), ("planar", 400, 49, 0.5),
                                              ("far", 600, 50, 0.2), ("rotation", 300, 51, 0.0)])
def test_counts_match_a_numpy_restatement(R, O, kind, n, seed, frac):
    from test_gpu_init_motion import scene
    pr = scene(kind, n, seed, frac)
    ref = R.esti_motion_by_essential(O, pr["src"], pr["dst"], pr["K"])
    assert ref["found"]
    rp = ref["rp"]
    mask = np.zeros(n, np.uint8)
    mask[ref["inliers"]] = 1
    combos = numpy_recover_pose(pr["src"], pr["dst"], pr["K"], ref["E"], mask)
    for k in range(4):  # the numpy SVD may order the combinations differently: pair them by (R, t)
        Rk = rp["R1"] if k % 2 == 0 else rp["R2"]
        tk = rp["tdec"] if k < 2 else -rp["tdec"]
        m = [c for c in combos if np.abs(c["R"] - Rk).max() < 1e-9 and np.abs(c["t"] - tk).max() < 1e-9]
        assert len(m) == 1, k
        bit = (rp["masks"] >> k & 1).astype(bool)
        keep = ~m[0]["near"]
        assert np.array_equal(bit[keep], m[0]["ok"][keep])
        if keep.all():
            assert rp["good"][k] == m[0]["ok"].sum()
        assert rp["good"][k] == bit.sum()


def numpy_scores(kp1, kp2, K, E, inl_e, H, inl_h, sigma=1.0):
    """The reference's two loops (motion_estimation.cpp:501-664) in float64, sequentially."""
    p1 = np.asarray(kp1, np.float32).astype(np.float64)
    p2 = np.asarray(kp2, np.float32).astype(np.float64)
    inv = 1.0 / (sigma * sigma)
    se, ke = 0.0, []
    if E is not None:
        Ki = np.linalg.inv(K)
        F = Ki.T @ E @ Ki
        for i in inl_e:
            (u1, v1), (u2, v2) = p1[i], p2[i]
            good = True
            a2, b2, c2 = F @ [u1, v1, 1.0]
            chi = (a2 * u2 + b2 * v2 + c2) ** 2 / (a2 * a2 + b2 * b2) * inv
            if chi > 3.841:
                good = False
            else:
                se += 5.991 - chi
            a1, b1, c1 = F.T @ [u2, v2, 1.0]
            chi = (a1 * u1 + b1 * v1 + c1) ** 2 / (a1 * a1 + b1 * b1) * inv
            if chi > 3.841:
                good = False
            else:
                se += 5.991 - chi
            if good:
                ke.append(i)
    sh, kh = 0.0, []
    if H is not None:
        Hi = np.linalg.inv(H)
        for i in inl_h:
            (u1, v1), (u2, v2) = p1[i], p2[i]
            good = True
            x = Hi @ [u2, v2, 1.0]
            chi = ((u1 - x[0] / x[2]) ** 2 + (v1 - x[1] / x[2]) ** 2) * inv
            if chi > 5.991:
                good = False
            else:
                sh += 5.991 - chi
            x = H @ [u1, v1, 1.0]
            chi = ((u2 - x[0] / x[2]) ** 2 + (v2 - x[1] / x[2]) ** 2) * inv
            if chi > 5.991:
                good = False
            else:
                sh += 5.991 - chi
            if good:
                kh.append(i)
    return se, np.array(ke, np.int32), sh, np.array(kh, np.int32)


@pytest.mark.parametrize("kind,n,seed,frac,sigma", [("thick", 300, 52, 0.3, 1.0), ("planar", 500, 53, 0.5, 1.0),
                                                    ("planar", 200, 54, 0.0, 0.8), ("rotation", 300, 55, 0.2, 1.0)])
def test_scores_match_a_numpy_transcription(R, O, kind, n, seed, frac, sigma):
    from test_gpu_init_motion import scene
    pr = scene(kind, n, seed, frac)
    ref = R.esti_motion_by_essential(O, pr["src"], pr["dst"], pr["K"])
    h = R_h().find_homography(pr["src"], pr["dst"])
    assert ref["found"] and h["H"] is not None
    H = IR.scale_by_22(h["H"])
    got = R.check_init_scores(pr["src"], pr["dst"], pr["K"], ref["E"], ref["inliers"], H, h["inliers"], sigma)
    se, ke, sh, kh = numpy_scores(pr["src"], pr["dst"], pr["K"], ref["E"], ref["inliers"], H, h["inliers"], sigma)
    assert abs(got["score_e"] - se) <= 1e-12 * abs(se) and abs(got["score_h"] - sh) <= 1e-12 * abs(sh)
    assert np.array_equal(got["kept_e"], ke) and np.array_equal(got["kept_h"], kh)
    assert 0 < len(ke) <= len(ref["inliers"]) and 0 < len(kh) <= len(h["inliers"])


_HR = []


def R_h():
    if not _HR:
        _HR.append(HR.Restatement())
    return _HR[0]


def test_invert3_is_the_closed_form(R):
    rng = np.random.RandomState(56)
    for _ in range(20):
        M = rng.normal(size=(3, 3))
        assert np.allclose(R.invert3(M), np.linalg.inv(M), rtol=1e-12, atol=1e-12)
    K = HR.K_DEFAULT
    assert np.array_equal(R.invert3(K), np.array([[1 / 500, 0, -320 / 500], [0, 1 / 500, -240 / 500], [0, 0, 1]]))
    assert not R.invert3(np.ones((3, 3))).any()  # singular: cv::invert leaves zeros


def test_degenerate_inputs(R, O):
    pr = HR.two_view(60, 57, planar=False, noise=0.3)
    a, b, K = pr["src"], pr["dst"], pr["K"]
    for m in (0, 4):
        assert not R.esti_motion_by_essential(O, a[:m], b[:m], K)["found"]
    p5 = HR.two_view(5, several_candidate_seed(O), planar=False, noise=0.0)
    assert not R.esti_motion_by_essential(O, p5["src"], p5["dst"], p5["K"])["found"]
    # rotation only: the fitted E is dominated by noise; recoverPose still returns a rotation and a unit t
    pr = HR.two_view(400, 58, planar=False, noise=0.5, rotation_only=True)
    ref = R.esti_motion_by_essential(O, pr["src"], pr["dst"], pr["K"])
    assert ref["found"]
    assert np.abs(ref["R"] @ ref["R"].T - np.eye(3)).max() < 1e-9 and abs(np.linalg.det(ref["R"]) - 1) < 1e-9
    assert abs(np.linalg.norm(ref["t"]) - 1) < 1e-12
    # NULL models and empty lists
    g = R.esti_motion_by_essential(O, a, b, K)
    out = R.check_init_scores(a, b, K, None, g["inliers"], None, g["inliers"])
    assert out == dict(score_e=0.0, score_h=0.0, kept_e=out["kept_e"], kept_h=out["kept_h"])
    assert len(out["kept_e"]) == 0 and len(out["kept_h"]) == 0
    assert R.check_init_scores(a, b, K, g["E"], [], None, None)["score_e"] == 0.0
    # a match on the epipole of the first image: 0 / 0 in the reference's expression, NaN propagates into the sum
    p1, p2 = epipole_case(g["E"], K)
    se, _, _, _ = numpy_scores(p1, p2, K, g["E"], [0], None, None)
    got = R.check_init_scores(p1, p2, K, g["E"], [0, 1], None, None)
    assert np.isnan(got["score_e"]) == np.isnan(se)
