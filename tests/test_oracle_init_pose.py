"""Known answers for the restatement of the homography branch and the E / H choice of the monocular initialisation
(tests/init_pose_restatement.cpp via tests/pose_restate.py), on the CPU: the Malis-Vargas identity Hn = +-(R + t n^T)
for every candidate, the true motion and plane from a known plane homography, the rotation-only branch, the
visibility filter against numpy dot products, the decomposition against an independent float64 numpy transcription,
the choice rule on hand-made tables and invRt against the oracle's 4 x 4 inverse.

OpenCV computes v = 2 sqrtf(...) with a FLOAT square root, which perturbs v by up to ~1e-7
relative and the candidates by up to ~1e-7 absolute.  The 1e-9 identities are therefore asserted on the numpy
transcription with a double square root (the algorithm itself), and the restatement is held to that transcription
with OpenCV's float square root to 1e-12 relative, and to the identities within the float bound 1e-6."""
import numpy as np
import pytest

import h_restate as HR
import init_restate as IR
import pose_restate as PR


@pytest.fixture(scope="module")
def P(mvo):
    """The restatement of the product's entry points, which the library must export (dlsym, no GPU needed)."""
    lib = mvo.load_library()
    for sym in ("mvo_esti_motion_by_homography", "mvo_debug_get_homography_decomposition",
                "mvo_estimate_possible_relative_poses"):
        assert getattr(lib, sym) is not None
    assert all(hasattr(mvo.Context, m) for m in ("esti_motion_by_homography", "debug_homography_decomposition",
                                                   "estimate_possible_relative_poses"))
    return PR.Restatement()


def minor(S, r, c):
    x1, x2 = (1 if c == 0 else 0), (1 if c == 2 else 2)
    y1, y2 = (1 if r == 0 else 0), (1 if r == 2 else 2)
    return S[y1, x2] * S[y2, x1] - S[y1, x1] * S[y2, x2]


def numpy_decompose(Hs, K, float_sqrt=True):
    """HomographyDecompInria transcribed with numpy (LAPACK SVD and inverse): (count, index, Hn, w, [(R, t, n)])."""
    Hn = np.linalg.inv(K) @ Hs @ K
    w = np.linalg.svd(Hn, compute_uv=False)
    Hn = Hn / w[1]
    S = Hn.T @ Hn - np.eye(3)
    if np.abs(S).max() < 0.001:
        return 1, -1, Hn, w, [(Hn, np.zeros(3), np.zeros(3))]
    sg = lambda x: 1.0 if x >= 0 else -1.0  # noqa: E731
    M00, M11, M22 = minor(S, 0, 0), minor(S, 1, 1), minor(S, 2, 2)
    r00, r11, r22 = np.sqrt(M00), np.sqrt(M11), np.sqrt(M22)
    e01, e02, e12 = sg(minor(S, 0, 1)), sg(minor(S, 0, 2)), sg(minor(S, 1, 2))
    d = np.abs(np.diag(S))
    i = (2 if d[1] < d[2] else 1) if d[0] < d[1] else (2 if d[0] < d[2] else 0)
    if i == 0:
        npa = np.array([S[0, 0], S[0, 1] + r22, S[0, 2] + e12 * r11])
        npb = np.array([S[0, 0], S[0, 1] - r22, S[0, 2] - e12 * r11])
    elif i == 1:
        npa = np.array([S[0, 1] + r22, S[1, 1], S[1, 2] - e02 * r00])
        npb = np.array([S[0, 1] - r22, S[1, 1], S[1, 2] + e02 * r00])
    else:
        npa = np.array([S[0, 2] + e01 * r11, S[1, 2] + r00, S[2, 2]])
        npb = np.array([S[0, 2] - e01 * r11, S[1, 2] - r00, S[2, 2]])
    tr = np.trace(S)
    arg = 1 + tr - M00 - M11 - M22
    v = 2.0 * (float(np.sqrt(np.float32(arg))) if float_sqrt else np.sqrt(arg))
    r, n_t = np.sqrt(2 + tr + v), np.sqrt(2 + tr - v)
    na, nb = npa / np.linalg.norm(npa), npb / np.linalg.norm(npb)
    ta = 0.5 * n_t * (sg(S[i, i]) * r * nb - n_t * na)
    tb = 0.5 * n_t * (sg(S[i, i]) * r * na - n_t * nb)
    out = []
    for ts, n in ((ta, na), (tb, nb)):
        R = Hn @ (np.eye(3) - (2 / v) * np.outer(ts, n))
        if np.linalg.det(R) < 0:
            R = -R
        t = R @ ts
        out += [(R, t, n), (R, -t, -n)]
    return 4, i, Hn, w, out


def homographies():
    """Plane homographies away from the branch thresholds: the planar scenes of the device tests and variations."""
    for seed in range(6):
        pr = HR.two_view(10, 50 + seed, planar=True, noise=0.0)
        rng = np.random.RandomState(seed)
        R = HR.rot(rng.normal(size=3), rng.uniform(3, 25))
        t = rng.normal(size=3) * rng.uniform(0.05, 1.0)
        n = rng.normal(size=3)
        n[2] = abs(n[2]) + 0.5
        n /= np.linalg.norm(n)
        K = pr["K"]
        Ht = K @ (R + np.outer(t, n) / 3.0) @ np.linalg.inv(K)
        yield Ht / Ht[2, 2], K, R, t, n


def test_every_candidate_satisfies_the_homography_identity(P):
    for Hs, K, _, _, _ in homographies():
        cnt, _, Hn, _, cands = numpy_decompose(Hs, K, float_sqrt=False)
        assert cnt == 4
        for R, t, n in cands:
            M = R + np.outer(t, n)
            assert min(np.abs(M - Hn).max(), np.abs(M + Hn).max()) < 1e-9
            assert np.abs(R.T @ R - np.eye(3)).max() < 1e-9 and abs(np.linalg.det(R) - 1) < 1e-9
            assert abs(np.linalg.norm(n) - 1) < 1e-12
        d = P.decompose(Hs, K)
        assert d["count"] == 4 and not d["rotation_only"]
        for c in range(4):
            R, t, n = d["Rs"][c], d["ts"][c], d["normals"][c]
            M = R + np.outer(t, n)
            assert min(np.abs(M - d["Hn"]).max(), np.abs(M + d["Hn"]).max()) < 1e-6  # float sqrt of v
            assert np.abs(R.T @ R - np.eye(3)).max() < 1e-6 and np.linalg.det(R) > 0
            assert abs(np.linalg.norm(n) - 1) < 1e-12


def test_known_plane_gives_the_true_motion(P):
    for seed in (61, 62, 63):
        pr = HR.two_view(300, seed, planar=True, noise=0.0)
        tu = pr["t"] / np.linalg.norm(pr["t"])
        # the algorithm (double sqrt): one candidate is the truth to 1e-9
        _, _, _, _, cands = numpy_decompose(pr["H_true"] * 1.7, pr["K"], float_sqrt=False)
        assert any(np.abs(R - pr["R"]).max() < 1e-9 and np.abs(t / np.linalg.norm(t) - tu).max() < 1e-9 and
                   np.abs(n - pr["n"]).max() < 1e-9 for R, t, n in cands)
        # the restatement: the filter keeps exactly that candidate
        h = P.decompose(pr["H_true"] * 1.7, pr["K"])
        rej = P.filter(pr["src"], pr["dst"], np.arange(300), pr["K"], h)
        surv = [c for c in range(4) if rej[c] == 0]
        assert len(surv) == 1
        c = surv[0]
        assert np.abs(h["Rs"][c] - pr["R"]).max() < 1e-6
        assert np.abs(P.normalise_t(h["ts"][c]) - tu).max() < 1e-6
        assert np.abs(h["normals"][c] - pr["n"]).max() < 1e-9


def test_rotation_only_gives_one_candidate_that_the_filter_removes(P):
    pr = HR.two_view(100, 64, planar=False, rotation_only=True, noise=0.0)
    d = P.decompose(pr["H_true"], pr["K"])
    assert d["count"] == 1 and d["rotation_only"] and d["index"] == -1
    assert np.abs(d["Hn"] - pr["R"]).max() < 1e-9 and not d["normals"].any() and not d["ts"].any()
    assert np.isnan(P.normalise_t(d["ts"][0])).all()  # 0 * inf, unguarded as in the reference
    rej = P.filter(pr["src"], pr["dst"], np.arange(100), pr["K"], d)
    assert rej[0] == 100


def test_filter_matches_numpy_dot_products(P):
    for seed, frac in ((65, 0.0), (66, 0.4), (67, 0.2)):
        pr = HR.two_view(400, seed, planar=True, noise=0.5, outlier_frac=frac)
        h = P.esti_motion_by_homography(pr["src"], pr["dst"], pr["K"])
        K, inl, d = pr["K"], h["inliers"], h["dec"]
        p1 = ((pr["src"][inl] - K[:2, 2]) / np.diag(K)[:2]).astype(np.float32).astype(np.float64)
        p2 = ((pr["dst"][inl] - K[:2, 2]) / np.diag(K)[:2]).astype(np.float32).astype(np.float64)
        p1, p2 = np.c_[p1, np.ones(len(inl))], np.c_[p2, np.ones(len(inl))]
        for c in range(4):
            R, n = d["Rs"][c], d["normals"][c]
            bad = ((p1 @ n) <= 0) | ((p2 @ (R @ n)) <= 0)
            assert h["rejected"][c] == bad.sum()
        assert h["survivors"] == [c for c in range(4) if h["rejected"][c] == 0]


def test_decomposition_matches_a_numpy_transcription(P):
    for Hs, K, _, _, _ in homographies():
        cnt, idx, Hn, w, cands = numpy_decompose(Hs, K, float_sqrt=True)
        d = P.decompose(Hs, K)
        assert d["count"] == cnt and d["index"] == idx
        assert np.abs(d["w"] - w).max() <= 1e-12 * w.max()
        assert np.abs(d["Hn"] - Hn).max() <= 1e-12 * np.abs(Hn).max()
        for c, (R, t, n) in enumerate(cands):
            assert np.abs(d["Rs"][c] - R).max() <= 1e-12
            assert np.abs(d["ts"][c] - t).max() <= 1e-12 * max(1.0, np.abs(t).max())
            assert np.abs(d["normals"][c] - n).max() <= 1e-12


def test_choice_rule_on_hand_made_tables(P):
    assert P.choose(1.0, 1.0, True, [0.9, 0.95]) == (0, 0.5)  # exactly 0.5: E
    best, ratio = P.choose(1.0, 3.0, True, [0.9, 0.95, 0.95, 0.2])
    assert best == 2 and ratio == 0.75  # strictly larger |n_z| wins, the first of a tie stays
    assert P.choose(1.0, 3.0, True, [0.7, 0.7])[0] == 1
    best, ratio = P.choose(float("nan"), 3.0, True, [0.9])
    assert best == 0 and np.isnan(ratio)  # NaN ratio chooses E
    assert P.choose(0.0, 0.0, True, [])[0] == 0  # 0 / 0: NaN, E
    # best = -1: E absent with ratio <= 0.5 or NaN; ratio > 0.5 with no H survivor
    assert P.choose(0.0, 0.0, False, [])[0] == -1
    assert P.choose(2.0, 1.0, False, [0.5])[0] == -1
    assert P.choose(0.0, 5.0, True, [])[0] == -1


def test_inv_rt_matches_the_oracle_inverse(P, O):
    rng = np.random.RandomState(68)
    for _ in range(5):
        R = HR.rot(rng.normal(size=3), rng.uniform(1, 90))
        t = rng.normal(size=3)
        Ri, ti = P.inv_rt(R, t)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, t
        Ti = O.invert4x4(T)
        assert np.array_equal(Ri, Ti[:3, :3]) and np.array_equal(ti, Ti[:3, 3])
        assert np.abs(Ri - R.T).max() < 1e-12


def test_composed_restatement_table(P, O):
    pr = HR.two_view(400, 69, planar=True, noise=0.5, outlier_frac=0.2)
    ref = P.estimate_possible_relative_poses(O, pr["src"], pr["dst"], pr["K"])
    sols = ref["solutions"]
    assert sols[0]["kind"] == "E" and all(s["kind"] == "H" for s in sols[1:]) and len(sols) >= 2
    assert [s["candidate"] for s in sols[1:]] == ref["h"]["survivors"]
    for s in sols:
        assert len(s["pts3d"]) == len(s["inliers"])
    nz = [abs(s["normal"][2]) for s in sols[1:]]
    assert ref["ratio"] == ref["score_h"] / (ref["score_e"] + ref["score_h"])
    assert ref["best"] == (1 + int(np.argmax(nz)) if ref["ratio"] > 0.5 else 0)
    inv = P.estimate_possible_relative_poses(O, pr["src"], pr["dst"], pr["K"], motion_cam2_to_cam1=False)
    for a, b in zip(sols, inv["solutions"]):
        Ri, ti = P.inv_rt(a["R"], a["t"])
        assert np.array_equal(Ri, b["R"]) and np.array_equal(ti, b["t"]) and np.array_equal(a["pts3d"], b["pts3d"])
    kd = IR.kdict(pr["K"])
    s0 = sols[0]
    assert np.array_equal(s0["pts3d"], O.triangulate_points(pr["src"][s0["inliers"]], pr["dst"][s0["inliers"]], kd,
                                                            s0["R"], s0["t"])[0])
