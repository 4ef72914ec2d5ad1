"""Known answers for the test-side restatement of cv::findHomography (tests/homography_restatement.cpp), the CPU
reference the device homography RANSAC of the monocular initialisation is compared with bit for bit."""
import numpy as np
import pytest

import h_restate as HR


@pytest.fixture(scope="module")
def R():
    return HR.Restatement()


def _apply(H, p):
    q = np.c_[p.astype(float), np.ones(len(p))] @ H.T
    return q[:, :2] / q[:, 2:]


def test_exact_homography_from_exact_correspondences(R):
    """A homography whose images of small-integer pixels are exact in float32: every match is an inlier and the
    refined H equals the true one to 1e-9."""
    Ht = np.array([[1.25, 0.125, 16.0], [-0.0625, 0.75, -8.0], [0.0, 0.0, 1.0]])
    g = np.stack(np.meshgrid(np.arange(8, 600, 37.0), np.arange(8, 460, 29.0)), -1).reshape(-1, 2)
    src = g.astype(np.float32)
    dst = _apply(Ht, g).astype(np.float32)
    assert np.array_equal(dst.astype(float), _apply(Ht, g))
    r = R.find_homography(src, dst)
    assert r["H"] is not None and len(r["inliers"]) == len(g)
    H = r["H"] / r["H"][2, 2]
    assert np.abs(H - Ht).max() < 1e-9


@pytest.mark.parametrize("seed", [1, 2])
def test_plane_induced_homography(R, seed):
    """Noise-free plane correspondences (rounded to float32 pixels): H = K (R + t n^T / d) K^-1 up to the rounding."""
    pr = HR.two_view(300, seed, planar=True, noise=0.0)
    r = R.find_homography(pr["src"], pr["dst"])
    H = r["H"] / r["H"][2, 2]
    rel = np.abs(H - pr["H_true"]) / np.maximum(np.abs(pr["H_true"]), 1e-3)
    assert rel.max() < 1e-5, rel
    assert len(r["inliers"]) == 300 and r["lm_iters"] >= 1 and r["dlt"] == 1


@pytest.mark.parametrize("frac", [0.0, 0.3, 0.6])
def test_ransac_recovers_the_inlier_set(R, frac):
    """No wrong match is kept (they sit >= 25 px from the truth); the RANSAC mask comes from a 4-point model of noisy
    matches, so a few true matches may fall outside 3 px."""
    pr = HR.two_view(500, 7, planar=True, outlier_frac=frac, noise=0.3)
    r = R.find_homography(pr["src"], pr["dst"])
    gt = pr["inlier_gt"]
    assert gt[r["inliers"]].all() and len(r["inliers"]) >= 0.97 * gt.sum()
    assert r["iters_run"] < 2000
    # the refinement does not increase the squared reprojection error of the inliers
    i = r["inliers"]
    H = r["H"]
    Hr = R.run_kernel4(pr["src"], pr["dst"], i[:4])
    e = np.sum((_apply(H, pr["src"][i]) - pr["dst"][i]) ** 2)
    e4 = np.sum((_apply(Hr, pr["src"][i]) - pr["dst"][i]) ** 2)
    assert e <= e4 and e < 2 * 0.09 * len(i) * 1.5


def test_small_and_degenerate_inputs(R):
    pr = HR.two_view(40, 3, planar=True, noise=0.0)
    s, d = pr["src"], pr["dst"]
    for k in (0, 1, 3):
        r = R.find_homography(s[:k], d[:k])
        assert r["H"] is None and len(r["inliers"]) == 0
    # n == 4: runKernel on the four matches, no RANSAC, every match an inlier, no refinement
    r = R.find_homography(s[:4], d[:4])
    assert np.array_equal(r["inliers"], np.arange(4)) and r["lm_iters"] == 0 and r["iters_run"] == 1
    assert np.abs(_apply(r["H"], s[:4]) - d[:4]).max() < 1e-3
    # all points on one line: no subset passes checkSubset -> findHomography fails at the first iteration
    x = np.arange(10, 250, 8.0)
    line = np.c_[x, 2 * x + 7].astype(np.float32)
    r = R.find_homography(line, line + 3)
    assert r["H"] is None and r["n_subsets"] == 0
    # four identical points: degenerate scales, runKernel returns no model
    same = np.tile(np.float32([[5, 5]]), (4, 1))
    assert R.find_homography(same, same)["H"] is None


def _collinear_np(p):
    i = 3
    for j in range(i):
        dx1 = float(np.float32(p[j, 0]) - np.float32(p[i, 0]))
        dy1 = float(np.float32(p[j, 1]) - np.float32(p[i, 1]))
        for k in range(j):
            dx2 = float(np.float32(p[k, 0]) - np.float32(p[i, 0]))
            dy2 = float(np.float32(p[k, 1]) - np.float32(p[i, 1]))
            if abs(dx2 * dy1 - dy2 * dx1) <= np.finfo(np.float32).eps * (abs(dx1) + abs(dy1) + abs(dx2) + abs(dy2)):
                return True
    return False


def _det(a, b, c):
    m = np.array([[a[0], a[1], 1.0], [b[0], b[1], 1.0], [c[0], c[1], 1.0]], float)
    return (m[0, 0] * (m[1, 1] * m[2, 2] - m[2, 1] * m[1, 2]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[2, 0] * m[1, 2])
            + m[0, 2] * (m[1, 0] * m[2, 1] - m[2, 0] * m[1, 1]))


def test_check_subset_matches_a_transcription(R):
    """HomographyEstimatorCallback::checkSubset: collinear triples with the last point in either image, then the four
    triangle orientations agree in all or in none."""
    rng = np.random.RandomState(5)
    seen = {True: 0, False: 0}
    for trial in range(3000):
        src = rng.randint(0, 12, (4, 2)).astype(np.float32)
        dst = src + rng.randint(-3, 4, (4, 2)).astype(np.float32) if trial % 2 else rng.randint(0, 12, (4, 2)).astype(np.float32)
        ok = not (_collinear_np(src) or _collinear_np(dst))
        if ok:
            tt = [(0, 1, 2), (1, 2, 3), (0, 2, 3), (0, 1, 3)]
            neg = sum(_det(*src[list(t)]) * _det(*dst[list(t)]) < 0 for t in tt)
            ok = neg in (0, 4)
        assert R.check_subset(src, dst, np.arange(4)) == ok, (src, dst)
        seen[ok] += 1
    assert seen[True] > 300 and seen[False] > 300


def test_subsets_follow_cv_rng_and_the_retry_rule(R):
    pr = HR.two_view(60, 4, planar=True)
    sub = R.subsets(pr["src"], pr["dst"], 200)
    assert len(sub) == 200
    for s in sub:
        assert len(set(s.tolist())) == 4 and R.check_subset(pr["src"], pr["dst"], s)
    # the first draws are cv::RNG((uint64)-1).uniform(0, 60) as long as the subsets pass
    state = (1 << 64) - 1
    first = []
    for _ in range(4):
        state = ((state & 0xffffffff) * 4164903690 + (state >> 32)) & ((1 << 64) - 1)
        first.append((state & 0xffffffff) % 60)
    if len(set(first)) == 4 and R.check_subset(pr["src"], pr["dst"], np.array(first)):
        assert sub[0].tolist() == first


def test_general_scene_inliers_are_a_minority_subset_for_h(R):
    """A thick scene under translation is not a homography: the H inliers are a strict subset of the matches."""
    pr = HR.two_view(400, 9, planar=False, noise=0.3)
    r = R.find_homography(pr["src"], pr["dst"])
    assert r["H"] is not None and len(r["inliers"]) < 0.9 * 400
    rot_only = HR.two_view(400, 9, planar=False, noise=0.3, rotation_only=True)
    r2 = R.find_homography(rot_only["src"], rot_only["dst"])
    assert len(r2["inliers"]) > 0.93 * 400   # pure rotation: every match obeys the infinite homography
