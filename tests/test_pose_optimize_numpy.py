"""Known answers of tests/pose_optimize_numpy.py, the numpy transcription of the robust motion-only pose optimisation (DESIGN.md
section 21).  None of them rests on the transcription agreeing with itself: a scene whose minimiser is known, flags that must be
exactly the moved observations, the statuses by construction, the 6 x 6 solve against LAPACK with a bound from the backward error
of a Cholesky solve, the orthogonality of the reported rotations, and the declared summation order against a plain Python
restatement.  tests/test_pose_optimize_sim.py and tests/test_gpu_pose_optimize.py hold the emulated build and the MI355X to this
transcription bit for bit."""
import numpy as np

import pose_optimize_numpy as R

K = {k: float(np.float32(v)) for k, v in R.FR1_K.items()}
EPS = float(np.finfo(np.float64).eps)
U = EPS / 2         # unit roundoff


def pose_error(T, truth):
    """(translation distance, rotation angle in radians) between two camera-to-world poses."""
    dR = T[:3, :3].T @ truth[:3, :3]
    return float(np.linalg.norm(T[:3, 3] - truth[:3, 3])), float(np.arccos(min(1.0, (np.trace(dR) - 1) / 2)))


def chi2_at(p3, p2, s, T_w_c, take):
    """The declared chi2 (no kernel) of the observations `take` at a pose."""
    Tcw = np.linalg.inv(T_w_c)
    R0, t0 = [[float(v) for v in row[:3]] for row in Tcw[:3]], [float(v) for v in Tcw[:3, 3]]
    sums, front = R.evaluate(R0, t0, p3, p2, np.ones(len(p3)) if s is None else s, K, take, 1.0, False)
    assert front
    return sums[27]


def test_exact_pixels_end_below_the_chi2_of_the_true_pose():
    """(a) The observations are the f32 roundings of exact projections: the true pose is not the minimiser of the rounded data,
    the minimiser lies below it by about 6 / 2n of chi2 (six fitted unknowns of 2n residuals).  Status 0, no outlier, and a
    final chi2 strictly below the chi2 at the true pose."""
    n = 200
    p3, p2, T, _, _ = R.scene(np.random.RandomState(11), n)
    T_init = R.perturbed(T, 2.0, (0.1, -0.1, 0.15))        # 2 degrees; 0.2 of a depth of 2 .. 6: about 5 %
    Twc, Tcw, outlier, chi2, info, rows = R.optimize_pose(p3, p2, None, T_init, K)
    at_truth = chi2_at(p3, p2, None, T, np.ones(n, bool))
    assert info[0] == R.OPTIMISED and not outlier.any() and info[4] == n == info[5]
    assert 0 < at_truth < n * 2 * (2.0 ** -14) ** 2          # (pixels below 1024 round to within 2^-15)
    assert chi2[1] < at_truth, "final chi2 %.6g is not below the %.6g of the true pose" % (chi2[1], at_truth)
    assert chi2[0] > 100 * n                                  # (the start was far away: the Huber sum of errors of tens of pixels)
    dt, dr = pose_error(Twc, T)
    assert dt < 1e-6 and dr < 1e-6
    assert np.array_equal(Tcw[3], [0, 0, 0, 1]) and np.abs(Tcw @ Twc - np.eye(4)).max() < 1e-14


def test_exactly_the_moved_observations_are_flagged():
    """(b) 0.5 px noise, every fifth observation moved by (40, -30) px."""
    n = 300
    p3, p2, T, moved, _ = R.scene(np.random.RandomState(12), n, 0.5, 5)
    T_init = R.perturbed(T, 2.0, (0.1, -0.1, 0.15))
    Twc, _, outlier, chi2, info, rows = R.optimize_pose(p3, p2, None, T_init, K)
    assert info[0] == R.OPTIMISED and info[1] == 4
    assert np.array_equal(np.nonzero(outlier)[0], moved) and info[4] == n - len(moved)
    # the final round ran without the kernel: its chi2 is the plain sum of c over the inliers it started with, which were the
    # not-moved observations already (rows[2, 5] inliers came out of round 2)
    assert rows[3, 0] == n - len(moved)
    assert abs(chi2[1] - chi2_at(p3, p2, None, Twc, ~outlier.astype(bool))) <= 1e-9 * chi2[1]
    assert chi2[1] < 2 * (n - len(moved)) * 0.5 ** 2 * 1.5    # 2 residuals of variance 0.25 per inlier (and half as much again)
    one = R.optimize_pose(p3, p2, None, T_init, K, dict(rounds=1))
    e4, e1 = pose_error(Twc, T), pose_error(one[0], T)
    assert e4[0] < e1[0] and e4[1] < e1[1], "four rounds %r are not better than one %r" % (e4, e1)


def test_status_1_and_status_2():
    """(c)"""
    p3, p2, T, moved, _ = R.scene(np.random.RandomState(13), 18, 0.5, 2)
    T_init = R.perturbed(T, 1.0, (0.05, -0.05, 0.05))
    Twc, Tcw, outlier, chi2, info, rows = R.optimize_pose(p3, p2, None, T_init, K)
    assert info[0] == R.FEW_INLIERS and info[4] < 10 and info[1] == len(rows) >= 1 and info[5] == 18
    assert outlier.sum() == 18 - info[4] and rows[-1, 5] == info[4]
    assert Twc.tobytes() != T_init.tobytes()                  # the pose of that round is still reported
    p3, p2, T, _, behind = R.scene(np.random.RandomState(14), 40, 0.5, 0, 31)
    T_init = R.perturbed(T, 0.5, (0.01, 0.0, 0.0))
    Twc, Tcw, outlier, chi2, info, rows = R.optimize_pose(p3, p2, None, T_init, K)
    assert info.tolist() == [R.FEW_IN_FRONT, 0, 0, 0, 0, 9] and outlier.all() and not chi2.any() and len(rows) == 0
    assert Twc.tobytes() == T_init.tobytes()                  # bit for bit as given
    nine = R.optimize_pose(p3, p2, None, T_init, K, dict(min_inliers=9))
    assert nine[4][0] != R.FEW_IN_FRONT and nine[4][5] == 9 and nine[2][behind].all()


def test_status_3_at_a_stationary_start():
    """(d) The construction of pose_optimize_numpy.stationary_scene: every e is exactly 0.0 in f64 (integer-valued pixels,
    dyadic ratios, identity pose), so b = 0, the solve returns zeros, the Rodrigues matrix of a zero vector is I and the trial
    state is the state: chi2' < chi2 is 0 < 0."""
    p3, p2, T, Kd = R.stationary_scene()
    assert len(np.unique(p3, axis=0)) > 20 and (p2 == np.round(p2)).all()
    q, ax, ay, ex, ey, c = R.project([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]], [0.0, 0.0, 0.0], p3, p2, np.ones(len(p3)), Kd)
    assert not ex.any() and not ey.any()
    traces = []
    Twc, Tcw, outlier, chi2, info, rows = R.optimize_pose(p3, p2, None, T, Kd, None, traces)
    assert info.tolist() == [R.NO_STEP, 4, 40, 0, len(p3), len(p3)] and not outlier.any() and not chi2.any()
    assert Twc.tobytes() == np.eye(4).tobytes() and Tcw.tobytes() == np.eye(4).tobytes()
    assert not any(any(t) for t in traces)


def test_the_6x6_solve_against_lapack():
    """(e) Cholesky of order n = 6 followed by the two triangular solves computes the exact solution of (A + dA) x = b with
    |dA|_2 <= 4 n (3 n + 1) u |A|_2 = 456 u |A|_2 (Higham, Accuracy and Stability of Numerical Algorithms, theorem 10.4 with
    (10.7); u = 2^-53), valid while 456 u kappa < 1/2.  Hence the residual |b - A x|_2 <= 456 u |A|_2 |x|_2, to which evaluating
    the residual in f64 adds at most gamma_7 (|A| |x| + |b|) <= 8 u (|A|_2 |x|_2 sqrt(6) + |b|_2); and |x - x*|_2 <= kappa 456 u /
    (1 - kappa 456 u) |x*|_2.  LAPACK's own solution x~ carries an error of the same form (backward stable, in practice a
    backward error of a few u): it gets the same share, so |x - x~|_2 <= 2 * 456 u kappa / (1 - 456 u kappa) |x~|_2."""
    rng = np.random.RandomState(15)
    n, c = 6, 4 * 6 * (3 * 6 + 1)
    for case in range(40):
        G = rng.standard_normal((12, 6)) * 10.0 ** rng.uniform(-2, 2, 6)        # columns of different scales, like (omega, upsilon)
        H = G.T @ G
        H = (H + H.T) / 2
        b = rng.standard_normal(6) * 10.0 ** rng.uniform(-3, 3)
        lam = 1e-3 * H.diagonal().max() * 10.0 ** rng.randint(-2, 3)
        sums = [H[r, k] for r, k in R.UPPER] + list(b) + [0.0]
        x = np.array(R.solve6(sums, lam))
        A = H + lam * np.eye(6)
        kappa = np.linalg.cond(A)
        assert c * U * kappa < 0.5
        normA = np.linalg.norm(A, 2)
        res = np.linalg.norm(-b - A @ x)
        assert res <= c * U * normA * np.linalg.norm(x) + 8 * U * (np.sqrt(6) * normA * np.linalg.norm(x) + np.linalg.norm(b)), case
        ref = np.linalg.solve(A, -b)
        assert np.linalg.norm(x - ref) <= 2 * c * U * kappa / (1 - c * U * kappa) * np.linalg.norm(ref), case
    # a pivot that is not positive and finite makes the trial fail
    assert R.solve6([0.0] * 28, 0.0) is None and R.solve6([0.0] * 28, float("inf")) is None
    bad = [-1.0 if (r, k) == (3, 3) else (1.0 if r == k else 0.0) for r, k in R.UPPER] + [1.0] * 6 + [0.0]
    assert R.solve6(bad, 0.5) is None and R.solve6(bad, 1.5) is not None


def test_reported_rotations_are_orthogonal():
    """(f) |R^T R - I|_max <= 1e-12 of every reported pose.  A reported rotation is the initial one (the LU inverse of an
    orthogonal matrix given to a few eps) times at most `iterations` Rodrigues matrices, since every round starts again from
    the initial pose; the whole call makes at most rounds x iterations = 40 such products with the defaults, and the bound is
    taken for all 40 in one chain.  rodrigues_fwd is within 16 eps of a rotation (its bound in tests/wave_linalg_cases.py); a
    3 x 3 product of entries below 1 adds 3 roundings of at most eps / 2 per entry; R^T R - I is first order twice the
    departure.  So one factor adds at most 2 (16 + 1.5) eps = 35 eps to |R^T R - I|_max, 40 factors 1400 eps = 3.1e-13, and
    the start a few eps more: below 1e-12."""
    assert 40 * 2 * (16 + 1.5) * EPS + 100 * EPS < 1e-12
    for seed, n, params in ((16, 300, None), (17, 64, dict(rel_tolerance=0.0)), (18, 1000, dict(rounds=8, rel_tolerance=0.0, iterations=64))):
        p3, p2, T, _, _ = R.scene(np.random.RandomState(seed), n, 0.5, 5, 3)
        T_init = R.perturbed(T, 2.0, (0.1, -0.1, 0.15))
        Twc, Tcw, _, _, info, _ = R.optimize_pose(p3, p2, None, T_init, K, params)
        assert info[0] == R.OPTIMISED and info[3] >= 10
        for M in (Twc, Tcw):
            assert np.abs(M[:3, :3].T @ M[:3, :3] - np.eye(3)).max() <= 1e-12


def plain_tree(terms):
    """The declared order in plain Python floats."""
    S = [0.0] * 256
    for k, v in enumerate(terms):
        S[k % 256] = S[k % 256] + float(v)
    while len(S) > 1:
        S = [S[i] + S[i + 1] for i in range(0, len(S), 2)]
    return S[0]


def test_the_summation_order():
    """(g)"""
    rng = np.random.RandomState(19)
    t = rng.standard_normal(600) * 10.0 ** rng.uniform(-3, 3, 600)
    all_ = np.ones(600, bool)
    for n in (1, 2, 255, 256, 257, 511, 512, 513, 600):
        assert R.tree_sum(t[:n], all_[:n]) == plain_tree(t[:n])
        assert R.tree_sum(t[:n], all_[:n]) == R.tree_sum(t[:n].copy(), all_[:n])      # permuting nothing changes nothing
    # an observation that does not take part contributes 0.0 to its slot
    take = rng.rand(600) < 0.7
    assert R.tree_sum(t, take) == plain_tree(np.where(take, t, 0.0))
    # permuting observations within a stride moves them to other slots: other pairs, other bits
    perm = np.r_[rng.permutation(256), np.arange(256, 600)]
    assert R.tree_sum(t[perm], all_) != R.tree_sum(t, all_)
    assert abs(R.tree_sum(t[perm], all_) - R.tree_sum(t, all_)) <= 600 * EPS * np.abs(t).sum()
    # three observations of one slot in another order: ((0 + 1) + 1e16) - 1e16 = 0 against ((0 - 1e16) + 1e16) + 1 = 1
    z = np.zeros(600)
    z[[7, 263, 519]] = (1.0, 1e16, -1e16)
    swap = np.arange(600)
    swap[[7, 519]] = [519, 7]
    assert R.tree_sum(z, all_) == 0.0 and R.tree_sum(z[swap], all_) == 1.0
    # n = 257 is n = 256 with slot 0 = (0.0 + t_0) + t_256 and every other slot as it was
    S = [float(v) for v in t[:256]]
    S[0] = (0.0 + S[0]) + float(t[256])
    while len(S) > 1:
        S = [S[i] + S[i + 1] for i in range(0, len(S), 2)]
    assert R.tree_sum(t[:257], all_[:257]) == S[0]
    assert R.tree_sum(t[:257], all_[:257]) != R.tree_sum(t[:256], all_[:256]) + t[256]
    # ... and the optimiser's result depends on the order the same way: the same observations, permuted inside a stride
    p3, p2, T, _, _ = R.scene(np.random.RandomState(20), 300, 0.5, 5)
    T_init = R.perturbed(T, 2.0, (0.1, -0.1, 0.15))
    a = R.optimize_pose(p3, p2, None, T_init, K)
    b = R.optimize_pose(p3.copy(), p2.copy(), None, T_init, K)
    p = np.r_[np.arange(255, -1, -1), np.arange(256, 300)]
    c = R.optimize_pose(p3[p], p2[p], None, T_init, K)
    assert a[0].tobytes() == b[0].tobytes() and a[3].tobytes() == b[3].tobytes()
    assert a[3].tobytes() != c[3].tobytes() and np.array_equal(a[2][p], c[2]) and np.abs(a[0] - c[0]).max() < 1e-9
