"""Known answers of the numpy transcription of the map-point position refinement (tests/map_refine_numpy.py): what the MI355X
kernel and the emulated build are then compared with bit for bit (tests/test_gpu_map_refine.py, tests/test_map_refine_sim.py).
The scene is the one of DESIGN.md section 18: 20 cameras 0.03 apart, each with 0.01 rad more yaw than the last, depths 0.5 .. 1.5,
the TUM fr1 intrinsics, 2 .. 20 observations per point, start positions 3 % off."""
import functools

import numpy as np

import map_refine_numpy as R

# Measured with this transcription on the exact-pixel scene below (pixels exact up to their f32 rounding): the worst of the 300
# points ends 7.07e-7 x depth from the truth (median 3.2e-8).  The bound is ten times that: the factor covers another seed
# and the f32 store of the result.
MEASURED_WORST, BOUND = 7.07e-7, 7.07e-6
# intrinsics and poses whose projections are exact in f64 AND in f32: powers of two and small dyadic numbers
K2 = dict(fx=512.0, fy=512.0, cx=320.0, cy=240.0)


@functools.lru_cache(maxsize=None)
def run(noise, moved_every, lo, delta=None):
    rng = np.random.RandomState(1)
    counts = rng.randint(lo, 21, 300)
    s = R.scene(rng, counts, 20, noise, moved_every)
    out = R.refine(s[1], s[2], R.FR1_K, s[3], s[4], s[5], None if delta is None else dict(huber_delta=delta))
    return s, out


def rel_err(pos, truth):
    return np.linalg.norm(np.asarray(pos, np.float64) - truth, axis=1) / truth[:, 2]


def translation(x, y, z):
    T = np.eye(4)
    T[:3, 3] = (x, y, z)
    return T


def test_exact_pixels_end_at_the_truth():
    (truth, pos, T, frame, uv, start, _), (out, chi2, info, flags) = run(0.0, 0, 2)
    assert (info[:, 0] == R.REFINED).all() and not flags.any()
    assert info[:, 1].min() >= 2 and info[:, 1].max() <= 8 and info[:, 2].max() <= 20
    err = rel_err(out, truth)
    print("exact pixels: worst %.3g x depth, median %.3g; at most %d accepted steps" % (err.max(), np.median(err), info[:, 1].max()))
    assert err.max() < BOUND and rel_err(pos, truth).min() > 0.02
    assert 0.5 * MEASURED_WORST < err.max() < 2 * MEASURED_WORST, "the measured value written above is stale"


def test_chi2_never_rises_and_falls_for_every_refined_point():
    for args in ((0.0, 0, 2), (0.5, 0, 2), (0.5, 1, 3)):
        _, (out, chi2, info, flags) = run(*args)
        assert (chi2[:, 1] <= chi2[:, 0]).all()
        refined = info[:, 0] == R.REFINED
        assert refined.sum() > 250 and (chi2[refined, 1] < chi2[refined, 0]).all()
        assert (chi2[~refined, 1] == chi2[~refined, 0]).all()


def test_noisy_pixels_end_nearer_the_truth():
    (truth, pos, *_), (out, chi2, info, flags) = run(0.5, 0, 2)
    nearer = rel_err(out, truth) < rel_err(pos, truth)
    print("0.5 px noise: %.1f %% of the points end nearer the truth" % (100 * nearer.mean()))
    assert nearer.mean() > 0.95


def test_a_moved_observation_is_flagged_and_huber_lands_nearer_the_truth():
    (truth, pos, T, frame, uv, start, moved), huber = run(0.0, 1, 3)
    _, plain = run(0.0, 1, 3, 1e9)
    assert (moved >= 0).all() and (huber[2][:, 0] == R.REFINED).all() and (plain[2][:, 0] == R.REFINED).all()
    assert huber[3][moved].all(), "a moved observation is not flagged"
    assert huber[3].sum() < 1.1 * 300      # (with three observations the pull of the moved one can push another past delta)
    assert not plain[3].any()
    better = rel_err(huber[0], truth) < rel_err(plain[0], truth)
    print("a moved observation: Huber is nearer the truth than huber_delta = 1e9 on %d of 300 points" % better.sum())
    assert better.all()


def test_the_exact_point_with_consistent_pixels_takes_no_step():
    """Point (0.25, -0.5, 2), cameras at (0, 0, 0), (0.5, 0, 1) and (-1, 0.25, -2) without rotation: depths 2, 1, 4, every
    projection exact in f64 and representable in f32.  chi2 = 0 and b = 0: d = 0, chi2' = 0 is not below 0, every trial fails."""
    T = np.stack([translation(0, 0, 0), translation(0.5, 0, 1), translation(-1, 0.25, -2)])
    pos = np.float32([[0.25, -0.5, 2.0]])
    uv = np.float32([[384, 112], [192, -16], [480, 144]])     # 320 + 512 x / z, 240 + 512 y / z
    out, chi2, info, flags = R.refine(pos, T, K2, [0, 1, 2], uv, [0, 3])
    assert info.tolist() == [[R.NO_STEP, 0, 20]] and chi2.tolist() == [[0.0, 0.0]] and not flags.any()
    assert out.tobytes() == pos.tobytes()
    # one pixel off by 1: chi2 starts at exactly 1 and the point moves
    uv[1, 0] += 1
    out, chi2, info, flags = R.refine(pos, T, K2, [0, 1, 2], uv, [0, 3])
    assert info[0, 0] == R.REFINED and chi2[0, 0] == 1.0 and 0 < chi2[0, 1] < 1.0 and out.tobytes() != pos.tobytes()


def test_a_point_behind_one_camera_is_left_alone():
    T = np.stack([translation(0, 0, 0), translation(0.5, 0, 1), translation(0, 0, 2.5)])      # the third looks at it from behind
    pos = np.float32([[0.25, -0.5, 2.0]])
    uv = np.float32([[384, 112], [192, -16], [300, 200]])
    out, chi2, info, flags = R.refine(pos, T, K2, [0, 1, 2], uv, [0, 3])
    assert info.tolist() == [[R.BEHIND, 0, 0]] and chi2.tolist() == [[0.0, 0.0]] and not flags.any() and out.tobytes() == pos.tobytes()
    T[2] = translation(0, 0, 2.0)                               # depth exactly 0: !(q_z > 0)
    assert R.refine(pos, T, K2, [0, 1, 2], uv, [0, 3])[2][0, 0] == R.BEHIND


def test_too_few_observations():
    T = np.stack([translation(0, 0, 0), translation(0.5, 0, 1)])
    pos = np.float32([[0.25, -0.5, 2.0], [0.25, -0.5, 2.0], [0.25, -0.5, 2.0]])
    uv = np.float32([[385, 112], [385, 112], [192, -16]])
    out, chi2, info, flags = R.refine(pos, T, K2, [0, 0, 1], uv, [0, 0, 1, 3])      # m = 0, 1, 2
    assert info[:, 0].tolist() == [R.TOO_FEW, R.TOO_FEW, R.REFINED] and not info[:2, 1:].any() and not chi2[:2].any()
    assert out[:2].tobytes() == pos[:2].tobytes() and out[2].tobytes() != pos[2].tobytes()
    info = R.refine(pos, T, K2, [0, 0, 1], uv, [0, 0, 1, 3], dict(min_observations=3))[2]
    assert info[:, 0].tolist() == [R.TOO_FEW] * 3


def test_the_sums_the_solve_and_the_huber_branch():
    """One observation by hand: camera at the origin, K2, point (0, 0, 2), pixel (323, 236): e = (-3, 4), e2 = 25 > d^2 = 4 with
    d = 2: rho = 2 * 2 * 5 - 4 = 16, w = 2 / 5.  J = [256, 0, 0; 0, 256, 0]: H = w * 65536 * diag(1, 1, 0), b = w * 256 * (-3, 4, 0)."""
    Tcw = np.eye(4)[None, :3]
    H, b, chi2, e2, front = R.evaluate([np.float64(0), np.float64(0), np.float64(2)], Tcw, np.float32([[323, 236]]), K2, 2.0)
    w = np.float64(2.0) / np.float64(5.0)
    assert e2.tolist() == [25.0] and chi2 == 16.0 and front.all()
    assert H == [w * 65536.0, 0.0, 0.0, w * 65536.0, 0.0, 0.0] and b == [w * -768.0, w * 1024.0, 0.0]
    H, b, chi2, e2, front = R.evaluate([np.float64(0), np.float64(0), np.float64(2)], Tcw, np.float32([[323, 236]]), K2, 5.0)
    assert chi2 == 25.0 and H[0] == 65536.0 and b[:2] == [-768.0, 1024.0]       # e2 <= d^2 is inclusive: the quadratic branch
    # the Cholesky solve against numpy's, and a pivot that is not positive
    A = np.array([[4.0, 2.0, 0.6], [2.0, 5.0, 1.0], [0.6, 1.0, 3.0]])
    g = [1.0, -2.0, 0.5]
    d = R.solve([np.float64(v) for v in (4.0, 2.0, 0.6, 5.0, 1.0, 3.0)], [np.float64(v) for v in g], np.float64(0.25))
    assert np.allclose(d, np.linalg.solve(A + 0.25 * np.eye(3), -np.array(g)), rtol=1e-14, atol=0)
    assert R.solve([np.float64(v) for v in (1.0, 2.0, 0.0, 1.0, 0.0, 1.0)], [np.float64(0)] * 3, np.float64(0.5)) is None
    assert R.ordered_sum([1e16, 1.0, 1.0]) == 1e16 and R.ordered_sum([1.0, 1.0, 1e16]) == 1e16 + 2
