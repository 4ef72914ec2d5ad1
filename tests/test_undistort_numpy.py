"""Known answers of tests/undistort_numpy.py, the transcription of the declared undistortion that
the MI355X and the emulated build are compared with (tests/test_gpu_undistort.py, tests/test_undistort_sim.py): it is
pinned to geometry here, without the library, before anything is compared with it."""
import numpy as np

import undistort_numpy as U

CASE_A = (dict(fx=40.0, fy=41.0, cx=33.3, cy=17.1), (0.3, -0.1, 0.01, -0.008, 0.05), 67, 35)
CASE_B = (CASE_A[0], (-0.35, 0.12, 0.01, -0.008), 67, 35)
CASE_C = (dict(fx=129.3, fy=129.1, cx=81.3, cy=62.4), U.FR1_DIST, 160, 120)
CASE_D = (U.FR1_K, U.FR1_DIST, 640, 480)


def distorted_pixel(K, dist, j, i):
    """Where the model puts output pixel (j, i) in the source: a plain scalar evaluation of the Brown-Conrady model written
    separately from the transcription (normalise, radial factor, tangential terms, back to pixels)."""
    k1, k2, p1, p2, k3 = dist
    xn = (j - K["cx"]) / K["fx"]
    yn = (i - K["cy"]) / K["fy"]
    rr = xn * xn + yn * yn
    radial = 1.0 + k1 * rr + k2 * rr ** 2 + k3 * rr ** 3
    xd = xn * radial + 2.0 * p1 * xn * yn + p2 * (rr + 2.0 * xn * xn)
    yd = yn * radial + p1 * (rr + 2.0 * yn * yn) + 2.0 * p2 * xn * yn
    return K["fx"] * xd + K["cx"], K["fy"] * yd + K["cy"]


def test_zero_coefficients_are_the_identity():
    """All-zero coefficients with the fr1 K at 640 x 480: the map is the identity with every fraction 0, and the output is the
    input in every pixel -- the last row and column too, whose outside taps carry weight 0."""
    w, h = 640, 480
    ix, iy, ax, ay = U.undistort_map(U.FR1_K, (0, 0, 0, 0, 0), w, h)
    jj, ii = np.meshgrid(np.arange(w), np.arange(h))
    assert np.array_equal(ix, jj) and np.array_equal(iy, ii)
    assert not ax.any() and not ay.any()
    assert ix.dtype == np.int32 and iy.dtype == np.int32 and ax.dtype == np.uint8 and ay.dtype == np.uint8
    img = np.random.RandomState(5).randint(0, 256, (h, w, 3)).astype(np.uint8)
    out = U.undistort(img, U.FR1_K, (0, 0, 0, 0, 0))
    assert out.dtype == np.uint8 and out.shape == img.shape and np.array_equal(out, img)
    assert np.array_equal(U.undistort(img[:, :, 0], U.FR1_K, (0, 0, 0, 0)), img[:, :, 0])


def test_linear_ramp_follows_the_distortion_model():
    """A ramp round(0.2 x + 0.2 y + 10) (at most 234: u8 does not clip) undistorted with the fr1 set: where all four taps are
    inside, the result is within 1.02 grey levels of 0.2 u + 0.2 v + 10 with (u, v) from distorted_pixel -- 0.5 from rounding
    the ramp, 0.5 from rounding the result, at most 0.02 from the 1/32 px grid at these slopes."""
    K, dist, w, h = CASE_D
    jj, ii = np.meshgrid(np.arange(w), np.arange(h))
    ramp = np.rint(0.2 * jj + 0.2 * ii + 10)
    assert ramp.max() <= 234
    out = U.undistort(ramp.astype(np.uint8), K, dist)
    ix, iy, _, _ = U.undistort_map(K, dist, w, h)
    inside = U.taps_inside(ix, iy, w, h).all(axis=0)
    assert inside.sum() == 289145                      # (1942 pixels have some taps inside, 5.2 % none)
    u, v = distorted_pixel(K, dist, jj.astype(np.float64), ii.astype(np.float64))
    worst = float(np.abs(out - (0.2 * u + 0.2 * v + 10))[inside].max())
    print("ramp: worst deviation %.3f grey levels over %d pixels" % (worst, inside.sum()))
    assert worst <= 1.02


def test_hand_computed_pixels():
    src = np.array([[10, 21], [30, 40]], np.uint8)
    one = lambda v: np.array([[v]])
    # fractions (16, 16): every weight is 32 * 16 * 16 = 8192, the result the rounded mean (101 / 4 = 25.25)
    assert U.remap(src, one(0), one(0), one(16), one(16))[0, 0] == 25
    assert U.remap(np.array([[10, 21], [30, 41]], np.uint8), one(0), one(0), one(16), one(16))[0, 0] == 26   # 25.5 rounds up
    # a tap outside contributes 0: from (0, 1) the right-hand taps are outside -> (21 + 40) / 4 = 15.25
    assert U.remap(src, one(1), one(0), one(16), one(16))[0, 0] == 15
    # from (-1, -1) only the tap (0, 0) is inside -> 10 / 4 = 2.5, rounds up
    assert U.remap(src, one(-1), one(-1), one(16), one(16))[0, 0] == 3
    # all outside
    assert U.remap(src, one(2), one(5), one(16), one(16))[0, 0] == 0
    # fraction 0 picks the tap itself although its neighbours are outside
    assert U.remap(src, one(1), one(1), one(0), one(0))[0, 0] == 40
    # weights: ax = 8, ay = 24 -> (32*8*24*10 + 32*8*8*21 + 32*24*24*30 + 32*24*8*40 + 16384) >> 15
    want = (32 * 8 * 24 * 10 + 32 * 8 * 8 * 21 + 32 * 24 * 24 * 30 + 32 * 24 * 8 * 40 + 16384) >> 15
    assert U.remap(src, one(0), one(0), one(8), one(24))[0, 0] == want == 28       # 27.56 before rounding
    # a negative fixed-point coordinate takes the arithmetic shift and the mask
    for iu, ix, ax in ((-1, -1, 31), (-32, -1, 0), (-33, -2, 31), (31, 0, 31), (32, 1, 0), (-1056, -33, 0)):
        got = U.split(np.array([iu], np.int32))
        assert (int(got[0][0]), int(got[1][0])) == (ix, ax), iu
    # three channels are handled independently
    rgb = np.stack([src, src[::-1], src.T], axis=2)
    out = U.remap(rgb, one(0), one(0), one(16), one(16))
    assert out.shape == (1, 1, 3) and out[0, 0].tolist() == [25, 25, 25]
    assert U.remap(rgb, one(1), one(0), one(0), one(0))[0, 0].tolist() == [21, 40, 30]


def test_rounding_and_coefficient_counts():
    assert U.cv_round_i32([0.5, 1.5, 2.5, -0.5, -1.5, 1e12, -1e12, float("nan")]).tolist() == [0, 2, 2, 0, -2, 2 ** 31 - 1, -2 ** 31, 0]
    assert U.coefficients((1, 2, 3, 4)) == [1, 2, 3, 4, 0, 0, 0, 0]
    assert U.coefficients((1, 2, 3, 4, 5)) == [1, 2, 3, 4, 5, 0, 0, 0]
    for n in (0, 3, 6, 12, 14):
        try:
            U.coefficients([0.0] * n)
        except ValueError:
            continue
        raise AssertionError("%d coefficients accepted" % n)
    # the rational model: with k4..k6 equal to k1..k3 the radial factor is 1 -- only the tangential terms are left
    K, w, h = CASE_A[0], 67, 35
    a = U.fixed_point_coordinates(K, (0.3, -0.1, 0.01, -0.008, 0.05, 0.3, -0.1, 0.05), w, h)
    b = U.fixed_point_coordinates(K, (0, 0, 0.01, -0.008), w, h)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_the_cases_of_the_device_tests_reach_every_branch():
    """What the shapes of tests/test_gpu_undistort.py are chosen for: pixels with some, all and none of their taps inside."""
    def count(K, dist, w, h):
        ix, iy, _, _ = U.undistort_map(K, dist, w, h)
        n = U.taps_inside(ix, iy, w, h).sum(axis=0)
        return int(((n > 0) & (n < 4)).sum()), int((n == 0).sum()), int((n == 4).sum())
    assert count(*CASE_A) == (134, 395, 1816)          # 17 % with no tap inside
    assert count(*CASE_B) == (0, 0, 67 * 35)           # the barrel sign: every tap inside
    assert count(*CASE_C)[0] == 489
    assert count(*CASE_D)[0] == 1942
    iu, iv = U.fixed_point_coordinates(*CASE_D)
    jj, ii = np.meshgrid(np.arange(640), np.arange(480))
    assert 32.5 < np.hypot(iu / 32.0 - jj, iv / 32.0 - ii).max() < 33.5
    # no 32 u of the real configuration is within ulps of a tie (the nearest is 3.7e-7 away), so an evaluation that differs
    # from the declared one by ulps -- OpenCV's running sum, or distorted_pixel here -- rounds to the same grid point
    u, v = distorted_pixel(U.FR1_K, U.FR1_DIST, jj.astype(np.float64), ii.astype(np.float64))
    tie = min(np.abs(np.abs(32 * c - np.floor(32 * c)) - 0.5).min() for c in (u, v))
    print("nearest tie of the fr1 map: %.3g" % tie)
    assert 1e-7 < tie < 1e-6
    assert np.array_equal(U.cv_round_i32(32 * u), iu) and np.array_equal(U.cv_round_i32(32 * v), iv)
