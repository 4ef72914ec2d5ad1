"""Known answers of tests/window_triangulate_numpy.py itself, the transcription the triangulation of new map points against every
buffered frame is compared with: the gate on a line whose arithmetic can be done by hand, keypoints that
are not free on either side, frames without a baseline, the contested train, every status bit on numbers chosen so that the bound
is met exactly, the choice; and the scene of the CPU prototype, which shows what the step is for.  No GPU, no library (the DLT is
the CPU oracle's)."""
import functools

import numpy as np

import window_triangulate_numpy as W

K1 = dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0)                              # pixels are normalised coordinates
F_ROW = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float64)       # line of (x, y): -v + y = 0, nrm = 1


def shift(x=0.0, y=0.0, z=0.0):
    T = np.eye(4)
    T[:3, 3] = [x, y, z]
    return T


def view(xy, T, desc=None, conn=None, scale=None):
    xy = np.array(xy, np.float32).reshape(-1, 2)
    n = len(xy)
    return dict(desc=np.zeros((n, 32), np.uint8) if desc is None else np.array(desc, np.uint8).reshape(n, 32), xy=xy,
                scale=None if scale is None else np.array(scale, np.float32), conn=np.full(n, -1, np.int32) if conn is None
                else np.array(conn, np.int32), T=T)


def bits(k):
    """A descriptor with its first k bits set: k bits from the zero descriptor."""
    d = np.zeros(256, np.uint8)
    d[:k] = 1
    return np.packbits(d)


def test_the_frame_one_unit_to_the_left_has_the_row_line():
    F = W.fundamental(np.eye(4), shift(-1), K1)
    assert np.array_equal(F, F_ROW)
    R, t, active = W.relative(view([], np.eye(4)), view([], shift(-1)), 0.0)
    assert np.array_equal(R, np.eye(3)) and t.tolist() == [-1, 0, 0] and active


def test_exact_gate_is_inclusive_and_its_f32_neighbours_fall_out():
    up, down = np.nextafter(np.float32(102), np.float32(200)), np.nextafter(np.float32(98), np.float32(0))
    curr = view([[10, 100], [20, 50.5], [30, 7]], np.eye(4))
    fr = view([[5, 100], [600, 102], [7, up], [8, 98], [9, down], [300, 50.5]], shift(-1))
    idx, dist, cnt = W.search(curr, [fr], K1, 2.0)
    assert cnt.tolist() == [[3, 1, 0]]
    assert idx.tolist() == [[[0, 1], [5, -1], [-1, -1]]]                # (trains 0, 1, 3 pass for keypoint 0: the lower first)
    assert dist.tolist() == [[[0, 0], [0, W.INT32_MAX], [W.INT32_MAX, W.INT32_MAX]]]
    # the scale of a train widens its gate: 2.4 px for a train of scale 1.2
    wide = dict(fr, scale=np.array([1, 1, 1.2, 1, 1.2, 1], np.float32))
    assert W.search(curr, [wide], K1, 2.0)[2].tolist() == [[5, 1, 0]]


def test_a_train_that_is_not_free_never_passes_and_a_keypoint_that_is_not_free_is_not_active():
    curr = view([[10, 100], [20, 100]], np.eye(4), desc=[bits(0), bits(0)], conn=[-1, 7])
    # train 0 would win at distance 0 but is connected; train 1 (5 bits) is free; train 2 left the map (-2): not free either
    fr = view([[5, 100], [6, 100], [7, 100]], shift(-1), desc=[bits(0), bits(5), bits(1)], conn=[3, -1, -2])
    idx, dist, cnt = W.search(curr, [fr], K1, 2.0)
    assert idx[0].tolist() == [[1, -1], [-1, -1]] and dist[0].tolist() == [[5, W.INT32_MAX], [W.INT32_MAX, W.INT32_MAX]]
    assert cnt[0].tolist() == [1, -1]
    free = dict(fr, conn=np.full(3, -1, np.int32))
    assert W.search(curr, [free], K1, 2.0)[0][0].tolist() == [[0, 2], [-1, -1]]


def test_frames_without_a_baseline_are_not_active():
    curr = view([[0.0, 0.0]], np.eye(4))
    frames = [view([[0.25, 0.0]], shift(-1)), view([[0.0, 0.0]], np.eye(4)), view([[0.025, 0.0]], shift(-0.1))]
    idx, dist, cnt = W.search(curr, frames, K1, 2.0, 0.0)
    assert cnt.tolist() == [[1], [-1], [1]] and idx[1].tolist() == [[-1, -1]] and dist[1].tolist() == [[W.INT32_MAX] * 2]
    assert W.search(curr, frames, K1, 2.0, 0.5)[2].tolist() == [[1], [-1], [-1]]        # 0.1 < 0.5
    assert W.search(curr, frames, K1, 2.0, 1.0)[2].tolist() == [[1], [-1], [-1]]        # the test is b2 >= min^2: 1 >= 1
    assert W.search(curr, frames, K1, 2.0, np.nextafter(1.0, 2.0))[2].tolist() == [[-1], [-1], [-1]]
    counts = W.window_triangulate(curr, frames, K1, min_baseline=0.5)[2]
    assert counts[0] == 1 and counts[1] == 1


def test_two_keypoints_claiming_one_train_smaller_distance_then_lower_keypoint():
    # keypoints 0, 1, 2 on one row; the only train of the frame is 4, 3 and 3 bits away from them
    curr = view([[0, 0], [0.1, 0], [0.2, 0]], np.eye(4), desc=[bits(4), bits(3), bits(3)])
    # (bits(k) against bits(0): k; the train is bits(0))
    fr = view([[0.5, 0]], shift(-1), desc=[bits(0)])
    idx, dist, _ = W.search(curr, [fr], K1, 2.0)
    assert dist[0][:, 0].tolist() == [4, 3, 3]
    rows = W.filter_pairs(idx, dist, 0.8, 64)
    assert rows.tolist() == [[0, 1, 0, 3]]
    assert W.filter_pairs(idx, dist, 0.8, 2).tolist() == []             # the ceiling
    # pairs are ordered by (frame, train)
    two = view([[0.5, 0], [0.45, 0]], shift(-1), desc=[bits(0), bits(200)])
    c2 = view([[0, 0], [0.1, 0]], np.eye(4), desc=[bits(201), bits(1)])
    idx, dist, _ = W.search(c2, [two, two], K1, 2.0)
    assert W.filter_pairs(idx, dist, 0.8, 64).tolist() == [[0, 1, 0, 1], [0, 0, 1, 1], [1, 1, 0, 1], [1, 0, 1, 1]]


def test_a_pair_on_the_far_side_of_the_epipole_has_negative_depth():
    # the point (0, 0, 4) of curr lies at (1, 0, 4) in the frame one unit to the left: pixel (0.25, 0).  The pixel (-0.25, 0) is on
    # the same line, on the other side of the epipole (at infinity along the row): the rays meet 4 units BEHIND the cameras
    curr = view([[0, 0]], np.eye(4))
    good, bad = view([[0.25, 0]], shift(-1)), view([[-0.25, 0]], shift(-1))
    points, pairs, counts, _ = W.window_triangulate(curr, [good, bad], K1)
    assert pairs["status"].tolist() == [0, W.DEPTH]      # (v1 = (0, 0, -4), v2 = (1, 0, -4): the parallax is that of the good pair)
    assert np.allclose(pairs["p_curr"], [[0, 0, 4], [0, 0, -4]], atol=1e-5)
    assert np.allclose(pairs["p_frame"], [[1, 0, 4], [1, 0, -4]], atol=1e-5)
    assert counts.tolist() == [1, 2, 2, 2, 0, 1, 0, 0, 0, 0, 1, 1]
    assert points["frame"].tolist() == [0] and points["keypoint"].tolist() == [0] and points["train"].tolist() == [0]
    assert abs(pairs["cos2"][0] - 16.0 / 17.0) < 1e-6 and abs(pairs["cos2"][1] - 16.0 / 17.0) < 1e-6


def stub(p_f, p_c):
    """A triangulation that answers with the given points (the tests below choose numbers that meet a bound exactly)."""
    def triangulate(kp1, kp2, K, R, t):
        return (np.tile(np.array(p_f, np.float32), (len(kp1), 1)), np.tile(np.array(p_c, np.float32), (len(kp1), 1)))
    return triangulate


ROW = np.array([[0, 0, 0, 0]], np.int32)                                # frame 0, keypoint 0, train 0, distance 0
LOOSE = dict(max_cos_parallax=1.0, max_reproj_chi2=np.inf, ratio_factor=np.inf)


def status(curr, fr, p_f, p_c, **kw):
    return int(W.verify(curr, [fr], K1, ROW, triangulate=stub(p_f, p_c), **dict(LOOSE, **kw))["status"][0])


def test_parallax_at_the_bound_and_just_inside_it():
    # v1 = (1, 0, 1), t = (1, -1, 0): v2 = (0, 1, 1); dot = 1, n1 = n2 = 2: cos2 = 1 / 4 exactly
    curr, fr = view([[1, 0]], np.eye(4)), view([[0, 1]], shift(1, -1))
    p = W.verify(curr, [fr], K1, ROW, triangulate=stub((0, 1, 1), (1, 0, 1)), **LOOSE)
    assert p["cos2"][0] == 0.25 and p["status"][0] == 0
    assert status(curr, fr, (0, 1, 1), (1, 0, 1), max_cos_parallax=0.5) == W.PARALLAX                # cos2 < c2max is strict
    assert status(curr, fr, (0, 1, 1), (1, 0, 1), max_cos_parallax=np.nextafter(0.5, 1.0)) == 0
    # rays that point apart: dot <= 0 fails whatever the bound
    assert status(view([[1, 0]], np.eye(4)), view([[-1, 0]], shift(2)), (-1, 0, 1), (1, 0, 1)) == W.PARALLAX


def test_reprojection_error_exactly_at_the_bound_and_one_ulp_over_it():
    # p_c = (1, 0, 2) projects to (0.5, 0); the keypoint of curr is at (0.25, 0): e2 = 1 / 16.  p_f = (0, 1, 2) -> (0, 0.5), its
    # keypoint at (0, 0.5): e2 = 0
    curr, fr = view([[0.25, 0]], np.eye(4)), view([[0, 0.5]], shift(1, -1))
    assert status(curr, fr, (0, 1, 2), (1, 0, 2), max_reproj_chi2=0.0625) == 0                       # inclusive
    assert status(curr, fr, (0, 1, 2), (1, 0, 2), max_reproj_chi2=np.nextafter(0.0625, 0.0)) == W.REPROJ_CURR
    # the same error in the frame: bit 8
    curr, fr = view([[0.5, 0]], np.eye(4)), view([[0, 0.25]], shift(1, -1))
    assert status(curr, fr, (0, 1, 2), (1, 0, 2), max_reproj_chi2=0.0625) == 0
    assert status(curr, fr, (0, 1, 2), (1, 0, 2), max_reproj_chi2=np.nextafter(0.0625, 0.0)) == W.REPROJ_FRAME
    # a keypoint of scale 2 has four times the bound
    fr2 = dict(fr, scale=np.array([2.0], np.float32))
    assert status(curr, fr2, (0, 1, 2), (1, 0, 2), max_reproj_chi2=0.015625) == 0
    assert status(curr, fr2, (0, 1, 2), (1, 0, 2), max_reproj_chi2=np.nextafter(0.015625, 0.0)) == W.REPROJ_FRAME
    # a NaN fails: a point at depth 0 in the frame
    assert status(curr, fr, (0, 0, 0), (1, 0, 2)) & W.REPROJ_FRAME


def test_both_sides_of_the_scale_test():
    curr, fr = view([[0, 0]], np.eye(4)), view([[0, 0]], shift(1, -1))
    # a = |p_f|^2 s_f^2 = 4, b = |p_c|^2 s_c^2 = 1: a <= b rf2 holds down to ratio_factor 2
    assert status(curr, fr, (0, 0, 2), (0, 0, 1), ratio_factor=2.0) == 0
    assert status(curr, fr, (0, 0, 2), (0, 0, 1), ratio_factor=np.nextafter(2.0, 0.0)) == W.SCALE
    # a = 1, b = 4: a rf2 >= b
    assert status(curr, fr, (0, 0, 1), (0, 0, 2), ratio_factor=2.0) == 0
    assert status(curr, fr, (0, 0, 1), (0, 0, 2), ratio_factor=np.nextafter(2.0, 0.0)) == W.SCALE
    # equal distances, scales 2 and 1: the same numbers through the scales
    c2 = dict(curr, scale=np.array([2.0], np.float32))
    assert status(c2, fr, (0, 0, 1), (0, 0, 1), ratio_factor=2.0) == 0
    assert status(c2, fr, (0, 0, 1), (0, 0, 1), ratio_factor=1.9) == W.SCALE


def test_not_finite_and_every_test_is_evaluated():
    curr, fr = view([[0, 0]], np.eye(4)), view([[0, 0]], shift(1, -1))
    s = status(curr, fr, (np.nan, 0, 1), (0, 0, -1))
    assert s == W.NOT_FINITE | W.DEPTH | W.REPROJ_FRAME | W.SCALE        # (dot = 1 > 0 and cos2 = 1 / 2 < 1: the parallax holds)
    assert status(curr, fr, (0, 0, np.inf), (0, 0, 1)) & W.NOT_FINITE


def test_a_keypoint_accepted_in_two_frames_takes_the_smaller_cos2():
    # (0, 0, 4) seen from one unit and from two units to the left: the wider baseline is frame 1
    curr = view([[0, 0]], np.eye(4))
    frames = [view([[0.25, 0]], shift(-1)), view([[0.5, 0]], shift(-2))]
    points, pairs, counts, _ = W.window_triangulate(curr, frames, K1)
    assert pairs["status"].tolist() == [0, 0] and pairs["cos2"][1] < pairs["cos2"][0]
    assert points["frame"].tolist() == [1] and points["cos2"][0] == pairs["cos2"][1]
    assert points["p_curr"].tobytes() == pairs["p_curr"][1].tobytes()
    assert counts[10] == 2 and counts[11] == 1
    # ... in either order
    points = W.window_triangulate(curr, frames[::-1], K1)[0]
    assert points["frame"].tolist() == [0]


def test_equal_cos2_takes_the_lower_frame():
    curr = view([[0, 0], [0.3, 0.1]], np.eye(4), desc=[bits(0), bits(128)])
    fr = view([[0.5, 0], [0.8, 0.1]], shift(-2), desc=[bits(0), bits(128)])
    near = view([[0.25, 0]], shift(-1))
    points, pairs, _, _ = W.window_triangulate(curr, [near, fr, dict(fr)], K1)
    assert pairs["frame"].tolist() == [0, 1, 1, 2, 2] and (pairs["status"] == 0).all()
    assert pairs["cos2"][1] == pairs["cos2"][3] and pairs["cos2"][2] == pairs["cos2"][4]
    assert points["keypoint"].tolist() == [0, 1] and points["frame"].tolist() == [1, 1]              # sorted by keypoint
    # the rule in choose() itself, on records written by hand
    p = np.zeros(4, W.PAIR)
    p["frame"], p["keypoint"], p["status"], p["cos2"] = [0, 1, 2, 3], [5, 5, 5, 5], [4, 0, 0, 0], [0.1, 0.5, 0.5, 0.7]
    assert W.choose(p)["frame"].tolist() == [1]
    assert len(W.choose(p[:1])) == 0


# ---------------------------------------------------------------------------------------------- the scene of the prototype
# against the nearest frame alone: pairs, pairs failing the parallax test, points (150 of 385)
NEAREST = (383, 233, 150)


@functools.lru_cache(maxsize=None)
def prototype():
    s = W.prototype_scene()
    window = W.window_triangulate(s["curr"], s["frames"], W.FR1_K)
    nearest = W.window_triangulate(s["curr"], s["frames"][-1:], W.FR1_K)
    return s, window, nearest


def true_pair(s, pairs, frame_of=lambda f: f):
    pc = s["point_c"][pairs["keypoint"]]
    pf = np.array([s["point_f"][frame_of(f)][j] for f, j in zip(pairs["frame"], pairs["train"])], np.int32).reshape(-1)
    return (pc >= 0) & (pc == pf)


def test_prototype_scene_every_accepted_pair_is_a_true_pair():
    s, (points, pairs, counts, _), _ = prototype()
    ok = pairs[pairs["status"] == 0]
    assert len(ok) and true_pair(s, ok).all()
    chosen = np.zeros(len(points), W.PAIR)
    chosen["keypoint"], chosen["frame"], chosen["train"] = points["keypoint"], points["frame"], points["train"]
    assert true_pair(s, chosen).all()


def test_prototype_scene_the_window_gives_nearly_every_real_keypoint_a_point_and_the_nearest_frame_alone_does_not():
    """6 cameras 0.083 apart, 400 points at depth 2 to 6, 0.5 px noise, 15 flipped bits, a quarter of the keypoints distractors (the
    prototype of the issue measured 333 of 334 and 160 of 332 on its seed; this fixture's own counts are asserted exactly)."""
    s, (points, pairs, counts, _), (near_points, near_pairs, near_counts, _) = prototype()
    real = int((s["point_c"] >= 0).sum())
    print("keypoints %d, real %d; window: counts %r; nearest frame alone: counts %r" % (len(s["point_c"]), real, counts.tolist(),
                                                                                       near_counts.tolist()))
    assert (s["point_c"][points["keypoint"]] >= 0).all()
    assert len(points) >= real - 1
    assert len(near_points) < real / 2
    assert true_pair(s, near_pairs[near_pairs["status"] == 0], lambda f: len(s["frames"]) - 1).all()
    # the fixture's own numbers
    assert (len(s["point_c"]), real) == (513, 385)
    assert counts.tolist() == [513, 5, 2554, 1871, 0, 0, 233, 0, 0, 0, 1638, 384]
    assert (int(near_counts[3]), int(near_counts[6]), len(near_points)) == NEAREST

