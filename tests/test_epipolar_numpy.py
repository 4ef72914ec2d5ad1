"""Known answers of tests/epipolar_numpy.py itself, the transcription the pose-guided matcher is compared with: the exact
gate on a line whose arithmetic can be done by hand, the tie rule, the filter and the one-query-per-train rule, F from
poses on noise-free projections, and the two-view scene that shows what the feature is for.  No GPU, no library."""
import numpy as np

import epipolar_numpy as E

F_ROW = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float64)     # line of (x, y): -v + y = 0, nrm = 1


def exact_gate_inputs():
    up, down = np.nextafter(np.float32(102), np.float32(200)), np.nextafter(np.float32(98), np.float32(0))
    qxy = np.array([[10, 100], [20, 50.5], [30, 7]], np.float32)
    txy = np.array([[5, 100], [600, 102], [7, up], [8, 98], [9, down], [300, 50.5]], np.float32)
    return np.zeros((3, 32), np.uint8), qxy, np.zeros((6, 32), np.uint8), txy


def test_exact_gate_is_inclusive_and_its_f32_neighbours_fall_out():
    q, qxy, t, txy = exact_gate_inputs()
    a, b, c, nrm = E.lines(F_ROW, qxy)
    assert (a == 0).all() and (b == -1).all() and (c == qxy[:, 1]).all() and (nrm == 1).all()
    idx, dist, cnt = E.knn2(q, qxy, t, txy, F_ROW, 2.0)
    assert cnt.tolist() == [3, 1, 0]
    assert idx.tolist() == [[0, 1], [5, -1], [-1, -1]]                # (trains 0, 1, 3 pass for query 0: the lower first)
    assert dist.tolist() == [[0, 0], [0, E.INT32_MAX], [E.INT32_MAX, E.INT32_MAX]]
    assert E.gate(F_ROW, qxy, txy, E.tolerances(6, 2.0))[0].tolist() == [True, True, False, True, False, False]


def test_zero_f_and_nan_give_no_candidates():
    q, qxy, t, txy = exact_gate_inputs()
    idx, dist, cnt = E.knn2(q, qxy, t, txy, np.zeros(9), 2.0)
    assert (cnt == 0).all() and (idx == -1).all() and (dist == E.INT32_MAX).all()
    bad = txy.copy()
    bad[0, 1] = np.nan
    assert E.knn2(q, qxy, t, bad, F_ROW, 2.0)[2].tolist() == [2, 1, 0]


def test_scale_widens_the_tolerance_per_train():
    q, qxy, t, txy = exact_gate_inputs()
    txy = txy.copy()
    txy[:, 1] = [100, 102.25, 102.25, 97.25, 96, 50.5]
    scale = np.array([1, 1, 1.2, 1.44, 1.44, 1], np.float32)         # 2.4 px for train 2, 2.88 px for trains 3 and 4
    assert E.gate(F_ROW, qxy, txy, E.tolerances(6, 2.0, scale))[0].tolist() == [True, False, True, True, False, False]
    assert E.tolerances(2, 2.0, np.array([1, 1.2], np.float32)).tolist() == [4.0, (2.0 * float(np.float32(1.2))) ** 2]


def test_ties_keep_the_lower_train_index():
    rng = np.random.RandomState(1)
    t = rng.randint(0, 256, (5, 32)).astype(np.uint8)
    t[3] = t[1]
    q = t[1:2].copy()
    q[0, 0] ^= 1
    xy = np.zeros((5, 2), np.float32)
    idx, dist, cnt = E.knn2(q, xy[:1], t, xy, F_ROW, 2.0)
    assert idx.tolist() == [[1, 3]] and dist.tolist() == [[1, 1]] and cnt.tolist() == [5]
    assert E.hamming(np.zeros((1, 32), np.uint8), np.full((1, 32), 255, np.uint8)).tolist() == [[256]]


def test_filter_and_one_query_per_train():
    I = E.INT32_MAX
    idx = np.array([[4, 2], [4, 1], [3, -1], [0, 1], [2, 0], [-1, -1], [4, 0], [1, -1]], np.int32)
    dist = np.array([[10, 50], [10, 60], [64, I], [40, 50], [65, 200], [I, I], [9, 11], [65, I]], np.int32)
    m = E.filter_matches(idx, dist, 0.8, 64)
    # query 0 and 1 claim train 4 at distance 10: the lower queryIdx survives; query 6 is nearer but fails the ratio
    # (9 >= 0.8 * 11); query 2 has a single candidate at the ceiling: kept; query 3 fails the ratio (40 >= 40.0);
    # queries 4 and 7 are above the ceiling
    assert m["queryIdx"].tolist() == [2, 0] and m["trainIdx"].tolist() == [3, 4]
    assert m["distance"].tolist() == [64.0, 10.0] and (m["imgIdx"] == 0).all()
    # the nearer claim wins whatever the order
    idx2 = np.array([[7, -1], [7, -1], [7, -1]], np.int32)
    dist2 = np.array([[30, I], [12, I], [12, I]], np.int32)
    m2 = E.filter_matches(idx2, dist2, 0.8, 64)
    assert m2["queryIdx"].tolist() == [1] and m2["distance"].tolist() == [12.0]


def test_fundamental_from_poses_on_exact_projections():
    rng = np.random.RandomState(3)
    T1, T2 = np.eye(4), np.eye(4)
    T1[:3, :3], T1[:3, 3] = E.rodrigues([0.01, 0.02, -0.03]), [0.1, -0.2, 0.05]
    T2[:3, :3], T2[:3, 3] = E.rodrigues([-0.04, 0.05, 0.02]), [0.4, 0.1, -0.1]
    X = rng.uniform([-2, -1.5, 3], [2, 1.5, 8], (50, 3))
    p1, _ = E.project(T1, E.FR1_K, X)
    p2, _ = E.project(T2, E.FR1_K, X)
    F = E.fundamental_from_poses(T1, T2, E.FR1_K)
    F /= np.linalg.norm(F)
    h1, h2 = np.c_[p1, np.ones(50)], np.c_[p2, np.ones(50)]
    assert np.abs(np.einsum("ni,ij,nj->n", h2, F, h1)).max() < 1e-9
    # a pure translation along x: the lines are the rows
    T2 = np.eye(4)
    T2[0, 3] = 1.0
    F = E.fundamental_from_poses(np.eye(4), T2, dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0))
    assert np.allclose(F / F[2, 1], F_ROW, atol=1e-15)


def test_two_view_scene_gated_finds_every_partner_ungated_none():
    s = E.two_view_scene()
    n = len(s["d1"])
    assert n == 280 and len(s["d2"]) == 560
    assert E.line_distance(s["F"], s["xy1"], s["xy2"][s["partner"]]).max() < 2.0     # 1.23 px
    assert E.line_distance(s["F"], s["xy1"], s["xy2"][s["twin"]]).min() > 38.0
    cnt = E.knn2(s["d1"], s["xy1"], s["d2"], s["xy2"], s["F"], 2.0)[2]
    assert 5 < cnt.mean() < 9                                                          # 7.1 candidates per query
    m = E.match_features(s["d1"], s["xy1"], s["d2"], s["xy2"], s["F"], 2.0, 0.8, 64)
    assert len(m) == 280 and (s["partner"][m["queryIdx"]] == m["trainIdx"]).sum() == 280
    assert (np.diff(m["trainIdx"]) > 0).all()
    g = E.match_features(s["d1"], s["xy1"], s["d2"], s["xy2"], s["F"], 2.0, 0.8, 64, use_gate=False)
    assert len(g) == 280 and (s["twin"][g["queryIdx"]] == g["trainIdx"]).sum() == 280
    assert (s["partner"][g["queryIdx"]] == g["trainIdx"]).sum() == 0
