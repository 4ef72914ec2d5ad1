"""Known answers of tests/projection_numpy.py itself, the transcription tracking by projection is compared with: the disc
gate where its arithmetic can be done by hand, the per-keypoint scales, the in-view borders, NaN, the tie rule, the filter
with discs, the pose prediction, and the tracking scene that shows what the feature is for.  No GPU, no library."""
import numpy as np

import projection_numpy as P

K100 = dict(fx=100.0, fy=100.0, cx=50.0, cy=50.0)
I4 = np.eye(4)


def hand_gate_inputs():
    """Identity pose, map point (0, 0, 1) -> pixel (50, 50); max_px 3: trains 0 and 2 lie ON the circle and pass, the f32
    neighbour of 53 and the diagonal point at 3.54 px do not."""
    up = np.nextafter(np.float32(53), np.float32(100))
    pos = np.array([[0, 0, 1]], np.float32)
    txy = np.array([[53, 50], [up, 50], [50, 47], [52.5, 52.5]], np.float32)
    return pos, np.zeros((1, 32), np.uint8), np.zeros((4, 32), np.uint8), txy


def border_points():
    """z < 0, z = 0, exactly on u = 0, exactly on u = cols (100): none is in view; the last one is."""
    return np.array([[0, 0, -1], [0, 0, 0], [-0.5, 0, 1], [0.5, 0, 1], [0.25, 0, 1]], np.float32)


def test_hand_computable_gate_is_inclusive():
    pos, desc, t, txy = hand_gate_inputs()
    u, v, in_view = P.project_map(pos, I4, K100, 100, 100)
    assert u.tolist() == [50.0] and v.tolist() == [50.0] and in_view.tolist() == [True]
    assert P.gate(u, v, in_view, txy, P.radii2(4, 3.0))[0].tolist() == [True, False, True, False]
    px, idx, dist, cnt = P.knn2(pos, desc, I4, K100, 100, 100, t, txy, 3.0)
    assert px.tolist() == [[50.0, 50.0]] and idx.tolist() == [[0, 2]] and dist.tolist() == [[0, 0]] and cnt.tolist() == [2]


def test_scale_widens_the_radius_per_keypoint():
    pos, desc, t, txy = hand_gate_inputs()
    scale = np.array([1, 1.2, 1, 1.2], np.float32)            # 3.6 px for trains 1 and 3 (3.54 px away): both pass now
    u, v, in_view = P.project_map(pos, I4, K100, 100, 100)
    assert P.gate(u, v, in_view, txy, P.radii2(4, 3.0, scale))[0].tolist() == [True, True, True, True]
    assert P.radii2(2, 3.0, np.array([1, 1.2], np.float32)).tolist() == [9.0, (3.0 * float(np.float32(1.2))) ** 2]
    assert P.knn2(pos, desc, I4, K100, 100, 100, t, txy, 3.0, scale)[3].tolist() == [4]


def test_points_behind_at_zero_depth_and_on_the_border_are_not_in_view():
    pos = border_points()
    u, v, in_view = P.project_map(pos, I4, K100, 100, 100)
    assert in_view.tolist() == [False, False, False, False, True]
    assert u[2] == 0.0 and u[3] == 100.0 and u[4] == 75.0
    t, txy = np.zeros((1, 32), np.uint8), np.array([[75, 50]], np.float32)
    px, idx, dist, cnt = P.knn2(pos, np.zeros((5, 32), np.uint8), I4, K100, 100, 100, t, txy, 1e4)
    assert cnt.tolist() == [-1, -1, -1, -1, 1] and px[:4].tolist() == [[0.0, 0.0]] * 4 and px[4].tolist() == [75.0, 50.0]
    assert (idx[:4] == -1).all() and (dist[:4] == P.INT32_MAX).all() and idx[4].tolist() == [0, -1]
    # no keypoints at all: in view 0, the others -1
    assert P.knn2(pos, np.zeros((5, 32), np.uint8), I4, K100, 100, 100, t[:0], txy[:0], 3.0)[3].tolist() == [-1, -1, -1, -1, 0]


def test_nan_position_is_nobodys_candidate():
    pos, desc, t, txy = hand_gate_inputs()
    bad = txy.copy()
    bad[0, 1] = np.nan
    px, idx, dist, cnt = P.knn2(pos, desc, I4, K100, 100, 100, t, bad, 3.0)
    assert cnt.tolist() == [1] and idx.tolist() == [[2, -1]] and dist.tolist() == [[0, P.INT32_MAX]]


def test_ties_keep_the_lower_train_index():
    rng = np.random.RandomState(1)
    t = rng.randint(0, 256, (5, 32)).astype(np.uint8)
    t[3] = t[1]
    desc = t[1:2].copy()
    desc[0, 0] ^= 1
    txy = np.full((5, 2), 50, np.float32)
    px, idx, dist, cnt = P.knn2(np.array([[0, 0, 1]], np.float32), desc, I4, K100, 100, 100, t, txy, 3.0)
    assert idx.tolist() == [[1, 3]] and dist.tolist() == [[1, 1]] and cnt.tolist() == [5]


def flip(d, lo, n):
    bits = np.unpackbits(d)
    bits[lo:lo + n] ^= 1
    return np.packbits(bits)


def filter_case():
    """The filter cases of the epipolar tests with discs in place of rows: groups 100 px apart at depth 1 under the identity
    pose (K: f = 100, c = 500, a 1000 x 1000 frame); a map point sees the keypoints of its own disc only.
    (group: map points -> keypoints at distance).  -> pos, desc, t, txy, K, cols, rows"""
    base = np.random.RandomState(9).randint(0, 256, (8, 32)).astype(np.uint8)
    K = dict(fx=100.0, fy=100.0, cx=500.0, cy=500.0)
    pos, desc, t, txy = [], [], [], []

    def group(g, queries, trains):
        for k, d in enumerate(queries):
            desc.append(d), pos.append([g - 4.0, 0.01 * k, 1.0])          # pixel (100 + 100 g, 500 + k)
        for k, d in enumerate(trains):
            t.append(d), txy.append([100.0 + 100 * g + 0.5 * k, 500.5])

    group(0, [flip(base[0], 0, 3), flip(base[0], 10, 3)], [base[0]])            # q0, q1 claim t0 at distance 3: q0 survives
    group(1, [base[1]], [flip(base[1], 0, 64)])                                 # q2: single candidate at the ceiling: kept
    group(2, [base[2]], [flip(base[2], 0, 65)])                                 # q3: single candidate above it: dropped
    group(3, [base[3]], [flip(base[3], 0, 40), flip(base[3], 0, 50)])           # q4: 40 < 0.8 * 50 is false: dropped
    group(4, [base[4]], [flip(base[4], 0, 50), flip(base[4], 0, 39)])           # q5: 39 < 40: kept, train 6
    group(5, [flip(base[5], 0, 12), flip(base[5], 20, 5)], [base[5]])           # q6, q7 claim t7: the nearer q7 survives
    group(6, [base[6]], [flip(base[6], 0, 70), flip(base[6], 0, 200)])          # q8: passes the ratio, fails the ceiling
    return np.array(pos, np.float32), np.array(desc), np.array(t), np.array(txy, np.float32), K, 1000, 1000


def test_filter_ceiling_ratio_single_candidate_and_one_query_per_train():
    pos, desc, t, txy, K, cols, rows = filter_case()
    cnt = P.knn2(pos, desc, I4, K, cols, rows, t, txy, 3.0)[3]
    assert cnt.tolist() == [1, 1, 1, 1, 2, 2, 1, 1, 2]
    m = P.match_features(pos, desc, I4, K, cols, rows, t, txy, 3.0, 0.8, 64)
    assert m["queryIdx"].tolist() == [0, 2, 5, 7] and m["trainIdx"].tolist() == [0, 1, 6, 7]
    assert m["distance"].tolist() == [3.0, 64.0, 39.0, 5.0] and (m["imgIdx"] == 0).all()
    for ratio, ceiling, queries in ((1.0, 64, [0, 2, 4, 5, 7]), (0.8, 256, [0, 2, 3, 5, 7, 8])):
        assert P.match_features(pos, desc, I4, K, cols, rows, t, txy, 3.0, ratio, ceiling)["queryIdx"].tolist() == queries


def test_invert_pose_and_predict_pose():
    rng = np.random.RandomState(5)
    for _ in range(8):
        A = P.pose(rng.uniform(-0.4, 0.4, 3), rng.uniform(-2, 2, 3))
        B = P.pose(rng.uniform(-0.4, 0.4, 3), rng.uniform(-2, 2, 3))
        assert np.abs(P.invert_pose(A) - np.linalg.inv(A)).max() <= 1e-12 * np.abs(A).max()
        want = B @ (np.linalg.inv(A) @ B)
        assert np.abs(P.predict_pose(A, B) - want).max() <= 1e-12 * np.abs(want).max()
        assert np.array_equal(P.predict_pose(None, B), B)
    assert P.invert_pose(np.zeros((4, 4))) is None
    # a constant screw motion sampled at three instants: the third is predicted from the first two
    M = P.pose([0.02, -0.03, 0.05], [0.1, 0.02, -0.04])
    T0 = P.pose([0.3, 0.1, -0.2], [1.0, -0.5, 0.3])
    T1 = T0 @ M
    assert np.abs(P.predict_pose(T0, T1) - T1 @ M).max() < 1e-9


def test_tracking_scene_prediction_finds_every_partner_the_other_searches_do_not():
    s = P.tracking_scene()
    a = (s["pos"], s["desc"])
    b = (s["K"], s["cols"], s["rows"], s["t"], s["txy"])
    n = len(s["seen"])
    assert n == 343 and len(s["t"]) == 686
    u, v, in_view = P.project_map(s["pos"], s["T_pred"], s["K"], s["cols"], s["rows"])
    assert in_view.sum() == 348 and in_view[s["seen"]].all()
    se = s["seen"]
    d_partner = np.hypot(s["txy"][s["partner"], 0] - u[se], s["txy"][s["partner"], 1] - v[se])
    d_twin = np.hypot(s["txy"][s["twin"], 0] - u[se], s["txy"][s["twin"], 1] - v[se])
    assert d_partner.max() < 3.5 and d_twin.min() > 36.0                          # 3.30 px, 36.8 px
    cnt = P.knn2(*a, s["T_pred"], *b, 6.0)[3]
    assert 1.3 < cnt[cnt >= 0].mean() < 1.5                                       # 1.41 candidates per point in view
    # all seen points matched to their partners under the prediction
    assert P.scene_score(s, P.match_features(*a, s["T_pred"], *b, 6.0, 0.8, 64)) == (343, 343, 0)
    # fewer than half under the keyframe pose at either radius
    near, wide = (P.scene_score(s, P.match_features(*a, s["T_key"], *b, r, 0.8, 64)) for r in (6.0, 50.0))
    assert near == (18, 17, 1) and wide == (343, 109, 234)
    assert 2 * near[1] < n and 2 * wide[1] < n
    # no partner found by the global search
    assert P.scene_score(s, P.match_features(*a, s["T_key"], *b, 6.0, 0.8, 64, use_gate=False)) == (343, 0, 343)
