"""Known answers of the numpy transcription of tracking the local map (tests/local_map_numpy.py), worked
by hand.  The camera looks down +z with K100 (fx = fy = 100, cx = cy = 50, a 100 x 100 frame), so a point on the axis projects
to (50, 50) exactly, and with the camera on the axis at -c a point at the origin has dist = c exactly (sqrt(fl(c c)) = c in
binary floating point).  Every check_* takes the raw call as an argument: here the transcription, in
tests/test_gpu_local_map.py the library on the MI355X, in tests/test_local_map_sim.py the emulated build."""
import numpy as np

import local_map_numpy as LM
from test_projection_numpy import I4, K100

DYADIC = np.array([1.0, 2.0, 4.0, 8.0])
Z32 = np.zeros((1, 32), np.uint8)
NOT_ACTIVE = ([0.0, 0.0], [-1, -1], [LM.INT32_MAX, LM.INT32_MAX], -1, -1, 0.0)


def camera_at(c):
    """The camera on the axis at z = -c, looking down +z."""
    T = np.eye(4)
    T[2, 3] = -c
    return T


def one_point(run, T, normal, max_dist, ls, txy, t_level, pos=(0, 0, 0), skip=None, params=None, t=None):
    """One map point with the zero descriptor and keypoints with zero descriptors (or t) -> the row as python values."""
    txy = np.asarray(txy, np.float32).reshape(-1, 2)
    t = np.zeros((len(txy), 32), np.uint8) if t is None else t
    px, idx, dist, cnt, lv, vc = run(np.array([pos], np.float32), Z32, np.array([normal], np.float32), np.array([max_dist], np.float32),
                                     T, K100, 100, 100, t, txy, np.asarray(t_level, np.int32), np.asarray(ls, np.float64),
                                     None if skip is None else np.array([skip], np.uint8), params)
    return px[0].tolist(), idx[0].tolist(), dist[0].tolist(), int(cnt[0]), int(lv[0]), float(vc[0])


AXIS = (0, 0, 1)          # the normal along the viewing direction: vc = c / c = 1
HALF = (0, 0, 0.5)        # vc = (0.5 c) / c = 0.5 exactly: the far radius, 4 px times the level's scale
AT = [[50, 50]]


def check_levels(run):
    # md = 8, levels 1 2 4 8: dist 4 -> 4 < 8, 8 < 8 is not counted -> lv 1; dist 2 -> 2, 4 < 8, 8 not -> lv 2
    assert one_point(run, camera_at(4.0), AXIS, 8.0, DYADIC, AT, [1])[3:] == (1, 1, 1.0)
    assert one_point(run, camera_at(2.0), AXIS, 8.0, DYADIC, AT, [2])[3:] == (1, 2, 1.0)
    # dist 8 = md: nothing counted, lv 0 accepts octave 0 only (lv - 1 = -1 is nobody's octave, and not the taken mark -2)
    assert one_point(run, camera_at(8.0), AXIS, 8.0, DYADIC, AT * 3, [1, 0, -2])[1:5] == ([1, -1], [0, LM.INT32_MAX], 1, 0)
    # dist 1: 1, 2, 4 < 8 -> lv 3 = L - 1; the window is lv - 1 and lv, not lv + 1 (lv 2 with octaves 1 2 3)
    assert one_point(run, camera_at(1.0), AXIS, 8.0, DYADIC, AT * 4, [3, 2, 1, 0])[1:5] == ([0, 1], [0, 0], 2, 3)
    assert one_point(run, camera_at(2.0), AXIS, 8.0, DYADIC, AT * 3, [3, 2, 1])[1:5] == ([1, 2], [0, 0], 2, 2)
    # L = 1: lv 0 at either end of the range [0.8 md, 1.2 md]
    assert one_point(run, camera_at(8.0), AXIS, 8.0, [1.0], AT, [0])[3:] == (1, 0, 1.0)
    assert one_point(run, camera_at(7.0), AXIS, 8.0, [1.0], AT, [0])[3:] == (1, 0, 1.0)


def check_range(run):
    for ls in (DYADIC, [1.0], LM.level_scales(1.2, 8)):
        md = np.float64(np.float32(5.3))
        lo = np.float64(0.8) * (md / np.float64(ls[-1]))
        hi = np.float64(1.2) * md
        for c, active in ((lo, True), (np.nextafter(lo, 0), False), (hi, True), (np.nextafter(hi, np.inf), False)):
            row = one_point(run, camera_at(c), AXIS, md, ls, AT, [0])
            assert (row[3] >= 0) == active, (ls, c)
            if not active:
                assert row == NOT_ACTIVE
    # max_dist <= 0: never in range, whatever the distance
    for md in (0.0, -1.0, np.nan):
        assert one_point(run, camera_at(1.0), AXIS, md, [1.0], AT, [0]) == NOT_ACTIVE


def find_cos(target):
    """d = (dx, 0, dz) from the camera to the point with fl(dz / fl(sqrt(fl(fl(dx dx) + fl(dz dz))))) == target exactly (normal
    +z); found by stepping dx ulp by ulp."""
    dz = np.float64(target) * 4
    dx = np.sqrt(np.float64(16.0) - dz * dz) * (1 + 2e-13)          # from a few ulps of the cosine below the target
    for _ in range(8000):
        s = dx * dx
        s = s + np.float64(0.0) * np.float64(0.0)
        s = s + dz * dz
        if dz / np.sqrt(s) == np.float64(target):
            return dx, dz
        dx = np.nextafter(dx, 0)
    raise AssertionError("no such direction")


def check_facing_and_radius(run):
    # vc == 0.5 is kept (inclusive), one ulp of the f32 normal below is not, a NaN normal is not
    row = one_point(run, camera_at(3.0), HALF, 3.0, [1.0], AT, [0])
    assert row[3:] == (1, 0, 0.5)
    assert one_point(run, camera_at(3.0), (0, 0, np.nextafter(np.float32(0.5), np.float32(0))), 3.0, [1.0], AT, [0]) == NOT_ACTIVE
    assert one_point(run, camera_at(3.0), (0, np.nan, 1), 3.0, [1.0], AT, [0]) == NOT_ACTIVE
    # vc == 0.998 exactly takes radius_far (vc > near_cos is strict): a keypoint 3 px away passes; with vc = 1 it does not
    dx, dz = find_cos(0.998)
    T = np.eye(4)
    T[0, 3], T[2, 3] = -dx, -dz
    w = LM.view(np.zeros((1, 3), np.float32), [AXIS], [4.0], T, K100, 100, 100, [1.0])
    assert w["vc"][0] == 0.998 and w["in_view"][0]
    at = [[float(w["u"][0]) + 3.0, float(w["v"][0])]]
    row = one_point(run, T, AXIS, 4.0, [1.0], at, [0])
    assert row[1] == [0, -1] and row[3] == 1 and row[5] == 0.998
    assert one_point(run, camera_at(4.0), AXIS, 4.0, [1.0], [[53, 50]], [0])[3:] == (0, 0, 1.0)
    assert one_point(run, camera_at(4.0), AXIS, 4.0, [1.0], [[52.5, 50]], [0])[3:] == (1, 0, 1.0)       # 2.5 px, inclusive


def check_disc_taken_skip(run):
    # r = 4 px (vc 0.5 -> far) times level_scale[lv]: inclusive at 4 px on level 0, at 8 px on level 1
    far = np.nextafter(np.float32(54), np.float32(60))
    assert one_point(run, camera_at(3.0), HALF, 3.0, [1.0], [[54, 50], [50, far], [50, 46]], [0, 0, 0])[1:4] == ([0, 2], [0, 0], 2)
    assert one_point(run, camera_at(4.0), HALF, 8.0, DYADIC, [[58, 50], [50, 58.001]], [1, 1])[1:5] == ([0, -1], [0, LM.INT32_MAX], 1, 1)
    # a NaN keypoint is nobody's candidate; a taken keypoint never passes; a skipped point is not active
    assert one_point(run, camera_at(3.0), HALF, 3.0, [1.0], [[np.nan, 50], [50, 50], [50, 50]], [0, -2, 0])[1:4] == ([2, -1], [0, LM.INT32_MAX], 1)
    assert one_point(run, camera_at(3.0), HALF, 3.0, [1.0], AT, [0], skip=1) == NOT_ACTIVE
    assert one_point(run, camera_at(3.0), HALF, 3.0, [1.0], AT, [0], skip=0)[3] == 1
    # no keypoints: active with no candidates
    assert one_point(run, camera_at(3.0), HALF, 3.0, [1.0], np.zeros((0, 2)), [])[1:5] == ([-1, -1], [LM.INT32_MAX] * 2, 0, 0)
    # params: radius_scale doubles the disc, min_view_cos moves the facing limit
    assert one_point(run, camera_at(3.0), HALF, 3.0, [1.0], [[58, 50]], [0])[3] == 0
    assert one_point(run, camera_at(3.0), HALF, 3.0, [1.0], [[58, 50]], [0], params=dict(radius_scale=2.0))[3] == 1
    assert one_point(run, camera_at(3.0), HALF, 3.0, [1.0], AT, [0], params=dict(min_view_cos=0.75)) == NOT_ACTIVE


def bits(k):
    """A descriptor k bits from zero."""
    b = np.zeros(256, np.uint8)
    b[:k] = 1
    return np.packbits(b)


def filter_inputs():
    """Nine points in a row on level 1 (octaves 0 and 1 pass; vc 1: a disc of 2.5 * 2 = 5 px), each with its own keypoints:
    0: d 50 and 100 on one level  -> 50 <= 0.5 * 100 kept at ratio 0.5 (inclusive), and at 0.8
    1: d 90 and 100 on one level  -> the ratio stops it
    2: d 90 and 100 on two levels -> exempt, kept
    3: d 101 alone                -> over the ceiling
    4: d 100 alone                -> on the ceiling, kept
    5, 6 (6 px apart, the keypoint between them): both claim it at d 30 and 20 -> the smaller distance survives; 7, 8 likewise
    at d 20 each: the lower map index."""
    xs = np.array([10.0, 20, 30, 40, 50, 60, 66, 80, 86])
    z = 4.0
    pos = np.stack([(xs - 50) / 100 * z, np.zeros(9), np.full(9, z)], 1).astype(np.float32)
    desc = np.zeros((9, 32), np.uint8)
    desc[5], desc[6] = bits(30), bits(20)
    desc[7], desc[8] = bits(20), bits(20)
    kp = [(0, 50, 1), (0, 100, 1), (1, 90, 0), (1, 100, 0), (2, 90, 1), (2, 100, 0), (3, 101, 1), (4, 100, 1)]
    txy = [[xs[i], 50.0] for i, _, _ in kp] + [[(xs[5] + xs[6]) / 2, 50.0], [(xs[7] + xs[8]) / 2, 50.0]]
    t = np.stack([bits(d) for _, d, _ in kp] + [bits(0), bits(0)])
    lev = [l for _, _, l in kp] + [1, 1]
    d = pos.astype(np.float64)
    dist = np.linalg.norm(d, axis=1)
    normal = (d / dist[:, None]).astype(np.float32)
    max_dist = (dist * 2 * 0.95).astype(np.float32)          # dist * 1 < md, dist * 2 > md: lv 1
    return pos, desc, normal, max_dist, I4, K100, 100, 100, t, np.array(txy, np.float32), np.array(lev, np.int32), DYADIC


def check_filter(feat):
    a = filter_inputs()
    got = feat(*a, None, dict(lowe_ratio=0.5))
    assert got["queryIdx"].tolist() == [0, 2, 4, 6, 7] and got["trainIdx"].tolist() == [0, 4, 7, 8, 9]
    assert got["distance"].tolist() == [50.0, 90.0, 100.0, 20.0, 20.0] and (got["imgIdx"] == 0).all()
    assert feat(*a, None, None)["queryIdx"].tolist() == [0, 2, 4, 6, 7]                      # 50 <= 0.8 * 100 as well
    assert feat(*a, None, dict(lowe_ratio=0.9))["queryIdx"].tolist() == [0, 1, 2, 4, 6, 7]   # 90 <= 0.9 * 100, inclusive
    assert feat(*a, None, dict(lowe_ratio=0.49))["queryIdx"].tolist() == [2, 4, 6, 7]
    assert feat(*a, None, dict(max_hamming=101))["queryIdx"].tolist() == [0, 2, 3, 4, 6, 7]
    assert feat(*a, None, dict(max_hamming=89))["queryIdx"].tolist() == [0, 6, 7]
    skip = np.zeros(9, np.uint8)
    skip[6] = skip[7] = 1
    assert feat(*a, skip, None)["queryIdx"].tolist() == [0, 2, 4, 5, 8]


def test_levels():
    check_levels(LM.knn2)


def test_range_is_inclusive_to_the_ulp():
    check_range(LM.knn2)


def test_facing_and_the_two_radii():
    check_facing_and_radius(LM.knn2)


def test_disc_taken_keypoint_skipped_point_and_params():
    check_disc_taken_skip(LM.knn2)


def test_filter_ratio_levels_ceiling_and_one_point_per_keypoint():
    check_filter(LM.match_features)
    # the filter on hand-written rows: d0 == lowe_ratio d1 is kept, one more is not
    lev = np.array([0, 0, 1], np.int32)
    rows = lambda d0, d1, j1=1: (np.array([[0, j1]], np.int32), np.array([[d0, d1]], np.int32))
    assert len(LM.filter_local(*rows(80, 100), lev, 0.8, 100)) == 1
    assert len(LM.filter_local(*rows(81, 100), lev, 0.8, 100)) == 0
    assert len(LM.filter_local(*rows(81, 100, 2), lev, 0.8, 100)) == 1


def test_level_scales_and_the_guard_of_the_shared_scenes():
    assert LM.level_scales(2.0, 4).tolist() == [1, 2, 4, 8] and LM.level_scales(1.2, 3)[2] == np.float64(1.2) * np.float64(1.2)
    tr = LM.scene_trace(257, 2, 257)
    assert all(tr[c] > 0 for c in LM.CLAUSES), tr
