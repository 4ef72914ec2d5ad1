"""Tracking by projection on the MI355X (csrc/projection_kernels.hip, csrc/projection_host.cpp) against its numpy
transcription (tests/projection_numpy.py; known answers of its own in tests/test_projection_numpy.py), bit for bit: pixels,
the two nearest gated keypoints, their distances and the candidate counts over the lane / wave / slice / train-group
boundaries, the in-view set against mvo_map_points_in_view, the hand-computable gate, the filter, the tracking scene, the
device-pointer form, moved positions, the largest train set, every error code and the pose prediction.
tests/test_projection_sim.py runs the same functions on the emulated build."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import projection_numpy as P
from test_projection_numpy import I4, K100, border_points, filter_case, hand_gate_inputs

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 2), (63, 17), (64, 64), (65, 1037), (130, 2049), (1200, 1500)]
COLS, ROWS = 640, 480


def _to_device(a):
    import torch
    t = torch.from_numpy(np.array(a)).cuda()
    torch.cuda.synchronize()
    return t


@contextlib.contextmanager
def resident(ctx, pos, desc):
    m = ctx.map_create()
    try:
        ctx.map_upload(m, pos, desc)
        yield m
    finally:
        ctx.map_release(m)


def random_pose(rng, rot=0.08, trans=0.4):
    return P.pose(rng.uniform(-rot, rot, 3), rng.uniform(-trans, trans, 3))


def radius(nt):
    """12 px where the frame has enough keypoints to leave one or two in such a disc; a wider disc for the small sets, which
    would otherwise have none; everything for one or two keypoints."""
    return 12.0 if nt >= 1000 else (150.0 if nt > 2 else 1e4)


def map_points(rng, n, T_w_c, K):
    """Random pixels of the frame back-projected to random depths under the pose; every fifth point (i % 5 == 4) is pushed
    behind the camera or outside the frame."""
    pix = rng.uniform([1, 1], [COLS - 1, ROWS - 1], (n, 2))
    z = rng.uniform(1.0, 8.0, n)
    out = np.arange(n) % 5 == 4
    how = rng.randint(0, 3, n)
    pix[out & (how == 1), 0] += COLS
    pix[out & (how == 2), 1] -= ROWS
    z[out & (how == 0)] *= -1
    Xc = np.stack([(pix[:, 0] - K["cx"]) / K["fx"] * z, (pix[:, 1] - K["cy"]) / K["fy"] * z, z], 1)
    return (Xc @ T_w_c[:3, :3].T + T_w_c[:3, 3]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def raw_inputs(mvo, n_map, nt, kind, scaled):
    """descriptors of mvo.synth.match_inputs, map points seen under a random pose, random f32 keypoints in a 640 x 480 frame;
    with the transcription's answer.  Computed once, read-only."""
    rng = np.random.RandomState(1000 * n_map + nt + (7 if scaled else 0))
    desc, t = mvo.synth.match_inputs(kind, n_map, nt, seed=n_map + nt)
    T = random_pose(rng)
    pos = map_points(rng, n_map, T, P.FR1_K)
    txy = rng.uniform([0, 0], [COLS, ROWS], (nt, 2)).astype(np.float32)
    scale = (np.float32(1.2) ** rng.randint(0, 4, nt)).astype(np.float32) if scaled else None
    r = radius(nt)
    want = P.knn2(pos, desc, T, P.FR1_K, COLS, ROWS, t, txy, r, scale)
    for a in (pos, desc, T, t, txy, scale) + want:
        if a is not None:
            a.setflags(write=False)
    return pos, desc, T, t, txy, r, scale, want


def assert_raw_equal(got, want, what):
    for name, g, w in zip(("px", "idx", "dist", "n_candidates"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s is %s %s" % (what, name, g.dtype, g.shape)
        bad = np.nonzero((g.view(np.int32) != w.view(np.int32)).reshape(len(g), -1).any(1))[0]    # px by its bits
        assert len(bad) == 0, "%s: %s differs at %d points, first %d: %r vs %r" % (what, name, len(bad), bad[0], g[bad[0]], w[bad[0]])


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("kind", ["perturbed", "ties"])
@pytest.mark.parametrize("n_map,nt", SHAPES)
def test_raw_call_bit_exact(mvo, ctx, n_map, nt, kind, scaled):
    pos, desc, T, t, txy, r, scale, want = raw_inputs(mvo, n_map, nt, kind, scaled)
    cnt = want[3]
    if nt >= 17:                 # the case is not vacuous: some pairs pass and not all, a point with two candidates, one not in view
        assert 0 < cnt[cnt > 0].sum() < (cnt >= 0).sum() * nt and (cnt >= 2).any() and (cnt == -1).any() and (cnt >= 0).any()
    else:                        # (a single map point, in view, that sees the one or two keypoints there are)
        assert cnt.tolist() == [nt]
    with resident(ctx, pos, desc) as m:
        got = ctx.map_match_knn2_projection(m, T, P.FR1_K, COLS, ROWS, t, txy, r, scale)
        assert_raw_equal(got, want, "%d x %d %s" % (n_map, nt, kind))
        # the in-view set and its pixels are those of mvo_map_points_in_view for the same pose
        idx, px, _ = ctx.map_points_in_view(m, T, P.FR1_K, COLS, ROWS, cap=n_map)
        assert np.array_equal(idx, np.nonzero(got[3] >= 0)[0]) and px.tobytes() == got[0][idx].tobytes()


def test_ties_are_decided_by_the_train_index(mvo):
    """(the tie set does make the rule decide: some point's two nearest candidates are equally far)"""
    want = raw_inputs(mvo, 1200, 1500, "ties", True)[7]
    both = want[1][:, 1] >= 0
    tie = want[2][both, 0] == want[2][both, 1]
    assert tie.sum() > 3 and (want[1][both, 0] < want[1][both, 1])[tie].all()


def test_hand_computable_gate_borders_and_nan(ctx):
    pos, desc, t, txy = hand_gate_inputs()
    with resident(ctx, pos, desc) as m:
        px, idx, dist, cnt = ctx.map_match_knn2_projection(m, I4, K100, 100, 100, t, txy, 3.0)
        assert px.tolist() == [[50.0, 50.0]] and idx.tolist() == [[0, 2]] and dist.tolist() == [[0, 0]] and cnt.tolist() == [2]
        scale = np.array([1, 1.2, 1, 1.2], np.float32)
        assert ctx.map_match_knn2_projection(m, I4, K100, 100, 100, t, txy, 3.0, scale)[3].tolist() == [4]
        bad = txy.copy()
        bad[0, 1] = np.nan                                    # a NaN position is nobody's candidate
        got = ctx.map_match_knn2_projection(m, I4, K100, 100, 100, t, bad, 3.0)
        assert got[1].tolist() == [[2, -1]] and got[3].tolist() == [1]
        assert_raw_equal(got, P.knn2(pos, desc, I4, K100, 100, 100, t, bad, 3.0), "NaN")
    pos = border_points()
    desc = np.zeros((5, 32), np.uint8)
    t, txy = np.zeros((1, 32), np.uint8), np.array([[75, 50]], np.float32)
    with resident(ctx, pos, desc) as m:
        got = ctx.map_match_knn2_projection(m, I4, K100, 100, 100, t, txy, 1e4)
        assert got[3].tolist() == [-1, -1, -1, -1, 1]          # z < 0, z = 0, u = 0, u = cols: none in view
        assert_raw_equal(got, P.knn2(pos, desc, I4, K100, 100, 100, t, txy, 1e4), "borders")
        got = ctx.map_match_knn2_projection(m, I4, K100, 100, 100, t[:0], txy[:0], 3.0)
        assert got[3].tolist() == [-1, -1, -1, -1, 0] and got[0][4].tolist() == [75.0, 50.0]
        assert_raw_equal(got, P.knn2(pos, desc, I4, K100, 100, 100, t[:0], txy[:0], 3.0), "no keypoints")


def scene_call(ctx, m, s, T, max_px, **kw):
    return ctx.map_match_features_projection(m, T, s["K"], s["cols"], s["rows"], s["t"], s["txy"], max_px, 0.8, 64, **kw)


def test_tracking_scene_every_partner_found(ctx):
    s = P.tracking_scene()
    b = (s["K"], s["cols"], s["rows"], s["t"], s["txy"])
    with resident(ctx, s["pos"], s["desc"]) as m:
        got, px, in_view = scene_call(ctx, m, s, s["T_pred"], 6.0)
        assert got.tobytes() == P.match_features(s["pos"], s["desc"], s["T_pred"], *b, 6.0, 0.8, 64).tobytes()
        assert P.scene_score(s, got) == (343, 343, 0)
        u, v, want_view = P.project_map(s["pos"], s["T_pred"], s["K"], s["cols"], s["rows"])
        assert np.array_equal(in_view, want_view) and in_view.sum() == 348
        assert px[in_view].tobytes() == np.stack([u, v], 1)[in_view].tobytes() and (px[~in_view] == 0).all()
        # under the keyframe's pose, as the reference projects: fewer than half at either radius
        for r, score in ((6.0, (18, 17, 1)), (50.0, (343, 109, 234))):
            got = scene_call(ctx, m, s, s["T_key"], r)[0]
            assert got.tobytes() == P.match_features(s["pos"], s["desc"], s["T_key"], *b, r, 0.8, 64).tobytes()
            assert P.scene_score(s, got) == score
        # the global search with the ratio test (matchFeatures method 2 on the points in view) finds no partner
        idx, _, _ = ctx.map_points_in_view(m, s["T_key"], s["K"], s["cols"], s["rows"], cap=len(s["pos"]))
    blind = ctx.match_features(s["desc"][idx], s["t"], method=2, lowe_ratio=0.8)
    blind["queryIdx"] = idx[blind["queryIdx"]]
    n, partners, twins = P.scene_score(s, blind)
    assert partners == 0 and twins == n and n > 300


def test_filter_ceiling_ratio_single_candidate_and_one_query_per_train(ctx):
    pos, desc, t, txy, K, cols, rows = filter_case()
    with resident(ctx, pos, desc) as m:
        got = ctx.map_match_features_projection(m, I4, K, cols, rows, t, txy, 3.0, 0.8, 64)[0]
        assert got["queryIdx"].tolist() == [0, 2, 5, 7] and got["trainIdx"].tolist() == [0, 1, 6, 7]
        assert got["distance"].tolist() == [3.0, 64.0, 39.0, 5.0] and (got["imgIdx"] == 0).all()
        for ratio, ceiling, queries in ((0.8, 64, [0, 2, 5, 7]), (1.0, 64, [0, 2, 4, 5, 7]), (0.8, 256, [0, 2, 3, 5, 7, 8])):
            got = ctx.map_match_features_projection(m, I4, K, cols, rows, t, txy, 3.0, ratio, ceiling)[0]
            assert got["queryIdx"].tolist() == queries
            assert got.tobytes() == P.match_features(pos, desc, I4, K, cols, rows, t, txy, 3.0, ratio, ceiling).tobytes()


def test_device_pointer_form_equals_the_host_form(mvo, ctx):
    for n_map, nt, kind, scaled in ((65, 1037, "perturbed", True), (130, 2049, "ties", False)):
        pos, desc, T, t, txy, r, scale, want = raw_inputs(mvo, n_map, nt, kind, scaled)
        d_t = _to_device(t)
        with resident(ctx, pos, desc) as m:
            got = ctx.map_match_knn2_projection_dev(m, T, P.FR1_K, COLS, ROWS, d_t.data_ptr(), txy, r, scale)
        assert_raw_equal(got, want, "dev form %d x %d" % (n_map, nt))


def test_moved_positions_are_seen_by_the_next_call(mvo, ctx):
    pos, desc, T, t, txy, r, scale, want = raw_inputs(mvo, 130, 2049, "perturbed", False)
    moved = pos.copy()
    moved[40:100] += np.float32(0.05)
    with resident(ctx, pos, desc) as m:
        assert_raw_equal(ctx.map_match_knn2_projection(m, T, P.FR1_K, COLS, ROWS, t, txy, r), want, "before")
        ctx.map_update_positions(m, moved[40:100], first=40)
        got = ctx.map_match_knn2_projection(m, T, P.FR1_K, COLS, ROWS, t, txy, r)
    after = P.knn2(moved, desc, T, P.FR1_K, COLS, ROWS, t, txy, r)
    assert not np.array_equal(after[0], want[0])
    assert_raw_equal(got, after, "after map_update_positions")


def test_the_largest_train_set(ctx):
    """nt = 65535, the last size the 16-bit index holds: the last keypoint is some point's nearest candidate."""
    rng = np.random.RandomState(4)
    nt = 65535
    t = rng.randint(0, 256, (nt, 32)).astype(np.uint8)
    txy = rng.uniform([5, 5], [COLS - 5, ROWS - 5], (nt, 2)).astype(np.float32)
    pick = [nt - 1, 40000, 0]
    z = np.array([2.0, 3.0, 5.0])
    K = P.FR1_K
    pos = np.stack([(txy[pick, 0] - K["cx"]) / K["fx"] * z, (txy[pick, 1] - K["cy"]) / K["fy"] * z, z], 1).astype(np.float32)
    desc = t[pick].copy()
    with resident(ctx, pos, desc) as m:
        got = ctx.map_match_knn2_projection(m, I4, K, COLS, ROWS, t, txy, 0.25)
    assert got[1][:, 0].tolist() == pick and got[2][:, 0].tolist() == [0, 0, 0]
    assert_raw_equal(got, P.knn2(pos, desc, I4, K, COLS, ROWS, t, txy, 0.25), "65535 keypoints")


def test_partial_scratch_regrows_between_calls(mvo):
    """One context of its own, six raw calls: 64 x 300 (two train groups, so the arrival counters are used), 4200 x 300
    (past the 4096 floor: the partial scratch is freed and reallocated for 6300, its counters zeroed again), 6400 x 300 (past
    6300: once more), 64 x 4200 and 64 x 6400 (the keypoint staging the same way), 64 x 300 again."""
    c = mvo.Context(0)
    try:
        for n_map, nt in ((64, 300), (4200, 300), (6400, 300), (64, 4200), (64, 6400), (64, 300)):
            pos, desc, T, t, txy, r, scale, want = raw_inputs(mvo, n_map, nt, "perturbed", True)
            assert (want[3] > 0).any() and (want[3] == -1).any()
            with resident(c, pos, desc) as m:
                assert_raw_equal(c.map_match_knn2_projection(m, T, P.FR1_K, COLS, ROWS, t, txy, r, scale), want, "%d x %d" % (n_map, nt))
    finally:
        c.close()


def test_errors(mvo, ctx):
    pos, desc, T, t, txy, r, scale, want = raw_inputs(mvo, 63, 17, "perturbed", True)
    lib, h, K = ctx.lib, ctx.h, P.FR1_K

    def code(fn, *a, **kw):
        with pytest.raises(mvo.MvoError) as e:
            fn(*a, **kw)
        return e.value.code

    with resident(ctx, pos, desc) as m:
        def raw(m_, T_, t_, txy_, nt, idx=True, dist=True):
            p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
            idx_, dist_ = np.zeros((63, 2), np.int32), np.zeros((63, 2), np.int32)
            T_ = None if T_ is None else np.ascontiguousarray(T_, np.float64)
            k = [C.c_double(K[name]) for name in ("fx", "fy", "cx", "cy")]
            return lib.mvo_map_match_knn2_projection(h, m_, p(T_), *k, COLS, ROWS, p(t_), p(txy_), None, nt, C.c_double(2.0), None,
                                                     p(idx_) if idx else None, p(dist_) if dist else None, None)

        # a null pointer with a positive count, a null map
        assert raw(m, T, None, txy, 17) == mvo.MVO_ERR_INVALID
        assert raw(m, T, t, None, 17) == mvo.MVO_ERR_INVALID
        assert raw(m, T, t, txy, 17, idx=False) == mvo.MVO_ERR_INVALID
        assert raw(m, T, t, txy, 17, dist=False) == mvo.MVO_ERR_INVALID
        assert raw(m, None, t, txy, 17) == mvo.MVO_ERR_INVALID
        assert raw(None, T, t, txy, 17) == mvo.MVO_ERR_INVALID
        assert raw(m, T, t, txy, -1) == mvo.MVO_ERR_INVALID
        assert raw(m, T, t, txy, 17) == mvo.MVO_OK             # (optional outputs may be null)
        call = lambda T_=T, K_=K, cols=COLS, rows=ROWS, r_=r, s_=scale: ctx.map_match_knn2_projection(m, T_, K_, cols, rows, t, txy, r_, s_)
        # a singular or non-finite pose
        singular = np.array(T)
        singular[:3, :3] = 0
        assert code(call, T_=singular) == mvo.MVO_ERR_INVALID
        for bad in (np.nan, np.inf):
            Tb = np.array(T)
            Tb[1, 3] = bad
            assert code(call, T_=Tb) == mvo.MVO_ERR_INVALID
        # the intrinsics, the frame, the radius, the scales
        assert code(call, K_=dict(K, fx=0.0)) == mvo.MVO_ERR_INVALID
        assert code(call, K_=dict(K, fy=0.0)) == mvo.MVO_ERR_INVALID
        assert code(call, cols=0) == mvo.MVO_ERR_INVALID
        assert code(call, rows=-480) == mvo.MVO_ERR_INVALID
        assert code(call, r_=-0.5) == mvo.MVO_ERR_INVALID
        assert code(call, r_=float("nan")) == mvo.MVO_ERR_INVALID
        for bad in (-1.0, np.nan, np.inf):
            sb = np.array(scale)
            sb[5] = bad
            assert code(call, s_=sb) == mvo.MVO_ERR_INVALID
        d_t = _to_device(t)
        dev = lambda d, r_: ctx.map_match_knn2_projection_dev(m, T, K, COLS, ROWS, d, txy, r_, scale)
        assert code(dev, d_t.data_ptr(), -1.0) == mvo.MVO_ERR_INVALID
        assert code(dev, None, r) == mvo.MVO_ERR_INVALID
        def feat(r_=r, **kw):
            return ctx.map_match_features_projection(m, T, K, COLS, ROWS, t, txy, r_, 0.8, 256, scale, **kw)

        assert code(feat, r_=-1.0) == mvo.MVO_ERR_INVALID
        # capacity: the output buffer (with the count reported), the 16-bit train index
        n_all = len(feat()[0])
        assert n_all > 1 and code(feat, cap=n_all - 1) == mvo.MVO_ERR_CAPACITY and len(feat(cap=n_all)[0]) == n_all
        out, cnt = np.zeros(1, mvo.DMATCH_DTYPE), C.c_int(-5)
        k = [C.c_double(K[name]) for name in ("fx", "fy", "cx", "cy")]
        p = lambda a: C.c_void_p(a.ctypes.data)
        Tc = np.ascontiguousarray(T, np.float64)
        assert lib.mvo_map_match_features_projection(h, m, p(Tc), *k, COLS, ROWS, p(t), p(txy), p(scale), 17, C.c_double(r), C.c_double(0.8),
                                                     256, None, None, p(out), 1, C.byref(cnt)) == mvo.MVO_ERR_CAPACITY
        assert cnt.value == n_all
        big, bigxy = np.zeros((65536, 32), np.uint8), np.zeros((65536, 2), np.float32)
        assert code(ctx.map_match_knn2_projection, m, T, K, COLS, ROWS, big, bigxy, r) == mvo.MVO_ERR_CAPACITY
        assert code(ctx.map_match_features_projection, m, T, K, COLS, ROWS, big, bigxy, r, 0.8, 64) == mvo.MVO_ERR_CAPACITY
        # no keypoints: succeeds, in view 0, the others -1
        px, idx, dist, cnt = ctx.map_match_knn2_projection(m, T, K, COLS, ROWS, t[:0], txy[:0], r)
        assert (idx == -1).all() and (dist == P.INT32_MAX).all() and np.array_equal(cnt, np.where(want[3] >= 0, 0, -1))
        assert px.tobytes() == want[0].tobytes()
        assert len(ctx.map_match_features_projection(m, T, K, COLS, ROWS, t[:0], txy[:0], r, 0.8, 64)[0]) == 0
        # the context still works after all of them
        assert_raw_equal(ctx.map_match_knn2_projection(m, T, K, COLS, ROWS, t, txy, r, scale), want, "after the errors")
    # an empty map succeeds
    e = ctx.map_create()
    try:
        got = ctx.map_match_knn2_projection(e, T, K, COLS, ROWS, t, txy, r)
        assert got[0].shape == (0, 2) and got[3].shape == (0,)
        assert len(ctx.map_match_features_projection(e, T, K, COLS, ROWS, t, txy, r, 0.8, 64)[0]) == 0
    finally:
        ctx.map_release(e)


def test_predict_pose(mvo):
    rng = np.random.RandomState(21)
    for _ in range(8):
        A, B = random_pose(rng, 0.4, 2.0), random_pose(rng, 0.4, 2.0)
        got = mvo.predict_pose(A, B)
        assert got.tobytes() == P.predict_pose(A, B).tobytes()                      # the declared order, bit for bit
        want = B @ (np.linalg.inv(A) @ B)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        assert np.array_equal(mvo.predict_pose(None, B), B)
    M, T0 = P.pose([0.02, -0.03, 0.05], [0.1, 0.02, -0.04]), P.pose([0.3, 0.1, -0.2], [1.0, -0.5, 0.3])
    assert np.abs(mvo.predict_pose(T0, T0 @ M) - T0 @ M @ M).max() < 1e-9
    singular = np.array(A)
    singular[:3, :3] = 0
    with pytest.raises(mvo.MvoError) as e:
        mvo.predict_pose(singular, B)
    assert e.value.code == mvo.MVO_ERR_INVALID
