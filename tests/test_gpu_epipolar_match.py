"""The pose-guided matcher on the MI355X (csrc/epipolar_kernels.hip, csrc/epipolar_host.cpp) against its numpy transcription
(tests/epipolar_numpy.py; known answers of its own in tests/test_epipolar_numpy.py), bit for bit: the raw 2-NN with the
candidate counts over the lane / wave / slice / workgroup boundaries, the exact gate, the filter, the two-view scene, the
device-pointer form, every error code and F from poses.  tests/test_epipolar_sim.py runs the same functions on the emulated
build."""
import ctypes as C
import functools

import numpy as np
import pytest

import epipolar_numpy as E
from test_epipolar_numpy import F_ROW, exact_gate_inputs

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 2), (63, 17), (64, 64), (65, 1037), (130, 2049), (1200, 1500)]


def _to_device(a):
    import torch
    t = torch.from_numpy(np.array(a)).cuda()
    torch.cuda.synchronize()
    return t


def random_pose(rng, rot=0.08, trans=0.4):
    T = np.eye(4)
    T[:3, :3] = E.rodrigues(rng.uniform(-rot, rot, 3))
    T[:3, 3] = rng.uniform(-trans, trans, 3)
    return T


def line_tolerance(nt):
    """2 px where the train set is large enough to leave a dozen candidates in the band; wider bands for the small sets, which
    would otherwise have none (a 4 px band holds about 1 % of a 640 x 480 frame), everything for one or two trains."""
    return 2.0 if nt >= 1000 else (60.0 if nt > 2 else 1e4)


@functools.lru_cache(maxsize=None)
def raw_inputs(mvo, nq, nt, kind, scaled):
    """descriptors of mvo.synth.match_inputs, random f32 positions in a 640 x 480 frame, F of two random poses through the
    library; with the transcription's answer.  Computed once, read-only."""
    rng = np.random.RandomState(1000 * nq + nt + (7 if scaled else 0))
    q, t = mvo.synth.match_inputs(kind, nq, nt, seed=nq + nt)
    qxy = rng.uniform([0, 0], [640, 480], (nq, 2)).astype(np.float32)
    txy = rng.uniform([0, 0], [640, 480], (nt, 2)).astype(np.float32)
    F = mvo.fundamental_from_poses(random_pose(rng), random_pose(rng), E.FR1_K)
    scale = (np.float32(1.2) ** rng.randint(0, 4, nt)).astype(np.float32) if scaled else None
    px = line_tolerance(nt)
    want = E.knn2(q, qxy, t, txy, F, px, scale)
    for a in (q, t, qxy, txy, F, scale) + want:
        if a is not None:
            a.setflags(write=False)
    return q, qxy, t, txy, F, px, scale, want


def assert_raw_equal(got, want, what):
    for name, g, w in zip(("idx", "dist", "n_candidates"), got, want):
        bad = np.nonzero((g != w).reshape(len(g), -1).any(1))[0]
        assert len(bad) == 0, "%s: %s differs at %d queries, first %d: %r vs %r" % (what, name, len(bad), bad[0], g[bad[0]], w[bad[0]])


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("kind", ["perturbed", "ties"])
@pytest.mark.parametrize("nq,nt", SHAPES)
def test_raw_call_bit_exact(mvo, ctx, nq, nt, kind, scaled):
    q, qxy, t, txy, F, px, scale, want = raw_inputs(mvo, nq, nt, kind, scaled)
    if nt >= 17:                                             # the case is not vacuous: the gate passes some pairs and not all
        assert 0 < want[2].sum() < nq * nt and (want[2] >= 2).any()
    else:
        assert (want[2] == nt).all()
    got = ctx.match_knn2_epipolar(q, qxy, t, txy, F, px, scale)
    assert_raw_equal(got, want, "%d x %d %s" % (nq, nt, kind))
    assert all(g.dtype == np.int32 for g in got)


def test_ties_are_decided_by_the_train_index(mvo):
    """(the tie set does make the rule decide: some query's two nearest candidates are equally far)"""
    want = raw_inputs(mvo, 1200, 1500, "ties", False)[7]
    both = want[0][:, 1] >= 0
    assert (want[1][both, 0] == want[1][both, 1]).sum() > 10
    assert (want[0][both, 0] < want[0][both, 1])[want[1][both, 0] == want[1][both, 1]].all()


def test_exact_gate_and_zero_f(ctx):
    q, qxy, t, txy = exact_gate_inputs()
    idx, dist, cnt = ctx.match_knn2_epipolar(q, qxy, t, txy, F_ROW, 2.0)
    assert cnt.tolist() == [3, 1, 0]                          # inclusive at 2 px, the f32 neighbours outside fall out
    assert idx.tolist() == [[0, 1], [5, -1], [-1, -1]]
    assert dist.tolist() == [[0, 0], [0, E.INT32_MAX], [E.INT32_MAX, E.INT32_MAX]]
    got = ctx.match_knn2_epipolar(q, qxy, t, txy, np.zeros((3, 3)), 2.0)
    assert (got[2] == 0).all() and (got[0] == -1).all() and (got[1] == E.INT32_MAX).all()
    assert_raw_equal(got, E.knn2(q, qxy, t, txy, np.zeros(9), 2.0), "F = 0")
    bad = txy.copy()
    bad[0, 1] = np.nan                                        # a NaN position is nobody's candidate
    assert_raw_equal(ctx.match_knn2_epipolar(q, qxy, t, bad, F_ROW, 2.0), E.knn2(q, qxy, t, bad, F_ROW, 2.0), "NaN")
    scale = np.array([1, 1, 1.2, 1.44, 1.44, 1], np.float32)
    far = txy.copy()
    far[:, 1] = [100, 102.25, 102.25, 97.25, 96, 50.5]
    got = ctx.match_knn2_epipolar(q, qxy, t, far, F_ROW, 2.0, scale)
    assert got[2].tolist() == [3, 1, 0] and got[0][0].tolist() == [0, 2]
    assert_raw_equal(got, E.knn2(q, qxy, t, far, F_ROW, 2.0, scale), "scaled")


def test_two_view_scene_every_partner_found(ctx):
    s = E.two_view_scene()
    want = E.match_features(s["d1"], s["xy1"], s["d2"], s["xy2"], s["F"], 2.0, 0.8, 64)
    got = ctx.match_features_epipolar(s["d1"], s["xy1"], s["d2"], s["xy2"], s["F"], 2.0, 0.8, 64)
    assert got.tobytes() == want.tobytes()
    assert len(got) == 280 and (s["partner"][got["queryIdx"]] == got["trainIdx"]).sum() == 280
    # the global search with the ratio test takes the twin every time
    blind = ctx.match_features(s["d1"], s["d2"], method=2, lowe_ratio=0.8)
    assert len(blind) == 280 and (s["partner"][blind["queryIdx"]] == blind["trainIdx"]).sum() == 0
    assert (s["twin"][blind["queryIdx"]] == blind["trainIdx"]).sum() == 280


def flip(d, lo, n):
    bits = np.unpackbits(d)
    bits[lo:lo + n] ^= 1
    return np.packbits(bits)


def filter_case():
    """Rows of the line y = v, 10 px apart: a query sees the trains of its row only.  (row: queries -> trains at distance)"""
    base = np.random.RandomState(9).randint(0, 256, (8, 32)).astype(np.uint8)
    q, qy, t, ty = [], [], [], []

    def row(y, queries, trains):
        for d in queries:
            q.append(d), qy.append(y)
        for d in trains:
            t.append(d), ty.append(y)

    row(10, [flip(base[0], 0, 3), flip(base[0], 10, 3)], [base[0]])            # q0, q1 claim t0 at distance 3: q0 survives
    row(20, [base[1]], [flip(base[1], 0, 64)])                                 # q2: single candidate at the ceiling: kept
    row(30, [base[2]], [flip(base[2], 0, 65)])                                 # q3: single candidate above it: dropped
    row(40, [base[3]], [flip(base[3], 0, 40), flip(base[3], 0, 50)])           # q4: 40 < 0.8 * 50 is false: dropped
    row(50, [base[4]], [flip(base[4], 0, 50), flip(base[4], 0, 39)])           # q5: 39 < 40: kept, train 6
    row(60, [flip(base[5], 0, 12), flip(base[5], 20, 5)], [base[5]])           # q6, q7 claim t7: the nearer q7 survives
    row(70, [base[6]], [flip(base[6], 0, 70), flip(base[6], 0, 200)])          # q8: passes the ratio, fails the ceiling
    xy1 = np.stack([np.arange(len(q)) * 7.0, qy], 1).astype(np.float32)
    xy2 = np.stack([600.0 - np.arange(len(t)) * 11.0, ty], 1).astype(np.float32)
    return np.array(q), xy1, np.array(t), xy2


def test_filter_ceiling_ratio_single_candidate_and_one_query_per_train(ctx):
    d1, xy1, d2, xy2 = filter_case()
    got = ctx.match_features_epipolar(d1, xy1, d2, xy2, F_ROW, 2.0, 0.8, 64)
    assert got["queryIdx"].tolist() == [0, 2, 5, 7] and got["trainIdx"].tolist() == [0, 1, 6, 7]
    assert got["distance"].tolist() == [3.0, 64.0, 39.0, 5.0] and (got["imgIdx"] == 0).all()
    assert got.tobytes() == E.match_features(d1, xy1, d2, xy2, F_ROW, 2.0, 0.8, 64).tobytes()
    # the ceiling alone (ratio 1.0 keeps q4 as well), the ratio alone (ceiling 256 keeps q3 and q8)
    for ratio, ceiling, queries in ((1.0, 64, [0, 2, 4, 5, 7]), (0.8, 256, [0, 2, 3, 5, 7, 8])):
        got = ctx.match_features_epipolar(d1, xy1, d2, xy2, F_ROW, 2.0, ratio, ceiling)
        assert got["queryIdx"].tolist() == queries
        assert got.tobytes() == E.match_features(d1, xy1, d2, xy2, F_ROW, 2.0, ratio, ceiling).tobytes()


def test_device_pointer_form_equals_the_host_form(mvo, ctx):
    for nq, nt, kind, scaled in ((65, 1037, "perturbed", True), (130, 2049, "ties", False)):
        q, qxy, t, txy, F, px, scale, want = raw_inputs(mvo, nq, nt, kind, scaled)
        d_q, d_t = _to_device(q), _to_device(t)
        got = ctx.match_knn2_epipolar_dev(d_q.data_ptr(), qxy, d_t.data_ptr(), txy, F, px, scale)
        assert_raw_equal(got, ctx.match_knn2_epipolar(q, qxy, t, txy, F, px, scale), "dev form %d x %d" % (nq, nt))
        assert_raw_equal(got, want, "dev form %d x %d" % (nq, nt))


def test_errors(mvo, ctx):
    q, qxy, t, txy, F, px, scale, want = raw_inputs(mvo, 63, 17, "perturbed", True)
    lib, h = ctx.lib, ctx.h

    def code(fn, *a, **kw):
        with pytest.raises(mvo.MvoError) as e:
            fn(*a, **kw)
        return e.value.code

    def raw(q_, qxy_, nq, t_, txy_, nt, F_=F, idx=True):
        p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        idx_, dist_ = np.zeros((max(nq, 1), 2), np.int32), np.zeros((max(nq, 1), 2), np.int32)
        return lib.mvo_match_knn2_epipolar(h, p(q_), p(qxy_), nq, p(t_), p(txy_), None, nt, p(np.ascontiguousarray(F_, np.float64)),
                                           C.c_double(2.0), p(idx_) if idx else None, p(dist_), None)

    # a null pointer with a positive count
    assert raw(None, qxy, 63, t, txy, 17) == mvo.MVO_ERR_INVALID
    assert raw(q, None, 63, t, txy, 17) == mvo.MVO_ERR_INVALID
    assert raw(q, qxy, 63, None, txy, 17) == mvo.MVO_ERR_INVALID
    assert raw(q, qxy, 63, t, None, 17) == mvo.MVO_ERR_INVALID
    assert raw(q, qxy, 63, t, txy, 17, idx=False) == mvo.MVO_ERR_INVALID
    assert raw(q, qxy, -1, t, txy, 17) == mvo.MVO_ERR_INVALID
    assert raw(q, qxy, 63, t, txy, 17) == mvo.MVO_OK
    # F, the tolerance, the scales
    for bad in (np.nan, np.inf):
        Fb = np.array(F)
        Fb[1, 2] = bad
        assert code(ctx.match_knn2_epipolar, q, qxy, t, txy, Fb, px) == mvo.MVO_ERR_INVALID
    assert code(ctx.match_knn2_epipolar, q, qxy, t, txy, F, -0.5) == mvo.MVO_ERR_INVALID
    assert code(ctx.match_knn2_epipolar, q, qxy, t, txy, F, float("nan")) == mvo.MVO_ERR_INVALID
    for bad in (-1.0, np.nan, np.inf):
        sb = np.array(scale)
        sb[5] = bad
        assert code(ctx.match_knn2_epipolar, q, qxy, t, txy, F, px, sb) == mvo.MVO_ERR_INVALID
    d_q, d_t = _to_device(q), _to_device(t)
    assert code(ctx.match_knn2_epipolar_dev, d_q.data_ptr(), qxy, d_t.data_ptr(), txy, F, -1.0) == mvo.MVO_ERR_INVALID
    assert code(ctx.match_knn2_epipolar_dev, None, qxy, d_t.data_ptr(), txy, F, px) == mvo.MVO_ERR_INVALID
    assert code(ctx.match_features_epipolar, q, qxy, t, txy, F, -1.0, 0.8, 64) == mvo.MVO_ERR_INVALID
    # capacity: the output buffer, the 16-bit train index
    s = E.two_view_scene()
    assert code(ctx.match_features_epipolar, s["d1"], s["xy1"], s["d2"], s["xy2"], s["F"], 2.0, 0.8, 64, cap=279) == mvo.MVO_ERR_CAPACITY
    assert len(ctx.match_features_epipolar(s["d1"], s["xy1"], s["d2"], s["xy2"], s["F"], 2.0, 0.8, 64, cap=280)) == 280
    big, bigxy = np.zeros((65536, 32), np.uint8), np.zeros((65536, 2), np.float32)
    assert code(ctx.match_knn2_epipolar, q, qxy, big, bigxy, F, px) == mvo.MVO_ERR_CAPACITY
    assert code(ctx.match_features_epipolar, q, qxy, big, bigxy, F, px, 0.8, 64) == mvo.MVO_ERR_CAPACITY
    # empty sets succeed
    idx, dist, cnt = ctx.match_knn2_epipolar(q, qxy, t[:0], txy[:0], F, px)
    assert (idx == -1).all() and (dist == E.INT32_MAX).all() and (cnt == 0).all() and idx.shape == (63, 2)
    assert ctx.match_knn2_epipolar(q[:0], qxy[:0], t, txy, F, px)[0].shape == (0, 2)
    assert len(ctx.match_features_epipolar(q, qxy, t[:0], txy[:0], F, px, 0.8, 64)) == 0
    assert len(ctx.match_features_epipolar(q[:0], qxy[:0], t, txy, F, px, 0.8, 64)) == 0
    # the context still works after all of them
    assert_raw_equal(ctx.match_knn2_epipolar(q, qxy, t, txy, F, px, scale), want, "after the errors")


def test_the_largest_train_set(mvo, ctx):
    """nt = 65535, the last size the 16-bit index holds: the last train is some query's nearest candidate."""
    rng = np.random.RandomState(4)
    nt = 65535
    t = rng.randint(0, 256, (nt, 32)).astype(np.uint8)
    txy = rng.uniform([0, 0], [640, 480], (nt, 2)).astype(np.float32)
    q = t[[nt - 1, 40000, 0]].copy()
    qxy = np.stack([[1.0, 2.0, 3.0], txy[[nt - 1, 40000, 0], 1]], 1).astype(np.float32)
    idx, dist, cnt = ctx.match_knn2_epipolar(q, qxy, t, txy, F_ROW, 0.25)
    assert idx[:, 0].tolist() == [nt - 1, 40000, 0] and dist[:, 0].tolist() == [0, 0, 0]
    assert_raw_equal((idx, dist, cnt), E.knn2(q, qxy, t, txy, F_ROW, 0.25), "65535 trains")


def test_partial_scratch_regrows_between_calls(mvo):
    """One context of its own, six raw calls: 64 x 300 (two train groups, so the arrival counters are used), 4200 x 300
    (past the 4096 floor: the partial scratch and the query staging are freed and reallocated for 6300, the counters zeroed
    again), 6400 x 300 (past 6300: once more), 64 x 4200 and 64 x 6400 (the train staging the same way), 64 x 300 again."""
    c = mvo.Context(0)
    try:
        for nq, nt in ((64, 300), (4200, 300), (6400, 300), (64, 4200), (64, 6400), (64, 300)):
            q, qxy, t, txy, F, px, scale, want = raw_inputs(mvo, nq, nt, "perturbed", True)
            assert 0 < want[2].sum() < nq * nt
            assert_raw_equal(c.match_knn2_epipolar(q, qxy, t, txy, F, px, scale), want, "%d x %d" % (nq, nt))
    finally:
        c.close()


def test_fundamental_from_poses(mvo):
    rng = np.random.RandomState(21)
    for k in range(8):
        T1, T2 = random_pose(rng, 0.3, 1.0), random_pose(rng, 0.3, 1.0)
        F = mvo.fundamental_from_poses(T1, T2, E.FR1_K)
        want = E.fundamental_from_poses(T1, T2, E.FR1_K)
        assert np.abs(F - want).max() <= 1e-12 * np.abs(want).max()
        X = rng.uniform([-2, -1.5, 4], [2, 1.5, 9], (40, 3))
        p1, _ = E.project(T1, E.FR1_K, X)
        p2, _ = E.project(T2, E.FR1_K, X)
        Fn = F / np.linalg.norm(F)
        assert np.abs(np.einsum("ni,ij,nj->n", np.c_[p2, np.ones(40)], Fn, np.c_[p1, np.ones(40)])).max() < 1e-9
    assert np.array_equal(mvo.fundamental_from_poses(T1, T2, np.array([[517.3, 0, 325.1], [0, 516.5, 249.7], [0, 0, 1]])), F)
    singular = np.array(T1)
    singular[:3, :3] = 0
    for a in ((singular, T2, E.FR1_K), (T1, singular, E.FR1_K), (T1, T2, dict(E.FR1_K, fx=0.0)), (T1, T2, dict(E.FR1_K, fy=0.0))):
        with pytest.raises(mvo.MvoError) as e:
            mvo.fundamental_from_poses(*a)
        assert e.value.code == mvo.MVO_ERR_INVALID
