"""Tracking the local map on the MI355X (csrc/local_map_kernels.hip, csrc/local_map_host.cpp) against its numpy transcription
(tests/local_map_numpy.py; known answers of its own in tests/test_local_map_numpy.py), bit for bit: pixels, the two nearest
passing keypoints, their distances, the candidate counts, the predicted levels and the viewing cosines over the lane / wave /
slice / train-group boundaries and 1, 2 and 8 levels; the matches behind ORB-SLAM's acceptance rule; the hand-worked cases; a
wave without an active point, a smaller map on the same ctx, a re-upload that invalidates the view data, other parameters,
the device-pointer form and every error code with sentinel fills.  tests/test_local_map_sim.py runs the same functions on the
emulated build."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import local_map_numpy as LM
import test_local_map_numpy as H

pytestmark = pytest.mark.gpu

MAP_SIZES = [1, 63, 64, 65, 257, 700]
NTS = [0, 1, 2, 255, 256, 257, 1100]          # 1100: more than one train group, so the partials and the arrival counters
LEVELS = [1, 2, 8]
OTHER = (("lowe_ratio", 0.9), ("max_hamming", 64), ("min_view_cos", 0.3), ("near_cos", 0.99), ("radius_far", 6.0), ("radius_near", 3.0),
         ("radius_scale", 1.5))
NAMES = ("px", "idx", "dist", "n_candidates", "level", "view_cos")


def _to_device(a):
    import torch
    t = torch.from_numpy(np.array(a)).cuda()
    torch.cuda.synchronize()
    return t


@contextlib.contextmanager
def resident(ctx, pos, desc, normal=None, max_dist=None):
    m = ctx.map_create()
    try:
        ctx.map_upload(m, pos, desc)
        if normal is not None:
            ctx.map_upload_view(m, normal, max_dist)
        yield m
    finally:
        ctx.map_release(m)


def scene_map(ctx, s):
    return resident(ctx, s["pos"], s["desc"], s["normal"], s["max_dist"])


def assert_raw_equal(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s is %s %s" % (what, name, g.dtype, g.shape)
        bad = np.nonzero((g.view(np.uint32) != w.view(np.uint32)).reshape(len(g), -1).any(1))[0]    # floats by their bits
        assert len(bad) == 0, "%s: %s differs at %d points, first %d: %r vs %r" % (what, name, len(bad), bad[0], g[bad[0]], w[bad[0]])


def lib_raw(ctx):
    """The raw call with the signature of the transcription's knn2: a resident map made for the call."""
    def run(pos, desc, normal, max_dist, T, K, cols, rows, t, txy, t_level, ls, skip=None, params=None):
        with resident(ctx, pos, desc, normal, max_dist) as m:
            return ctx.map_match_knn2_local(m, T, K, cols, rows, t, txy, t_level, ls, skip, params)
    return run


def lib_features(ctx):
    def run(pos, desc, normal, max_dist, T, K, cols, rows, t, txy, t_level, ls, skip=None, params=None):
        with resident(ctx, pos, desc, normal, max_dist) as m:
            return ctx.map_match_features_local(m, T, K, cols, rows, t, txy, t_level, ls, skip, params)[0]
    return run


def check_guard(n_map, L, nt):
    """The scene makes every clause decide: each stops (the level exemption: keeps) at least one pair that every other clause
    lets through.  With one level every keypoint sits on the predicted one, so the window and the exemption have nothing to
    decide there.  Small scenes cannot hold all nine; the guard is held from 257 points and 255 keypoints on."""
    tr = LM.scene_trace(n_map, L, nt)
    for c in LM.CLAUSES:
        if L == 1 and c in ("level window", "level exemption"):
            assert tr[c] == 0
        else:
            assert tr[c] > 0, "scene %d x %d, %d levels: no pair decided by '%s' alone: %r" % (n_map, nt, L, c, tr)


@pytest.mark.parametrize("L", LEVELS)
@pytest.mark.parametrize("n_map", MAP_SIZES)
def test_scenes_bit_exact(ctx, n_map, L):
    s = LM.scene(n_map, L)
    with scene_map(ctx, s) as m:
        for nt in NTS:
            raw, feat = LM.scene_answer(n_map, L, nt)
            if n_map >= 257 and nt >= 255:
                check_guard(n_map, L, nt)
                assert (raw[3] == -1).any() and (raw[3] == 0).any() and (raw[3] >= 2).any()
            what = "%d points, %d keypoints, %d levels" % (n_map, nt, L)
            assert_raw_equal(ctx.map_match_knn2_local(m, *LM.scene_args(s, nt), s["skip"]), raw, what)
            got, px, lv = ctx.map_match_features_local(m, *LM.scene_args(s, nt), s["skip"])
            assert got.tobytes() == feat.tobytes(), what
            assert px.tobytes() == raw[0].tobytes() and lv.tobytes() == raw[4].tobytes()


def test_hand_worked_cases(ctx):
    H.check_levels(lib_raw(ctx))
    H.check_range(lib_raw(ctx))
    H.check_facing_and_radius(lib_raw(ctx))
    H.check_disc_taken_skip(lib_raw(ctx))
    H.check_filter(lib_features(ctx))


def test_idle_wave_other_params_and_the_device_pointer_form(ctx):
    s = LM.scene(257, 8)
    a = LM.scene_args(s, 1100)
    m4 = (s["pos"], s["desc"], s["normal"], s["max_dist"])
    skip = np.array(s["skip"])
    skip[64:128] = 1                                  # the second wave of the first workgroup row has no active point
    d_t = _to_device(s["t"])
    with scene_map(ctx, s) as m:
        want = LM.knn2(*m4, *a, skip)
        assert (want[3][64:128] == -1).all() and (want[3][:64] > 0).any() and (want[3][128:] > 0).any()
        assert_raw_equal(ctx.map_match_knn2_local(m, *a, skip), want, "idle wave")
        # without a skip mask nothing is skipped
        assert_raw_equal(ctx.map_match_knn2_local(m, *a), LM.knn2(*m4, *a), "no mask")
        # other parameters
        P = dict(OTHER)
        raw, feat = LM.scene_answer(257, 8, 1100, OTHER)
        assert not np.array_equal(raw[3], LM.scene_answer(257, 8, 1100)[0][3])
        assert_raw_equal(ctx.map_match_knn2_local(m, *a, s["skip"], P), raw, "other parameters")
        assert ctx.map_match_features_local(m, *a, s["skip"], P)[0].tobytes() == feat.tobytes()
        # the frame's descriptors in HBM
        got = ctx.map_match_knn2_local_dev(m, a[0], a[1], a[2], a[3], d_t.data_ptr(), *a[5:], s["skip"])
        assert_raw_equal(got, LM.scene_answer(257, 8, 1100)[0], "device-pointer form")


def test_a_smaller_map_on_the_same_ctx_and_a_reupload(mvo):
    c = mvo.Context(0)
    try:
        for n_map in (700, 63, 700):
            s = LM.scene(n_map, 8)
            with scene_map(c, s) as m:
                assert_raw_equal(c.map_match_knn2_local(m, *LM.scene_args(s, 1100), s["skip"]), LM.scene_answer(n_map, 8, 1100)[0],
                                 "%d points" % n_map)
        # one map handle: 257 points, then 65 in the same buffers; the upload takes the view data with it
        big, small = LM.scene(257, 2), LM.scene(65, 2)
        with scene_map(c, big) as m:
            assert_raw_equal(c.map_match_knn2_local(m, *LM.scene_args(big, 257), big["skip"]), LM.scene_answer(257, 2, 257)[0], "before")
            c.map_upload(m, small["pos"], small["desc"])
            with pytest.raises(mvo.MvoError) as e:
                c.map_match_knn2_local(m, *LM.scene_args(small, 257), small["skip"])
            assert e.value.code == mvo.MVO_ERR_INVALID and "no view data since the last upload" in str(e.value)
            with pytest.raises(mvo.MvoError):
                c.map_match_features_local(m, *LM.scene_args(small, 257), small["skip"])
            c.map_upload_view(m, small["normal"], small["max_dist"])
            assert_raw_equal(c.map_match_knn2_local(m, *LM.scene_args(small, 257), small["skip"]), LM.scene_answer(65, 2, 257)[0], "after")
    finally:
        c.close()


def test_errors_write_nothing(mvo, ctx):
    s = LM.scene(63, 2)
    nt = 257
    T, K, cols, rows, t, txy, t_level, ls = LM.scene_args(s, nt)
    lib, h = ctx.lib, ctx.h
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    Tc = np.ascontiguousarray(T, np.float64)
    k = dict(K)

    def call(m, T_=Tc, t_=t, txy_=txy, lev=t_level, n=nt, ls_=ls, L=2, params=None, idx=True, dist=True, cols_=cols, rows_=rows, **kw):
        """-> (code, whether any output byte changed)"""
        k_ = [C.c_double(dict(k, **kw)[name]) for name in ("fx", "fy", "cx", "cy")]
        outs = [np.full((63, 2), 7, np.float32), np.full((63, 2), 7, np.int32), np.full((63, 2), 7, np.int32), np.full(63, 7, np.int32),
                np.full(63, 7, np.int32), np.full(63, 7, np.float64)]
        before = [o.tobytes() for o in outs]
        pp = None if params is None else C.byref(mvo.LocalMapParams(*params))
        r = lib.mvo_map_match_knn2_local(h, m, p(T_), *k_, cols_, rows_, p(t_), p(txy_), p(lev), n, p(s["skip"]), p(ls_), L, pp,
                                         p(outs[0]), p(outs[1]) if idx else None, p(outs[2]) if dist else None, p(outs[3]), p(outs[4]),
                                         p(outs[5]))
        return r, any(o.tobytes() != b for o, b in zip(outs, before))

    INV, CAP = (mvo.MVO_ERR_INVALID, False), (mvo.MVO_ERR_CAPACITY, False)
    with scene_map(ctx, s) as m:
        assert call(m) == (mvo.MVO_OK, True)
        # a null pointer with a positive count, a null map, a negative count
        for kw in (dict(t_=None), dict(txy_=None), dict(lev=None), dict(idx=False), dict(dist=False), dict(T_=None), dict(ls_=None),
                   dict(n=-1)):
            assert call(m, **kw) == INV, kw
        assert call(None) == INV
        # the pose, the intrinsics, the frame
        singular = np.array(Tc)
        singular[:3, :3] = 0
        assert call(m, T_=singular) == INV
        for bad in (np.nan, np.inf):
            Tb = np.array(Tc)
            Tb[1, 3] = bad
            assert call(m, T_=Tb) == INV
        assert call(m, fx=0.0) == INV and call(m, fy=0.0) == INV and call(m, cx=np.nan) == INV
        assert call(m, cols_=0) == INV and call(m, rows_=-480) == INV
        # the level table: its length, positive, finite, strictly increasing
        assert call(m, L=0) == INV and call(m, L=17, ls_=LM.level_scales(1.2, 17)) == INV
        for bad in ([1.0, 1.0], [1.2, 1.0], [0.0, 1.0], [-1.0, 1.0], [1.0, np.inf], [1.0, np.nan]):
            assert call(m, ls_=np.array(bad)) == INV, bad
        # a keypoint level outside 0..L-1 that is not the taken mark
        for bad in (2, -1, -3):
            lev = np.array(t_level)
            lev[200] = bad
            assert call(m, lev=lev) == INV, bad
        # the parameters
        good = [0.5, 2.5, 4.0, 0.998, 1.0, 0.8, 100, 0]
        assert call(m, params=good) == (mvo.MVO_OK, True)
        for i, bad in ((0, np.nan), (1, -1.0), (1, np.inf), (2, -0.5), (2, np.nan), (3, np.inf), (4, -1.0), (4, np.nan)):
            assert call(m, params=good[:i] + [bad] + good[i + 1:]) == INV, (i, bad)
        # more keypoints than the 16-bit index holds
        big, bigxy, biglev = np.zeros((65536, 32), np.uint8), np.zeros((65536, 2), np.float32), np.zeros(65536, np.int32)
        assert call(m, t_=big, txy_=bigxy, lev=biglev, n=65536) == CAP
        # the view data given for fewer points than the map holds is an error of the Python mirror; without any: INVALID
        ctx.map_upload(m, s["pos"], s["desc"])
        assert call(m) == INV and b"no view data since the last upload" in lib.mvo_last_error(h)
        assert lib.mvo_map_upload_view(h, m, None, p(s["max_dist"])) == mvo.MVO_ERR_INVALID
        assert lib.mvo_map_upload_view(h, None, p(s["normal"]), p(s["max_dist"])) == mvo.MVO_ERR_INVALID
        assert call(m) == INV
        ctx.map_upload_view(m, s["normal"], s["max_dist"])
        # the matches: the capacity convention (the count reported, nothing written), then the context still works
        n_all = len(LM.scene_answer(63, 2, nt)[1])
        assert n_all > 2
        a = LM.scene_args(s, nt)
        with pytest.raises(mvo.MvoError) as e:
            ctx.map_match_features_local(m, *a, s["skip"], cap=n_all - 1)
        assert e.value.code == mvo.MVO_ERR_CAPACITY
        out, cnt = np.full(n_all - 1, 7, mvo.DMATCH_DTYPE), C.c_int(-5)
        k_ = [C.c_double(k[name]) for name in ("fx", "fy", "cx", "cy")]
        assert lib.mvo_map_match_features_local(h, m, p(Tc), *k_, cols, rows, p(t), p(txy), p(t_level), nt, p(s["skip"]), p(ls), 2, None,
                                                None, None, p(out), n_all - 1, C.byref(cnt)) == mvo.MVO_ERR_CAPACITY
        assert cnt.value == n_all and out.tobytes() == np.full(n_all - 1, 7, mvo.DMATCH_DTYPE).tobytes()
        assert lib.mvo_map_match_features_local(h, m, p(Tc), *k_, cols, rows, p(t), p(txy), p(t_level), nt, p(s["skip"]), p(ls), 2, None,
                                                None, None, p(out), n_all - 1, None) == mvo.MVO_ERR_INVALID
        assert len(ctx.map_match_features_local(m, *a, s["skip"], cap=n_all)[0]) == n_all
        assert_raw_equal(ctx.map_match_knn2_local(m, *a, s["skip"]), LM.scene_answer(63, 2, nt)[0], "after the errors")
    # an empty map succeeds and writes nothing, with or without view data
    e = ctx.map_create()
    try:
        assert call(e) == (mvo.MVO_OK, False)
        ctx.map_upload_view(e, np.zeros((0, 3), np.float32), np.zeros(0, np.float32))
        assert call(e) == (mvo.MVO_OK, False)
        got = ctx.map_match_knn2_local(e, *LM.scene_args(s, nt))
        assert got[0].shape == (0, 2) and got[5].shape == (0,)
        assert len(ctx.map_match_features_local(e, *LM.scene_args(s, nt))[0]) == 0
    finally:
        ctx.map_release(e)
