"""The triangulation of new map points against every buffered frame on the MI355X (csrc/window_triangulate_kernels.hip,
csrc/window_triangulate_host.cpp) against its numpy transcription (tests/window_triangulate_numpy.py; known answers of its own in
tests/test_window_triangulate_numpy.py), bit for bit: the raw search (idx, dist, n_candidates of every frame), every pair with its
status, cos2 and both points, the chosen points and the counts; over one to 64 frames, one to three train groups, frames whose
waves have empty slices, empty frames, frames without a baseline; 0, 1, 256 and 257 pairs in front of the verification; a repeated
call, scales, every parameter away from its default, a resident map left alone, every error code.  A NaN equals a NaN whatever its
sign (0 / 0 has none that IEEE 754 fixes).  tests/test_window_triangulate_sim.py runs the same functions on the emulated build."""
import ctypes as C
import functools

import numpy as np
import pytest

import window_triangulate_numpy as W

pytestmark = pytest.mark.gpu

K = W.FR1_K
# (keypoints of curr, frames) -> keypoints per frame
SHAPES = {
    (1, 1): [1],
    (3, 2): [5, 0],
    (64, 1): [64],
    (65, 3): [257, 63, 1],         # two query groups, two train groups; frames 1 and 2 leave most waves an empty slice
    (130, 19): [40, 300] + [int(x) for x in np.random.RandomState(19).randint(40, 301, 17)],
    (40, 64): [20, 80] + [int(x) for x in np.random.RandomState(64).randint(20, 81, 62)],
    (70, 2): [513, 700],           # three train groups
}
CASES = sorted(SHAPES)
# how the scene of a shape differs from the default one
SCENES = {
    (130, 19): dict(block=64),                                                       # the first 64 keypoints of curr are not free
    (40, 64): dict(step=0.02, yaw=0.0, still=tuple(range(2, 64, 5))),                # every fifth frame stands where curr stands
}
# what each shape must exercise (asserted on the transcription's answer, so that no case is vacuous)
EVENTS = {
    (1, 1): {"point"},
    (3, 2): {"point", "empty frame"},
    (64, 1): {"point", "depth"},
    (65, 3): {"point", "multi-group fold", "depth"},
    (130, 19): {"point", "inactive wave", "contested train", "several frames", "depth", "parallax"},
    (40, 64): {"point", "inactive wave", "inactive frame", "several frames", "depth", "parallax"},
    (70, 2): {"point", "multi-group fold", "depth", "parallax"},
}
# every parameter away from its default; the scales of the scene and these bounds bring out the status bits the defaults leave rare
PARAMS = [
    dict(max_line_px=3.5, lowe_ratio=0.9, max_hamming=80, max_cos_parallax=0.9999, max_reproj_chi2=0.8, ratio_factor=1.25, min_baseline=0.5),
    dict(max_line_px=0.0),
    dict(max_hamming=0),
    dict(max_hamming=256, lowe_ratio=2.0, max_cos_parallax=1.0),
    dict(min_baseline=100.0),
    dict(max_reproj_chi2=0.0, ratio_factor=0.0, max_cos_parallax=0.0),
]


def frozen(d):
    return tuple(sorted(d.items()))


@functools.lru_cache(maxsize=None)
def case(n, F, scales=False, params=()):
    """Inputs and the transcription's answer; computed once, read-only."""
    s = W.scene(np.random.RandomState(1000 * n + F), n, SHAPES[(n, F)], K=K, scales=scales, **SCENES.get((n, F), {}))
    assert len(s["curr"]["desc"]) == n
    points, pairs, counts, raw = W.window_triangulate(s["curr"], s["frames"], K, **dict(params))
    for a in (points, pairs, counts) + raw:
        a.setflags(write=False)
    return dict(s, raw=raw, want=(points, pairs, counts), params=dict(params))


def events(c):
    """The special cases the transcription met on this case."""
    idx, dist, cnt = c["raw"]
    points, pairs, counts = c["want"]
    kp = [len(fr["desc"]) for fr in c["frames"]]
    n = len(c["curr"]["desc"])
    P = dict(W.DEFAULTS, **c["params"])
    out = set()
    out |= {"point"} if len(points) else set()
    out |= {"empty frame"} if 0 in kp else set()
    out |= {"inactive frame"} if counts[1] < len(kp) else set()
    if any((cnt[f, b:b + 64] == -1).all() for f in range(len(kp)) for b in range(0, n, 64)):
        out.add("inactive wave")       # a group of 64 keypoints of curr none of which is active in the frame
    if max(kp) > 256:                  # more than one train group: some first neighbour from beyond the first group's trains
        f = int(np.argmax(kp))
        groups = -(-kp[f] // 256)
        first_group = 4 * (-(-kp[f] // (4 * groups)))
        if (idx[f, :, 0] >= first_group).any() and ((idx[f, :, 0] >= 0) & (idx[f, :, 0] < first_group)).any():
            out.add("multi-group fold")
    claims = (idx[:, :, 0] >= 0) & (dist[:, :, 0] <= P["max_hamming"]) & ((idx[:, :, 1] < 0) | (dist[:, :, 0].astype(np.float64)
                                                                          < P["lowe_ratio"] * dist[:, :, 1].astype(np.float64)))
    out |= {"contested train"} if claims.sum() > len(pairs) else set()
    ok = pairs[pairs["status"] == 0]
    out |= {"several frames"} if len(ok) > len(np.unique(ok["keypoint"])) else set()
    for bit, name in ((1, "not finite"), (2, "depth"), (4, "parallax"), (8, "reprojection in the frame"), (16, "reprojection in curr"),
                      (32, "scale")):
        out |= {name} if (pairs["status"] & bit).any() else set()
    return out


def same_bits(g, w):
    """Elementwise: the same bits, or both NaN."""
    if g.dtype.kind == "f":
        return (g.view("u%d" % g.dtype.itemsize) == w.view("u%d" % w.dtype.itemsize)) | (np.isnan(g) & np.isnan(w))
    return g == w


def assert_same(got, want, names, what):
    for name, g, w in zip(names, got, want):
        if w.dtype.names:
            assert len(g) == len(w), "%s: %s has %d records, expected %d" % (what, name, len(g), len(w))
            for field in w.dtype.names:
                gf, wf = np.ascontiguousarray(g[field]), np.ascontiguousarray(w[field])
                assert gf.dtype == wf.dtype, "%s: %s.%s is %s, expected %s" % (what, name, field, gf.dtype, wf.dtype)
                bad = np.argwhere(~same_bits(gf, wf))
                assert not len(bad), "%s: %s.%s differs by its bits at %d places, first %r: %r vs %r" % (
                    what, name, field, len(bad), tuple(bad[0]), gf[tuple(bad[0])], wf[tuple(bad[0])])
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s is %s %s, expected %s %s" % (what, name, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)
            raise AssertionError("%s: %s differs by its bits at %d places, first %r: %r vs %r"
                                 % (what, name, len(bad), tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])]))


RAW, RULE = ("idx", "dist", "n_candidates"), ("points", "pairs", "counts")


def run(ctx, c, what):
    P = dict(W.DEFAULTS, **c["params"])
    assert_same(ctx.window_triangulate_search(c["curr"], c["frames"], K, P["max_line_px"], P["min_baseline"]), c["raw"], RAW, what)
    assert_same(ctx.window_triangulate(c["curr"], c["frames"], K, **c["params"]), c["want"], RULE, what)


@pytest.mark.parametrize("n,F", CASES)
def test_search_bit_exact(ctx, n, F):
    c = case(n, F)
    assert_same(ctx.window_triangulate_search(c["curr"], c["frames"], K), c["raw"], RAW, "%d keypoints, %d frames" % (n, F))


@pytest.mark.parametrize("n,F", CASES)
def test_window_triangulate_bit_exact(ctx, O, n, F):
    c = case(n, F)
    missing = EVENTS[(n, F)] - events(c)
    assert not missing, "the case does not exercise %r (counts %r)" % (sorted(missing), c["want"][2])
    points, pairs, counts = ctx.window_triangulate(c["curr"], c["frames"], K)
    assert_same((points, pairs, counts), c["want"], RULE, "%d keypoints, %d frames" % (n, F))
    # the triangulated floats against the oracle's helperTriangulatePoints, frame by frame
    for f in np.unique(pairs["frame"]):
        p = pairs[pairs["frame"] == f]
        R, t, _ = W.relative(c["curr"], c["frames"][f], 0.0)
        p_f, p_c = O.triangulate_points(c["frames"][f]["xy"][p["train"]], c["curr"]["xy"][p["keypoint"]], K, R, t)
        assert same_bits(np.ascontiguousarray(p["p_frame"]), p_f).all() and same_bits(np.ascontiguousarray(p["p_curr"]), p_c).all()


def degenerate():
    """A keypoint on the principal point of both cameras of a sideways pair: the two rays are parallel, the DLT's answer is the point
    at infinity (0, 0, 1, 0) exactly, and the division by w leaves nothing finite."""
    K2 = dict(fx=500.0, fy=500.0, cx=320.0, cy=240.0)
    d = np.zeros((1, 32), np.uint8)
    one = lambda x: dict(desc=d, xy=np.array([[320, 240]], np.float32), scale=None, conn=np.array([-1], np.int32), T=W.camera(x))
    return K2, one(0.0), [one(-1.0)]


def test_every_status_bit_occurs_over_the_set():
    seen = set()
    for n, F in CASES:
        seen |= events(case(n, F))
    for p in PARAMS:
        seen |= events(case(130, 19, True, frozen(p)))
    K2, curr, frames = degenerate()
    want = W.window_triangulate(curr, frames, K2)
    assert want[1]["status"][0] & W.NOT_FINITE
    assert {"depth", "parallax", "reprojection in the frame", "reprojection in curr", "scale", "contested train", "several frames",
            "inactive wave", "inactive frame", "empty frame", "multi-group fold"} <= seen


def test_a_pair_that_is_not_finite(ctx):
    K2, curr, frames = degenerate()
    want = W.window_triangulate(curr, frames, K2)
    got = ctx.window_triangulate(curr, frames, K2)
    assert_same(got, want[:3], RULE, "parallel rays")
    assert got[1]["status"][0] & W.NOT_FINITE and len(got[0]) == 0 and got[2][4] == 1


@functools.lru_cache(maxsize=None)
def counted(n_pairs):
    """A keyframe and one frame 0.3 to its left with exactly n_pairs pairs after the filter: n_pairs points at depth 4 (the partner
    38.8 px to the right, with the same descriptor), and four keypoints more on each side that match nothing."""
    rng = np.random.RandomState(n_pairs + 5)
    n = n_pairs + 4
    i = np.arange(n)
    xy = np.stack([60 + 2.0 * (i % 200), 40 + 7.0 * (i // 200)], 1).astype(np.float32)
    d = np.packbits(rng.randint(0, 2, (n, 256)).astype(np.uint8), axis=1).reshape(n, 32)
    d2 = d.copy()
    d2[n_pairs:] ^= 255                                                               # 256 bits away: above every ceiling
    shift = np.float32(K["fx"] * 0.3 / 4.0)
    curr = dict(desc=d, xy=xy, scale=None, conn=np.full(n, -1, np.int32), T=W.camera(0.0))
    frame = dict(desc=d2, xy=(xy + np.array([shift, 0], np.float32)).astype(np.float32), scale=None, conn=np.full(n, -1, np.int32),
                 T=W.camera(-0.3))
    want = W.window_triangulate(curr, [frame], K)
    assert want[2][3] == n_pairs and want[2][11] == n_pairs, want[2]
    return curr, [frame], want


@pytest.mark.parametrize("n_pairs", [0, 1, 256, 257])
def test_pair_counts_around_the_verification_launch(ctx, n_pairs):
    curr, frames, want = counted(n_pairs)
    assert_same(ctx.window_triangulate(curr, frames, K), want[:3], RULE, "%d pairs" % n_pairs)


def test_a_repeated_call_gives_the_same_bytes(ctx):
    c = case(65, 3)
    for k in range(3):
        run(ctx, c, "call %d" % k)


def test_a_smaller_call_between_two_larger_ones(ctx):
    """The buffers and the arrival counters of a three-group call serve a one-group call and the other way round."""
    a, b = case(70, 2), case(64, 1)
    for c in (a, b, a):
        run(ctx, c, "%d keypoints" % len(c["curr"]["desc"]))


def test_scales(ctx):
    """Per-keypoint scales 1.2^octave widen the gate of a frame's keypoint and the reprojection bound of both; scale NULL is every
    scale 1."""
    c, plain = case(130, 19, True), case(130, 19, False)
    assert all(len(set(fr["scale"].tolist())) == 4 for fr in [c["curr"]] + c["frames"][1:3])
    narrow = W.search(c["curr"], [dict(fr, scale=None) for fr in c["frames"]], K)
    assert c["raw"][2].sum() > narrow[2].sum(), "the scales admit no keypoint more"
    run(ctx, c, "scales")
    ones = lambda fr: dict(fr, scale=np.ones(len(fr["desc"]), np.float32))
    got = ctx.window_triangulate(ones(plain["curr"]), [ones(fr) for fr in plain["frames"]], K)
    assert_same(got, plain["want"], RULE, "scales of 1")


@pytest.mark.parametrize("k", range(len(PARAMS)))
def test_parameters_other_than_the_defaults(ctx, k):
    c, d = case(130, 19, True, frozen(PARAMS[k])), case(130, 19, True)
    counts, default = c["want"][2], d["want"][2]
    assert counts.tobytes() != default.tobytes()
    if k == 0:
        assert counts[1] < default[1] and all(counts[4 + b] > 0 for b in (1, 3, 4, 5)) and counts[11] > 0
    if PARAMS[k].get("max_line_px") == 0.0:
        assert (c["raw"][2] <= 0).all()
    if PARAMS[k].get("max_hamming") == 0:
        assert counts[3] == 0 and counts[2] > 0
    if PARAMS[k].get("max_hamming") == 256:
        assert counts[3] > default[3] and counts[6] < default[6]
    if PARAMS[k].get("min_baseline") == 100.0:
        assert counts[1] == 0 and (c["raw"][2] == -1).all()
    if PARAMS[k].get("max_reproj_chi2") == 0.0:
        assert counts[3] > 0 and counts[10] == 0 and counts[6] == counts[3] and counts[9] == counts[3]
    run(ctx, c, "parameters %r" % (PARAMS[k],))


def test_explicit_defaults_are_the_defaults(ctx):
    c = case(65, 3)
    assert_same(ctx.window_triangulate(c["curr"], c["frames"], K, **W.DEFAULTS), c["want"], RULE, "explicit defaults")


def test_the_resident_map_is_left_alone(ctx):
    c = case(65, 3)
    rng = np.random.RandomState(3)
    pos, desc = rng.rand(100, 3).astype(np.float32), rng.randint(0, 256, (100, 32)).astype(np.uint8)
    m = ctx.map_create()
    try:
        ctx.map_upload(m, pos, desc)
        run(ctx, c, "with a resident map")
        got_pos, got_desc = ctx.map_debug_get(m)
        assert got_pos.tobytes() == pos.tobytes() and got_desc.tobytes() == desc.tobytes()
    finally:
        ctx.map_release(m)


def test_errors(mvo, ctx):
    c = case(65, 3)
    n, F = 65, 3
    k = [K[name] for name in ("fx", "fy", "cx", "cy")]
    idx, dist, cnt = np.full((F, n, 2), 77, np.int32), np.full((F, n, 2), 77, np.int32), np.full((F, n), 77, np.int32)
    points, pairs = np.full(1000 * 10, 77, np.int32), np.full(1000 * 14, 77, np.int32)       # 1000 records each, as words
    n_points, n_pairs, counts = C.c_int(77), C.c_int(77), np.full(12, 77, np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    INV, CAP = mvo.MVO_ERR_INVALID, mvo.MVO_ERR_CAPACITY

    def untouched():
        return all((a == 77).all() for a in (idx, dist, cnt, points, pairs, counts))

    def params(**kw):
        d = dict(W.DEFAULTS, **kw)
        return mvo.WindowTriangulateParams(d["max_line_px"], d["lowe_ratio"], d["max_hamming"], d["max_cos_parallax"], d["max_reproj_chi2"],
                                           d["ratio_factor"], d["min_baseline"])

    def both(curr, frames, n_frames=None, kk=k, outs=True, search=True, **kw):
        """The two entry points on the same bad input -> their codes (which must agree)."""
        carr, _, ckeep = ctx._fuse_frames([curr]) if curr is not None else (None, None, None)
        arr, _, keep = ctx._fuse_frames(frames) if frames is not None else (None, None, None)
        nf = len(frames) if n_frames is None else n_frames
        kc = [C.c_double(v) for v in kk]
        d = dict(W.DEFAULTS, **kw)
        a = search and ctx.lib.mvo_window_triangulate_search(ctx.h, carr, arr, nf, *kc, C.c_double(d["max_line_px"]), C.c_double(d["min_baseline"]),
                                                             p(idx) if outs else None, p(dist) if outs else None, p(cnt))
        b = ctx.lib.mvo_window_triangulate(ctx.h, carr, arr, nf, *kc, C.byref(params(**kw)), p(points) if outs else None, 1000,
                                           C.byref(n_points), p(pairs), 1000, C.byref(n_pairs), p(counts))
        assert n_points.value == 77 and n_pairs.value == 77
        return a, b

    curr, frames = c["curr"], c["frames"]

    def changed(f, **kw):
        out = [dict(fr) for fr in frames]
        out[f].update(kw)
        return out

    assert both(None, frames) == (INV, INV)                                                    # null pointers with a positive count
    assert both(curr, None, n_frames=3) == (INV, INV)
    assert both(curr, frames, outs=False) == (INV, INV)
    assert both(curr, frames, n_frames=-1) == (INV, INV)
    for field in ("desc", "xy", "conn"):
        for which in (0, 1):
            carr, _, ckeep = ctx._fuse_frames([curr])
            arr, _, keep = ctx._fuse_frames(frames)
            setattr((carr, arr)[which][0], field, None)
            kc = [C.c_double(v) for v in k]
            assert ctx.lib.mvo_window_triangulate_search(ctx.h, carr, arr, F, *kc, C.c_double(2.0), C.c_double(0.0), p(idx), p(dist), p(cnt)) == INV
            assert ctx.lib.mvo_window_triangulate(ctx.h, carr, arr, F, *kc, None, p(points), 1000, C.byref(n_points), p(pairs), 1000,
                                                  C.byref(n_pairs), p(counts)) == INV
    carr, _, ckeep = ctx._fuse_frames([curr])
    arr, _, keep = ctx._fuse_frames(frames)
    arr[1].n = -1
    kc = [C.c_double(v) for v in k]
    assert ctx.lib.mvo_window_triangulate_search(ctx.h, carr, arr, F, *kc, C.c_double(2.0), C.c_double(0.0), p(idx), p(dist), p(cnt)) == INV
    arr, _, keep = ctx._fuse_frames(frames)
    for args in ((None, 1000, C.byref(n_points), p(pairs), 1000, C.byref(n_pairs), p(counts)),         # points null with a capacity
                 (p(points), 1000, None, p(pairs), 1000, C.byref(n_pairs), p(counts)),                  # no n_points
                 (p(points), 1000, C.byref(n_points), p(pairs), 1000, None, p(counts)),                 # pairs without n_pairs
                 (p(points), 1000, C.byref(n_points), p(pairs), 1000, C.byref(n_pairs), None),          # no counts
                 (p(points), -1, C.byref(n_points), p(pairs), 1000, C.byref(n_pairs), p(counts))):
        assert ctx.lib.mvo_window_triangulate(ctx.h, carr, arr, F, *kc, None, *args) == INV
    for v in (np.nan, np.inf):                                                                 # a non-finite pose, a singular pose
        T = frames[2]["T"].copy()
        T[1, 3] = v
        assert both(curr, changed(2, T=T)) == (INV, INV)
        assert both(dict(curr, T=T), frames) == (INV, INV)
    T = frames[1]["T"].copy()
    T[:3, :3] = 0
    assert both(curr, changed(1, T=T)) == (INV, INV) and both(dict(curr, T=T), frames) == (INV, INV)
    for bad in ([0.0, k[1], k[2], k[3]], [k[0], 0.0, k[2], k[3]], [k[0], k[1], np.nan, k[3]], [np.inf, k[1], k[2], k[3]]):
        assert both(curr, frames, kk=bad) == (INV, INV)
    for name in ("max_line_px", "min_baseline"):
        for v in (-0.5, float("nan")):
            assert both(curr, frames, **{name: v}) == (INV, INV)
    for name, values in (("max_reproj_chi2", (-1.0, np.nan)), ("ratio_factor", (-1.0, np.nan)), ("lowe_ratio", (np.nan,)),
                         ("max_cos_parallax", (-0.1, 1.5, np.nan)), ("max_hamming", (-1, 257))):
        for v in values:
            assert both(curr, frames, search=False, **{name: v})[1] == INV
    for v in (-1.0, np.nan, np.inf):                                                           # a bad scale entry, in a frame and in curr
        scale = np.ones(len(frames[0]["desc"]), np.float32)
        scale[7] = v
        assert both(curr, changed(0, scale=scale)) == (INV, INV)
        scale = np.ones(n, np.float32)
        scale[7] = v
        assert both(dict(curr, scale=scale), frames) == (INV, INV)
    with pytest.raises(mvo.MvoError) as e:
        ctx.window_triangulate(curr, frames, K, max_hamming=300)
    assert e.value.code == INV
    with pytest.raises(TypeError):
        ctx.window_triangulate(curr, frames, K, max_px=3.0)
    assert untouched()
    # MVO_ERR_CAPACITY: 65 frames; 65536 keypoints in a frame or in curr; an output too small (the needed count is set, nothing else
    # is written)
    assert both(curr, [frames[2]] * 65) == (CAP, CAP)
    big = dict(desc=np.zeros((65536, 32), np.uint8), xy=np.zeros((65536, 2), np.float32), conn=np.full(65536, -1, np.int32), scale=None,
               T=np.eye(4))
    assert both(curr, [frames[0], big]) == (CAP, CAP)
    with pytest.raises(mvo.MvoError) as e:
        ctx.window_triangulate_search(big, frames, K)
    assert e.value.code == CAP
    with pytest.raises(mvo.MvoError) as e:
        ctx.window_triangulate(big, frames, K)
    assert e.value.code == CAP
    assert untouched()
    want_points, want_pairs, want_counts = c["want"]
    n_want, np_want = len(want_points), len(want_pairs)
    assert 1 < n_want < np_want
    carr, _, ckeep = ctx._fuse_frames([curr])
    arr, _, keep = ctx._fuse_frames(frames)
    call = lambda cap_points, pairs_, cap_pairs: ctx.lib.mvo_window_triangulate(
        ctx.h, carr, arr, F, *kc, None, p(points), cap_points, C.byref(n_points), pairs_, cap_pairs, C.byref(n_pairs), p(counts))
    assert call(n_want - 1, p(pairs), 1000) == CAP
    assert n_points.value == n_want and n_pairs.value == np_want and untouched()
    n_points.value = n_pairs.value = 77
    assert call(1000, p(pairs), np_want - 1) == CAP
    assert n_points.value == n_want and n_pairs.value == np_want and untouched()
    # pairs NULL: its capacity and count are not looked at
    n_points.value = n_pairs.value = 77
    assert call(n_want, None, -5) == mvo.MVO_OK
    assert n_points.value == n_want and n_pairs.value == 77 and (pairs == 77).all() and counts.tobytes() == want_counts.tobytes()
    got = points[:10 * n_want].view(mvo.WINDOW_POINT_DTYPE)
    assert_same((got,), (want_points,), ("points",), "exact capacity")
    assert (points[10 * n_want:] == 77).all()
    assert call(n_want, p(pairs), np_want) == mvo.MVO_OK
    assert_same((pairs[:14 * np_want].view(mvo.WINDOW_PAIR_DTYPE),), (want_pairs,), ("pairs",), "exact capacity")
    assert (pairs[14 * np_want:] == 77).all()
    # the optional output of the search
    assert ctx.lib.mvo_window_triangulate_search(ctx.h, carr, arr, F, *kc, C.c_double(2.0), C.c_double(0.0), p(idx), p(dist), None) == mvo.MVO_OK
    assert idx.tobytes() == c["raw"][0].tobytes() and dist.tobytes() == c["raw"][1].tobytes() and (cnt == 77).all()
    # no frames, no keypoints, no free keypoint: success without a launch
    got = ctx.window_triangulate(curr, [], K)
    assert len(got[0]) == 0 and len(got[1]) == 0 and got[2].tolist() == [int((curr["conn"] == -1).sum())] + [0] * 11
    assert [a.shape for a in ctx.window_triangulate_search(curr, [], K)] == [(0, n, 2), (0, n, 2), (0, n)]
    empty = dict(desc=np.zeros((0, 32), np.uint8), xy=np.zeros((0, 2), np.float32), conn=np.zeros(0, np.int32), scale=None, T=W.camera(5.0))
    got = ctx.window_triangulate(empty, frames, K)
    assert len(got[0]) == 0 and got[2].tolist() == [0, 3] + [0] * 10
    assert [a.shape for a in ctx.window_triangulate_search(empty, frames, K)] == [(3, 0, 2), (3, 0, 2), (3, 0)]
    taken = dict(curr, conn=np.zeros(n, np.int32))
    assert_same(ctx.window_triangulate(taken, frames, K), W.window_triangulate(taken, frames, K)[:3], RULE, "no free keypoint")
    assert_same(ctx.window_triangulate_search(taken, frames, K), W.search(taken, frames, K), RAW, "no free keypoint")
    # frames without keypoints: rows of active keypoints with no candidates
    got = ctx.window_triangulate_search(curr, [dict(empty, T=W.camera(-1.0)), dict(empty, T=W.camera(-2.0))], K)
    assert_same(got, W.search(curr, [dict(empty, T=W.camera(-1.0)), dict(empty, T=W.camera(-2.0))], K), RAW, "two empty frames")
    assert (got[2] == 0).any() and (got[0] == -1).all()
