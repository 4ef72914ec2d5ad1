"""The fusion of duplicate map points on the MI355X (csrc/map_fuse_kernels.hip, csrc/map_fuse_host.cpp) against its numpy
transcription (tests/map_fuse_numpy.py; known answers of its own in tests/test_map_fuse_numpy.py), bit for bit: the raw search
(idx, dist, n_candidates, px of every frame) and the rule (replaced_by, added, counts); over one to 64 frames, one to three train
groups, frames whose waves have empty slices, empty frames; a repeated call, scales, non-default parameters, the resident arrays
left alone, every error code.  tests/test_map_fuse_sim.py runs the same functions on the emulated build."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import map_fuse_numpy as M

pytestmark = pytest.mark.gpu

COLS, ROWS = 640, 480
K = M.FR1_K
# (map points, frames) -> keypoints per frame
SHAPES = {
    (1, 1): [1],
    (3, 2): [5, 0],
    (64, 1): [64],
    (65, 3): [257, 63, 1],         # two query groups, two train groups; frames 1 and 2 leave most waves an empty slice
    (130, 20): [40, 300] + [int(x) for x in np.random.RandomState(20).randint(40, 301, 18)],
    (257, 64): [20, 80] + [int(x) for x in np.random.RandomState(64).randint(20, 81, 62)],
    (70, 2): [513, 700],           # three train groups
}
CASES = sorted(SHAPES)
# what each shape must exercise (asserted on the transcription's answer, so that no case is vacuous)
EVENTS = {
    (1, 1): {"addition"},
    (3, 2): {"addition"},
    (64, 1): {"addition"},
    (65, 3): {"merge", "merge refused", "addition", "addition refused", "inactive wave", "multi-group fold"},
    (130, 20): {"merge", "merge refused", "three members", "addition", "addition refused", "contested keypoint", "inactive wave"},
    (257, 64): {"merge", "merge refused", "three members", "addition", "addition refused", "contested keypoint", "inactive wave"},
    (70, 2): {"merge", "merge refused", "addition", "addition refused", "multi-group fold"},
}


# scene seeds: the first of 0, 1, 2 ... at which the scene of a shape shows every special case listed for it
SEEDS = {(1, 1): 3, (70, 2): 1, (130, 20): 1}


@contextlib.contextmanager
def resident(ctx, pos, desc):
    m = ctx.map_create()
    try:
        ctx.map_upload(m, pos, desc)
        yield m
    finally:
        ctx.map_release(m)


@functools.lru_cache(maxsize=None)
def case(n, F, scales=False, max_px=M.DEFAULT_MAX_PX, max_hamming=M.DEFAULT_MAX_HAMMING):
    """Inputs and the transcription's answer; computed once, read-only."""
    s = M.scene(np.random.RandomState(1000 * n + F + 100000 * SEEDS.get((n, F), 0)), n, SHAPES[(n, F)], K=K, cols=COLS, rows=ROWS, scales=scales)
    assert len(s["pos"]) == n
    raw = M.search(s["pos"], s["desc"], s["frames"], K, COLS, ROWS, max_px)
    trace = {}
    want = M.resolve(n, s["frames"], raw[0], raw[1], max_hamming, trace=trace)
    for a in raw + want:
        a.setflags(write=False)
    return dict(s, raw=raw, want=want, trace=trace)


def events(c):
    """The special cases the transcription met on this case."""
    idx, dist, cnt, _ = c["raw"]
    counts, kp = c["want"][2], [len(fr["desc"]) for fr in c["frames"]]
    n = len(c["pos"])
    out = set()
    out |= {"merge"} if counts[1] else set()
    out |= {"merge refused"} if counts[2] else set()
    out |= {"three members"} if c["trace"]["sizes"][-1] >= 3 else set()
    out |= {"addition"} if counts[3] else set()
    out |= {"addition refused"} if counts[4] else set()
    out |= {"contested keypoint"} if c["trace"]["contested"] else set()
    if any((cnt[f, b:b + 64] == -1).all() for f in range(len(kp)) for b in range(0, n, 64)):
        out.add("inactive wave")       # a group of 64 map points none of which is active in the frame
    if max(kp) > 256:                  # more than one train group: some first neighbour from beyond the first group's trains
        f = int(np.argmax(kp))
        groups = -(-kp[f] // 256)
        first_group = 4 * (-(-kp[f] // (4 * groups)))
        if (idx[f, :, 0] >= first_group).any() and ((idx[f, :, 0] >= 0) & (idx[f, :, 0] < first_group)).any():
            out.add("multi-group fold")
    return out


def assert_same(got, want, names, what):
    for name, g, w in zip(names, got, want):
        if g.dtype.names:
            g = np.stack([g[k] for k in g.dtype.names], 1).reshape(-1, len(g.dtype.names))
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s is %s %s, expected %s %s" % (what, name, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)
            raise AssertionError("%s: %s differs by its bits at %d places, first %r: %r vs %r"
                                 % (what, name, len(bad), tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])]))


RAW, RULE = ("idx", "dist", "n_candidates", "px"), ("replaced_by", "added", "counts")


@pytest.mark.parametrize("n,F", CASES)
def test_search_bit_exact(ctx, n, F):
    c = case(n, F)
    with resident(ctx, c["pos"], c["desc"]) as m:
        assert_same(ctx.map_fuse_search(m, c["frames"], K, COLS, ROWS, M.DEFAULT_MAX_PX), c["raw"], RAW, "%d points, %d frames" % (n, F))


@pytest.mark.parametrize("n,F", CASES)
def test_fuse_bit_exact(ctx, n, F):
    c = case(n, F)
    missing = EVENTS[(n, F)] - events(c)
    assert not missing, "the case does not exercise %r (counts %r)" % (sorted(missing), c["want"][2])
    with resident(ctx, c["pos"], c["desc"]) as m:
        assert_same(ctx.map_fuse(m, c["frames"], K, COLS, ROWS), c["want"], RULE, "%d points, %d frames" % (n, F))
        pos, desc = ctx.map_debug_get(m)      # the resident arrays are not changed
        assert pos.tobytes() == c["pos"].tobytes() and desc.tobytes() == c["desc"].tobytes()


def test_a_repeated_call_gives_the_same_bytes(ctx):
    c = case(65, 3)
    with resident(ctx, c["pos"], c["desc"]) as m:
        for k in range(3):
            assert_same(ctx.map_fuse_search(m, c["frames"], K, COLS, ROWS, M.DEFAULT_MAX_PX), c["raw"], RAW, "call %d" % k)
            assert_same(ctx.map_fuse(m, c["frames"], K, COLS, ROWS), c["want"], RULE, "call %d" % k)


def test_a_smaller_call_after_a_larger_one(ctx):
    """The buffers and the arrival counters of a three-group call serve a one-group call and the other way round."""
    a, b = case(70, 2), case(64, 1)
    for c in (a, b, a):
        with resident(ctx, c["pos"], c["desc"]) as m:
            assert_same(ctx.map_fuse_search(m, c["frames"], K, COLS, ROWS, M.DEFAULT_MAX_PX), c["raw"], RAW, "%d points" % len(c["pos"]))


def test_scales(ctx):
    """Per-keypoint scales 1.2^octave widen the gate keypoint by keypoint; scale NULL is every scale 1."""
    c, plain = case(130, 20, True), case(130, 20, False)
    assert any(fr["scale"] is not None and len(set(fr["scale"].tolist())) == 4 for fr in c["frames"])
    ones = [dict(fr, scale=np.ones(len(fr["desc"]), np.float32)) for fr in plain["frames"]]
    wide = M.search(c["pos"], c["desc"], [dict(fr, scale=None) for fr in c["frames"]], K, COLS, ROWS, M.DEFAULT_MAX_PX)
    assert c["raw"][2].sum() > wide[2].sum(), "the scales admit no keypoint more"
    with resident(ctx, c["pos"], c["desc"]) as m:
        assert_same(ctx.map_fuse_search(m, c["frames"], K, COLS, ROWS, M.DEFAULT_MAX_PX), c["raw"], RAW, "scales")
        assert_same(ctx.map_fuse(m, c["frames"], K, COLS, ROWS), c["want"], RULE, "scales")
    with resident(ctx, plain["pos"], plain["desc"]) as m:
        assert_same(ctx.map_fuse_search(m, ones, K, COLS, ROWS, M.DEFAULT_MAX_PX), plain["raw"], RAW, "scales of 1")


@pytest.mark.parametrize("max_px,max_hamming", [(5.5, 30), (3.0, 0), (3.0, 256), (0.0, 50), (1.25, 40)])
def test_parameters_other_than_the_defaults(ctx, max_px, max_hamming):
    c, d = case(130, 20, False, max_px, max_hamming), case(130, 20)
    if max_hamming == 0:
        assert 0 < c["want"][2][0] == (c["raw"][1][:, :, 0] == 0).sum() < d["want"][2][0]      # (the twins: distance 0)
    if max_hamming == 256:
        assert c["want"][2][0] == (c["raw"][0][:, :, 0] >= 0).sum() > d["want"][2][0]
    if max_px == 0.0:
        assert (c["raw"][2] <= 0).all()
    if (max_px, max_hamming) in ((5.5, 30), (1.25, 40)):
        assert c["want"][2].tobytes() != d["want"][2].tobytes() and c["want"][2][1] > 0 and c["want"][2][3] > 0
    with resident(ctx, c["pos"], c["desc"]) as m:
        assert_same(ctx.map_fuse_search(m, c["frames"], K, COLS, ROWS, max_px), c["raw"], RAW, "max_px %r" % max_px)
        assert_same(ctx.map_fuse(m, c["frames"], K, COLS, ROWS, max_px=max_px, max_hamming=max_hamming), c["want"], RULE,
                    "max_px %r, max_hamming %d" % (max_px, max_hamming))


def test_explicit_defaults_are_the_defaults(ctx):
    c = case(65, 3)
    with resident(ctx, c["pos"], c["desc"]) as m:
        assert_same(ctx.map_fuse(m, c["frames"], K, COLS, ROWS, max_px=3.0, max_hamming=50), c["want"], RULE, "explicit defaults")


def test_errors(mvo, ctx):
    c = case(65, 3)
    n, F = 65, 3
    k = [K[name] for name in ("fx", "fy", "cx", "cy")]
    idx, dist = np.full((F, n, 2), 77, np.int32), np.full((F, n, 2), 77, np.int32)
    cnt, px = np.full((F, n), 77, np.int32), np.full((F, n, 2), 77, np.float32)
    rep, added, n_added, counts = np.full(n, 77, np.int32), np.full((1000, 3), 77, np.int32), C.c_int(77), np.full(6, 77, np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def untouched():
        return all((a == 77).all() for a in (idx, dist, cnt, px, rep, added, counts))

    with resident(ctx, c["pos"], c["desc"]) as m:
        def both(frames, n_frames=None, map_=m, kk=k, cols=COLS, rows=ROWS, max_px=3.0, max_hamming=50, outs=True, search=True):
            """The two entry points on the same bad input -> their codes (which must agree)."""
            arr, _, keep = ctx._fuse_frames(frames) if frames is not None else (None, None, None)
            nf = len(frames) if n_frames is None else n_frames
            kc = [C.c_double(v) for v in kk]
            a = search and ctx.lib.mvo_map_fuse_search(ctx.h, map_, arr, nf, *kc, cols, rows, C.c_double(max_px), p(idx) if outs else None,
                                                       p(dist) if outs else None, p(cnt), p(px))
            params = C.byref(mvo.MapFuseParams(max_px, max_hamming))
            b = ctx.lib.mvo_map_fuse(ctx.h, map_, arr, nf, *kc, cols, rows, params, p(rep) if outs else None, p(added), 1000,
                                     C.byref(n_added), p(counts))
            assert n_added.value == 77
            return a, b

        INV, CAP = mvo.MVO_ERR_INVALID, mvo.MVO_ERR_CAPACITY
        frames = c["frames"]

        def changed(f, **kw):
            out = [dict(fr) for fr in frames]
            out[f].update(kw)
            return out

        assert both(frames, map_=None) == (INV, INV)                                           # a null map
        assert both(None, n_frames=3) == (INV, INV)                                            # null pointers with a positive count
        assert both(frames, outs=False) == (INV, INV)
        assert both(frames, n_frames=-1) == (INV, INV)
        for field in ("desc", "xy", "conn"):
            arr, _, keep = ctx._fuse_frames(frames)
            setattr(arr[0], field, None)
            kc = [C.c_double(v) for v in k]
            assert ctx.lib.mvo_map_fuse_search(ctx.h, m, arr, F, *kc, COLS, ROWS, C.c_double(3.0), p(idx), p(dist), p(cnt), p(px)) == INV
            assert ctx.lib.mvo_map_fuse(ctx.h, m, arr, F, *kc, COLS, ROWS, None, p(rep), p(added), 1000, C.byref(n_added), p(counts)) == INV
        arr, _, keep = ctx._fuse_frames(frames)
        arr[1].n = -1
        assert ctx.lib.mvo_map_fuse_search(ctx.h, m, arr, F, *[C.c_double(v) for v in k], COLS, ROWS, C.c_double(3.0), p(idx), p(dist),
                                           p(cnt), p(px)) == INV
        for v in (-3, n):                                                                      # a conn outside [-2, n_map)
            conn = frames[0]["conn"].copy()
            conn[5] = v
            assert both(changed(0, conn=conn)) == (INV, INV)
        for v in (np.nan, np.inf):                                                             # a non-finite pose, a singular pose
            T = frames[2]["T"].copy()
            T[1, 3] = v
            assert both(changed(2, T=T)) == (INV, INV)
        T = frames[1]["T"].copy()
        T[:3, :3] = 0
        assert both(changed(1, T=T)) == (INV, INV)
        for bad in ([0.0, k[1], k[2], k[3]], [k[0], 0.0, k[2], k[3]], [k[0], k[1], np.nan, k[3]], [np.inf, k[1], k[2], k[3]]):
            assert both(frames, kk=bad) == (INV, INV)
        assert both(frames, cols=0) == (INV, INV) and both(frames, rows=-4) == (INV, INV)
        assert both(frames, max_px=-0.5) == (INV, INV) and both(frames, max_px=float("nan")) == (INV, INV)
        for v in (-1.0, np.nan, np.inf):                                                       # a bad scale entry
            scale = np.ones(len(frames[0]["desc"]), np.float32)
            scale[7] = v
            assert both(changed(0, scale=scale)) == (INV, INV)
        for v in (-1, 257):                                                                    # max_hamming outside 0..256
            assert both(frames, max_hamming=v, search=False)[1] == INV
        with pytest.raises(mvo.MvoError) as e:
            ctx.map_fuse(m, frames, K, COLS, ROWS, max_hamming=300)
        assert e.value.code == INV
        assert untouched()
        # MVO_ERR_CAPACITY: 65 frames; a frame with 65536 keypoints; cap_added too small (*n_added is set, nothing else written)
        assert both([frames[2]] * 65) == (CAP, CAP)
        big = dict(desc=np.zeros((65536, 32), np.uint8), xy=np.zeros((65536, 2), np.float32), conn=np.full(65536, -1, np.int32),
                   scale=None, T=np.eye(4))
        assert both([frames[0], big]) == (CAP, CAP)
        with pytest.raises(mvo.MvoError) as e:
            ctx.map_fuse_search(m, [big], K, COLS, ROWS, 3.0)
        assert e.value.code == CAP
        assert untouched()
        arr, _, keep = ctx._fuse_frames(frames)
        n_want = len(c["want"][1])
        assert n_want > 1
        assert ctx.lib.mvo_map_fuse(ctx.h, m, arr, F, *[C.c_double(v) for v in k], COLS, ROWS, None, p(rep), p(added), n_want - 1,
                                    C.byref(n_added), p(counts)) == CAP
        assert n_added.value == n_want and untouched()
        assert ctx.lib.mvo_map_fuse(ctx.h, m, arr, F, *[C.c_double(v) for v in k], COLS, ROWS, None, p(rep), p(added), n_want,
                                    C.byref(n_added), p(counts)) == mvo.MVO_OK
        assert rep.tobytes() == c["want"][0].tobytes() and added[:n_want].tobytes() == c["want"][1].tobytes()
        assert (added[n_want:] == 77).all() and counts.tobytes() == c["want"][2].tobytes()
        # the optional outputs of the search
        assert ctx.lib.mvo_map_fuse_search(ctx.h, m, arr, F, *[C.c_double(v) for v in k], COLS, ROWS, C.c_double(3.0), p(idx), p(dist),
                                           None, None) == mvo.MVO_OK
        assert idx.tobytes() == c["raw"][0].tobytes() and dist.tobytes() == c["raw"][1].tobytes() and (cnt == 77).all() and (px == 77).all()
        # no frames: nothing to search, every point stands for itself
        got = ctx.map_fuse(m, [], K, COLS, ROWS)
        assert (got[0] == np.arange(n)).all() and len(got[1]) == 0 and not got[2].any()
        assert [a.shape for a in ctx.map_fuse_search(m, [], K, COLS, ROWS, 3.0)] == [(0, n, 2), (0, n, 2), (0, n), (0, n, 2)]
        # frames without keypoints: rows of points in view with no candidates
        empty = dict(desc=np.zeros((0, 32), np.uint8), xy=np.zeros((0, 2), np.float32), conn=np.zeros(0, np.int32), scale=None, T=np.eye(4))
        got = ctx.map_fuse_search(m, [empty, empty], K, COLS, ROWS, 3.0)
        assert_same(got, M.search(c["pos"], c["desc"], [empty, empty], K, COLS, ROWS, 3.0), RAW, "two empty frames")
        assert (got[2] == 0).any() and (got[0] == -1).all()
    # an empty map succeeds (without a launch: there is nothing to write)
    with resident(ctx, np.zeros((0, 3), np.float32), np.zeros((0, 32), np.uint8)) as m:
        free = [dict(fr, conn=np.where(fr["conn"] >= 0, -1, fr["conn"]).astype(np.int32)) for fr in c["frames"]]
        got = ctx.map_fuse(m, free, K, COLS, ROWS)
        assert len(got[0]) == 0 and len(got[1]) == 0 and not got[2].any()
        assert [a.shape for a in ctx.map_fuse_search(m, free, K, COLS, ROWS, 3.0)] == [(3, 0, 2), (3, 0, 2), (3, 0), (3, 0, 2)]
        with pytest.raises(mvo.MvoError) as e:      # ... and a connection into it is outside [-2, 0)
            ctx.map_fuse(m, c["frames"], K, COLS, ROWS)
        assert e.value.code == mvo.MVO_ERR_INVALID
