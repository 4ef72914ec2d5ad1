"""The map-point position refinement on the MI355X (csrc/map_refine_kernels.hip, csrc/map_refine_host.cpp) against its numpy
transcription (tests/map_refine_numpy.py; known answers of its own in tests/test_map_refine_numpy.py), bit for bit: the positions
reported and the positions resident in HBM, chi2 before and after, status / accepted steps / trials, the outlier flags; over the
workgroup's four waves, observation counts from 0 to 64, 1 to 64 frames, every status; a repeated call, moved positions, the
matcher that reads the refined positions, non-default parameters, every error code.  tests/test_map_refine_sim.py runs the same
functions on the emulated build."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import map_refine_numpy as R
import projection_numpy as P

pytestmark = pytest.mark.gpu

# (map points, frames): every n of 1, 3, 4, 5, 65, 257 and every n_frames of 1, 2, 20, 64
CASES = [(1, 1), (3, 2), (4, 1), (5, 64), (65, 20), (65, 2), (257, 64), (257, 20)]
COLS, ROWS = 640, 480
# the TUM fr1 intrinsics rounded to f32: a pixel (cx, cy) is then a value an observation can carry exactly
K = {k: float(np.float32(v)) for k, v in R.FR1_K.items()}


@contextlib.contextmanager
def resident(ctx, pos, desc=None):
    m = ctx.map_create()
    try:
        ctx.map_upload(m, pos, np.zeros((len(pos), 32), np.uint8) if desc is None else desc)
        yield m
    finally:
        ctx.map_release(m)


@functools.lru_cache(maxsize=None)
def case(n, n_frames, counts=None, params=()):
    """Inputs and the transcription's answer; computed once, read-only.  0.5 px noise, every fifth point with an observation
    moved by (40, -30) px.  With n >= 65: every ninth point starts 60 % too deep (failed trials before an accepted one), every
    13th behind the cameras (status 2), every 17th sits on the optical axis of frame 0 and is seen there only, at exactly
    (cx, cy): chi2 = 0 and b = 0 in f64, no trial can lower it (status 3)."""
    rng = np.random.RandomState(1000 * n + n_frames + (sum(counts) if counts else 0))
    if counts is None:
        counts = rng.randint(0, 21, n)
        counts[6::7] = 63 + (np.arange(len(counts[6::7])) % 2)      # every seventh point: 63, 64, 63 ...
    step, yaw = (0.03, 0.01) if n_frames == 20 else (0.57 / max(n_frames - 1, 1), 0.19 / max(n_frames - 1, 1))
    truth, pos, T, frame, uv, start, moved = R.scene(rng, list(counts), n_frames, 0.5, 5, K=K, step=step, yaw=yaw)
    pos, frame, uv = pos.copy(), frame.copy(), uv.copy()
    if n >= 65:
        far, behind, exact = np.arange(8, n, 9), np.arange(10, n, 13), np.arange(12, n, 17)
        pos[far] = (truth[far] * np.array([1.0, 1.0, 1.6])).astype(np.float32)
        pos[behind, 2] = -pos[behind, 2]
        for i in exact:
            pos[i] = (0.0, 0.0, 1.0)
            frame[start[i]:start[i + 1]] = 0
            uv[start[i]:start[i + 1]] = (K["cx"], K["cy"])
    traces = {}
    want = R.refine(pos, T, K, frame, uv, start, dict(params), traces)
    for a in (truth, pos, T, frame, uv, start, moved) + want:
        a.setflags(write=False)
    return dict(truth=truth, pos=pos, T=T, frame=frame, uv=uv, start=start, moved=moved, want=want, traces=traces)


def call(ctx, m, c, **kw):
    return ctx.map_refine_positions(m, c["T"], K, c["frame"], c["uv"], c["start"], **kw)


def assert_equal(got, want, what):
    for name, g, w in zip(("pos_out", "chi2", "info", "obs_outlier"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s is %s %s" % (what, name, g.dtype, g.shape)
        if g.tobytes() != w.tobytes():
            bad = np.nonzero((g.reshape(len(g), -1) != w.reshape(len(w), -1)).any(1))[0]
            raise AssertionError("%s: %s differs by its bits at %d rows, first %d: %r vs %r" % (what, name, len(bad), bad[0], g[bad[0]], w[bad[0]]))


@pytest.mark.parametrize("n,n_frames", CASES)
def test_refine_bit_exact(ctx, n, n_frames):
    c = case(n, n_frames)
    want, m_i = c["want"], np.diff(c["start"])
    status = want[2][:, 0]
    if n >= 65:    # the case is not vacuous
        assert ((status == 0) & (want[2][:, 1] >= 3)).any(), "no refined point with three accepted steps"
        assert all((status == s).any() for s in (1, 2, 3)), "a status is missing: %r" % np.bincount(status, minlength=4)
        assert any(R.failed_then_accepted(t) for t in c["traces"].values()), "no failed trial followed by an accepted one"
        assert (m_i == 64).any() and (m_i == 63).any() and (m_i == 0).any()
        assert want[3][c["moved"][(c["moved"] >= 0) & (status == 0)]].all(), "a moved observation is not flagged"
    with resident(ctx, c["pos"]) as m:
        assert_equal(call(ctx, m, c), want, "%d points, %d frames" % (n, n_frames))
        rpos, rdesc = ctx.map_debug_get(m)
        assert rpos.tobytes() == want[0].tobytes(), "the resident positions are not the refined ones"
        assert rpos[status != 0].tobytes() == c["pos"][status != 0].tobytes() and not rdesc.any()
        assert (rpos[status == 0] != c["pos"][status == 0]).any(1).all()


@pytest.mark.parametrize("m_obs", [2, 64])
def test_a_single_point_with_2_and_64_observations(ctx, m_obs):
    c = case(1, 20, (m_obs,))
    assert c["want"][2][0, 0] == 0
    with resident(ctx, c["pos"]) as m:
        assert_equal(call(ctx, m, c), c["want"], "one point, %d observations" % m_obs)
        assert ctx.map_debug_get(m)[0].tobytes() == c["want"][0].tobytes()


def test_parameters_other_than_the_defaults(ctx):
    params = dict(max_trials=3, min_observations=4, huber_delta=1e9, rel_tolerance=0.0)
    c, d = case(65, 20, None, tuple(sorted(params.items()))), case(65, 20)
    assert c["want"][2][:, 2].max() == 3 and (c["want"][2][:, 0] == 1).sum() > (d["want"][2][:, 0] == 1).sum() and not c["want"][3].any()
    with resident(ctx, c["pos"]) as m:
        assert_equal(call(ctx, m, c, **params), c["want"], "max_trials 3, min_observations 4, huber_delta 1e9, rel_tolerance 0")


def test_a_second_call_starts_from_the_refined_positions(ctx):
    c = case(257, 20)
    second = R.refine(c["want"][0], c["T"], K, c["frame"], c["uv"], c["start"])
    assert second[0].tobytes() != c["want"][0].tobytes()      # (it starts from the f32 store of the first call's f64 result)
    with resident(ctx, c["pos"]) as m:
        assert_equal(call(ctx, m, c), c["want"], "first call")
        assert_equal(call(ctx, m, c), second, "second call")
        assert ctx.map_debug_get(m)[0].tobytes() == second[0].tobytes()


def test_moved_positions_are_what_the_next_call_starts_from(ctx):
    c = case(65, 20)
    moved = c["want"][0].copy()
    moved[10:30] = c["pos"][10:30] * np.float32(1.01)
    want_moved = R.refine(moved, c["T"], K, c["frame"], c["uv"], c["start"])
    assert want_moved[2].tobytes() != c["want"][2].tobytes()
    with resident(ctx, c["pos"]) as m:
        assert_equal(call(ctx, m, c), c["want"], "before the move")
        ctx.map_update_positions(m, moved[10:30], first=10)
        assert_equal(call(ctx, m, c), want_moved, "after the move")
        assert ctx.map_debug_get(m)[0].tobytes() == want_moved[0].tobytes()


def test_the_projection_matcher_projects_the_refined_positions(ctx):
    """The matcher of tracking by projection reads the same resident array: its px follows the refinement."""
    c = case(65, 20)
    T = c["T"][10]
    t, txy = np.zeros((1, 32), np.uint8), np.zeros((1, 2), np.float32)
    before, after = (P.project_map(p, T, K, COLS, ROWS) for p in (c["pos"], c["want"][0]))
    changed = (c["want"][2][:, 0] == 0) & before[2] & after[2]
    assert changed.sum() > 30 and ((before[0] != after[0]) | (before[1] != after[1]))[changed].all()
    with resident(ctx, c["pos"]) as m:
        px = ctx.map_match_knn2_projection(m, T, K, COLS, ROWS, t, txy, 0.5)[0]
        assert px[before[2]].tobytes() == np.stack([before[0], before[1]], 1)[before[2]].tobytes()
        call(ctx, m, c)
        px = ctx.map_match_knn2_projection(m, T, K, COLS, ROWS, t, txy, 0.5)[0]
        assert px[after[2]].tobytes() == np.stack([after[0], after[1]], 1)[after[2]].tobytes()


def _raw(ctx, m, T, n_frames, k, frame, uv, start, n_obs, params, pos, chi2, info, flags):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return ctx.lib.mvo_map_refine_positions(ctx.h, m, p(T), int(n_frames), *[C.c_double(v) for v in k], p(frame), p(uv), p(start),
                                            int(n_obs), params, p(pos), p(chi2), p(info), p(flags))


def test_errors(mvo, ctx):
    c = case(5, 64)
    n, n_obs, n_frames = 5, len(c["uv"]), 64
    assert n_obs > 0
    T = np.ascontiguousarray(c["T"], np.float64)
    k = [K[name] for name in ("fx", "fy", "cx", "cy")]
    pos, chi2, info, flags = np.full((n, 3), 77, np.float32), np.full((n, 2), 77.0), np.full((n, 3), 77, np.int32), np.full(n_obs, 77, np.uint8)

    with resident(ctx, c["pos"]) as m:
        def untouched():
            return ((pos == 77).all() and (chi2 == 77.0).all() and (info == 77).all() and (flags == 77).all()
                    and ctx.map_debug_get(m)[0].tobytes() == c["pos"].tobytes())

        base = [T, n_frames, k, c["frame"], c["uv"], c["start"], n_obs, None, pos, chi2, info, flags]

        def code(**kw):
            a = list(base)
            for name, v in kw.items():
                a[("T", "n_frames", "k", "frame", "uv", "start", "n_obs", "params", "pos", "chi2", "info", "flags").index(name)] = v
            return _raw(ctx, m, *a)

        assert _raw(ctx, None, *base) == mvo.MVO_ERR_INVALID                                  # a null map
        for name in ("T", "frame", "uv", "start", "pos", "chi2", "info"):                     # a null pointer with a positive count
            assert code(**{name: None}) == mvo.MVO_ERR_INVALID, name
        assert code(n_obs=-1) == mvo.MVO_ERR_INVALID and code(n_frames=-1) == mvo.MVO_ERR_INVALID
        start = c["start"]
        for bad in (start + 1, np.r_[start[:-1], start[-1] - 1], np.r_[start[:-1], start[-1] + 1], np.array([0, 3, 2, n_obs, n_obs, n_obs])):
            assert code(start=np.ascontiguousarray(bad, np.int32)) == mvo.MVO_ERR_INVALID
        for v in (-1, n_frames):                                                              # obs_frame outside [0, n_frames)
            frame = c["frame"].copy()
            frame[n_obs - 1] = v
            assert code(frame=frame) == mvo.MVO_ERR_INVALID
        assert code(n_frames=int(c["frame"].max())) == mvo.MVO_ERR_INVALID                    # ... the same from the other side
        for v in (np.nan, np.inf):                                                            # a non-finite pose, a singular pose
            Tb = T.copy()
            Tb[3, 1, 3] = v
            assert code(T=Tb) == mvo.MVO_ERR_INVALID
        Tb = T.copy()
        Tb[5, :3, :3] = 0
        assert code(T=Tb) == mvo.MVO_ERR_INVALID
        for bad in ([0.0, k[1], k[2], k[3]], [k[0], 0.0, k[2], k[3]], [k[0], k[1], np.nan, k[3]], [np.inf, k[1], k[2], k[3]]):
            assert code(k=bad) == mvo.MVO_ERR_INVALID
        for v in (np.nan, np.inf, -np.inf):                                                   # a non-finite pixel
            uv = c["uv"].copy()
            uv[n_obs - 1, 1] = v
            assert code(uv=uv) == mvo.MVO_ERR_INVALID
        d = float(np.sqrt(5.991))
        for bad in ((0, 2, d, 1e-6), (65, 2, d, 1e-6), (20, 1, d, 1e-6), (20, 65, d, 1e-6), (20, 2, 0.0, 1e-6), (20, 2, -1.0, 1e-6),
                    (20, 2, np.inf, 1e-6), (20, 2, np.nan, 1e-6), (20, 2, d, -1e-9), (20, 2, d, np.inf), (20, 2, d, np.nan)):
            assert code(params=C.byref(mvo.MapRefineParams(*bad))) == mvo.MVO_ERR_INVALID, bad
        with pytest.raises(mvo.MvoError) as e:
            ctx.map_refine_positions(m, T, K, c["frame"], c["uv"], c["start"], max_trials=0)
        assert e.value.code == mvo.MVO_ERR_INVALID
        assert untouched()
        # MVO_ERR_CAPACITY: 65 frames; a point with 65 observations
        T65 = np.concatenate([T, T[:1]])
        assert code(T=T65, n_frames=65) == mvo.MVO_ERR_CAPACITY
        s65 = np.array([0, 2, 67, 70, 70, 71], np.int32)
        f65, uv65 = np.zeros(71, np.int32), np.full((71, 2), 100, np.float32)
        assert code(frame=f65, uv=uv65, start=s65, n_obs=71, flags=np.full(71, 77, np.uint8)) == mvo.MVO_ERR_CAPACITY
        with pytest.raises(mvo.MvoError) as e:
            ctx.map_refine_positions(m, T, K, f65, uv65, s65)
        assert e.value.code == mvo.MVO_ERR_CAPACITY
        assert untouched()
        # obs_outlier is optional; explicit default parameters are the defaults
        assert code(flags=None, params=C.byref(mvo.MapRefineParams(20, 2, d, 1e-6))) == mvo.MVO_OK
        assert pos.tobytes() == c["want"][0].tobytes() and chi2.tobytes() == c["want"][1].tobytes() and info.tobytes() == c["want"][2].tobytes()
        assert (flags == 77).all() and ctx.map_debug_get(m)[0].tobytes() == c["want"][0].tobytes()
        # n_obs == 0 succeeds: every status 1, nothing moves
        held = ctx.map_debug_get(m)[0]
        got = ctx.map_refine_positions(m, T, K, np.zeros(0, np.int32), np.zeros((0, 2), np.float32), np.zeros(n + 1, np.int32))
        assert (got[2] == [1, 0, 0]).all() and got[0].tobytes() == held.tobytes() and not got[1].any() and len(got[3]) == 0
        assert code(T=None, n_frames=0, frame=None, uv=None, start=np.zeros(n + 1, np.int32), n_obs=0) == mvo.MVO_OK
    # an empty map succeeds (without a launch: there is nothing to write)
    with resident(ctx, np.zeros((0, 3), np.float32)) as m:
        got = ctx.map_refine_positions(m, T, K, np.zeros(0, np.int32), np.zeros((0, 2), np.float32), np.zeros(1, np.int32))
        assert [len(a) for a in got] == [0, 0, 0, 0]
        assert _raw(ctx, m, None, 0, k, None, None, None, 0, None, None, None, None, None) == mvo.MVO_OK
        assert _raw(ctx, m, T, n_frames, k, c["frame"], c["uv"], c["start"], n_obs, None, pos, chi2, info, None) == mvo.MVO_ERR_INVALID
