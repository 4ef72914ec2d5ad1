"""The robust motion-only pose optimisation on the MI355X (csrc/pose_optimize_kernels.hip, csrc/pose_optimize_host.cpp) against
its numpy transcription (tests/pose_optimize_numpy.py; known answers of its own in tests/test_pose_optimize_numpy.py), bit for
bit: T_w_c, T_c_w, the outlier flags, chi2, info and the per-round rows of the debug getter; over the edges of a wave (63, 64,
65), of the slot stride (255, 256, 257), of two strides (511, 513), the smallest useful problem (10) and the capacity (4096),
each with moved observations and points behind the camera, with and without inv_sigma2; non-default parameters, every status, a
second call with fewer observations, every error code.  tests/test_pose_optimize_sim.py runs the same functions on the emulated
build.

With the default rel_tolerance the Huber-weighted Levenberg-Marquardt never rejects a trial on these scenes (from 2 degrees to
35 degrees of initial error, near points, planes, narrow fields of view: the transcription accepted every trial), so every
shape also runs with rel_tolerance 0 and 32 trials per round: past convergence trials fail by rounding and a later, more damped
one is accepted again.  The guard of a shape reads the traces of its three runs together."""
import ctypes as C
import functools

import numpy as np
import pytest

import pose_optimize_numpy as R

pytestmark = pytest.mark.gpu

SHAPES = [10, 63, 64, 65, 255, 256, 257, 511, 513, 4096]
# the TUM fr1 intrinsics rounded to f32
K = {k: float(np.float32(v)) for k, v in R.FR1_K.items()}
PAST_CONVERGENCE = dict(rel_tolerance=0.0, iterations=32)
NAMES = ("T_w_c", "T_c_w", "outlier", "chi2", "info", "rows")


def frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


def base_params(n):
    return dict(min_inliers=6) if n == 10 else {}       # (ten observations, three of them outliers: the default would stop)


@functools.lru_cache(maxsize=None)
def scene(n, moved_every=5, seed=0):
    """0.5 px noise, every fifth observation moved by (40, -30) px, the last three points (one for n = 10) behind the camera, a
    start 2 degrees and about 5 % of the depth away; inv_sigma2 = 1 / 1.2^(2 level), level 0..7.  Computed once, read-only."""
    rng = np.random.RandomState(7919 * n + seed)
    p3, p2, T, moved, behind = R.scene(rng, n, 0.5, moved_every, 1 if n == 10 else 3)
    scale = np.float32(1.2) ** rng.randint(0, 8, n).astype(np.float32)
    sigma = (1.0 / (scale.astype(np.float64) * scale.astype(np.float64))).astype(np.float32)
    T_init = R.perturbed(T, 2.0, (0.1, -0.1, 0.15))
    frozen(p3, p2, T, moved, behind, sigma, T_init)
    return dict(p3=p3, p2=p2, T=T, moved=moved, behind=behind, sigma=sigma, T_init=T_init)


@functools.lru_cache(maxsize=None)
def answer(n, with_sigma, params=(), moved_every=5, seed=0):
    s = scene(n, moved_every, seed)
    traces = []
    want = R.optimize_pose(s["p3"], s["p2"], s["sigma"] if with_sigma else None, s["T_init"], K, dict(params), traces)
    frozen(*want)
    return want, traces


def key(params):
    return tuple(sorted(params.items()))


def call(ctx, s, with_sigma, params):
    got = ctx.optimize_pose(s["p3"], s["p2"], s["T_init"], K, s["sigma"] if with_sigma else None, **params)
    return got + (ctx.pose_optimize_debug_get(),)


def assert_equal(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        w = np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s is %s %s, not %s %s" % (what, name, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            raise AssertionError("%s: %s differs by its bits:\n%r\nvs\n%r" % (what, name, g, w))


@functools.lru_cache(maxsize=None)
def shape_seed(n):
    """The first seed whose scene makes the transcription reject a trial and accept a later one in the run past convergence
    (whether rounding does that depends on the noise drawn)."""
    p = key(dict(base_params(n), **PAST_CONVERGENCE))
    return next(seed for seed in range(50) if any(R.failed_then_accepted(t) for t in answer(n, True, p, 5, seed)[1]))


@pytest.mark.parametrize("n", SHAPES)
def test_shapes_bit_exact(ctx, n):
    seed = shape_seed(n)
    s = scene(n, 5, seed)
    runs = [(False, base_params(n)), (True, base_params(n)), (True, dict(base_params(n), **PAST_CONVERGENCE))]
    answers = [answer(n, sg, key(p), 5, seed) for sg, p in runs]
    # the case is not vacuous
    assert any(R.failed_then_accepted(t) for _, traces in answers for t in traces), "no failed trial followed by an accepted one"
    for want, _ in answers:
        assert want[4][0] == R.OPTIMISED and want[4][1] == 4
        assert (want[5][:, 5] != want[5][:, 0]).any(), "no round changes the inlier set"
        assert set(np.nonzero(want[2])[0]) == set(s["moved"]) | set(s["behind"]), "the flags are not the moved and the hidden"
        assert want[4][5] == n - len(s["behind"])
    for (sg, p), (want, _) in zip(runs, answers):
        assert_equal(call(ctx, s, sg, p), want, "%d observations, inv_sigma2 %s, %r" % (n, sg, p))


PARAMS = [dict(rounds=1), dict(rounds=8), dict(iterations=1), dict(rel_tolerance=0.0), dict(huber_delta=1e9),
          dict(rounds=2, iterations=3, min_inliers=100, chi2_threshold=2.0, huber_delta=1.0, rel_tolerance=1e-3)]


@pytest.mark.parametrize("params", PARAMS, ids=lambda p: "-".join("%s=%g" % kv for kv in sorted(p.items())))
def test_parameters_other_than_the_defaults(ctx, params):
    n = 257
    want, traces = answer(n, True, key(params))
    dflt, _ = answer(n, True)
    if params == dict(huber_delta=1e9):     # no kernel in any round: the moved fifth drags the pose and the loop stops early
        assert want[4][0] == R.FEW_INLIERS and not any(R.failed_then_accepted(t) for t in traces)
    else:
        assert want[4][1] == params.get("rounds", 4)
    if "iterations" in params:
        assert (want[5][:, 3] == params["iterations"]).all()
    if params == dict(rel_tolerance=0.0):
        assert (want[5][:, 3] == 10).all() and any(not all(t) for t in traces)
    if params != dict(rounds=8):
        assert any(np.ascontiguousarray(w).tobytes() != np.ascontiguousarray(d).tobytes() for w, d in zip(want, dflt))
    assert_equal(call(ctx, scene(n), True, params), want, repr(params))


def test_every_status(ctx):
    # 1: every second observation moved, 9 of 18 left
    s = scene(18, 2)
    want, _ = answer(18, False, (), 2)
    assert want[4][0] == R.FEW_INLIERS and want[4][4] < 10 and want[4][1] >= 1
    assert_equal(call(ctx, s, False, {}), want, "status 1")
    # 2: all but nine points behind the camera; the pose comes back bit for bit
    rng = np.random.RandomState(3)
    p3, p2, T, _, behind = R.scene(rng, 40, 0.5, 0, 31)
    T_init = R.perturbed(T, 0.5, (0.01, 0.0, 0.0))
    want = R.optimize_pose(p3, p2, None, T_init, K)
    assert want[4].tolist() == [R.FEW_IN_FRONT, 0, 0, 0, 0, 9] and want[2].all() and want[0].tobytes() == T_init.tobytes()
    got = ctx.optimize_pose(p3, p2, T_init, K) + (ctx.pose_optimize_debug_get(),)
    assert_equal(got, want, "status 2")
    # 3: a start that is stationary in f64
    p3, p2, T, Kd = R.stationary_scene()
    want = R.optimize_pose(p3, p2, None, T, Kd)
    assert want[4].tolist() == [R.NO_STEP, 4, 40, 0, 40, 40] and not want[2].any() and not want[3].any()
    got = ctx.optimize_pose(p3, p2, T, Kd) + (ctx.pose_optimize_debug_get(),)
    assert_equal(got, want, "status 3")
    # 0 is every case of test_shapes_bit_exact


def test_a_second_call_with_fewer_observations(ctx):
    """Nothing of the first call's staging (flags, rows of rounds that the second call does not run) shows in the second."""
    first, _ = answer(513, True)
    second, _ = answer(63, False, key(dict(rounds=2)))
    assert second[4][1] == 2 < first[4][1]
    assert_equal(call(ctx, scene(513), True, {}), first, "first call")
    assert_equal(call(ctx, scene(63), False, dict(rounds=2)), second, "second call")
    assert_equal(call(ctx, scene(513), True, {}), first, "third call")


def _raw(ctx, p3, p2, sg, n, T0, k, params, Twc, Tcw, flags, chi2, info):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return ctx.lib.mvo_optimize_pose(ctx.h, p(p3), p(p2), p(sg), int(n), p(T0), *[C.c_double(v) for v in k], params, p(Twc), p(Tcw),
                                     p(flags), p(chi2), p(info))


def test_errors(mvo, ctx):
    s = scene(65)
    n = 65
    want, _ = answer(n, True)
    k = [K[name] for name in ("fx", "fy", "cx", "cy")]
    T0 = np.ascontiguousarray(s["T_init"], np.float64)
    Twc, Tcw, flags = np.full((4, 4), 77.0), np.full((4, 4), 77.0), np.full(n, 77, np.uint8)
    chi2, info = np.full(2, 77.0), np.full(6, 77, np.int32)
    order = ("p3", "p2", "sg", "n", "T0", "k", "params", "Twc", "Tcw", "flags", "chi2", "info")
    base = [s["p3"], s["p2"], s["sigma"], n, T0, k, None, Twc, Tcw, flags, chi2, info]

    def untouched():
        return (Twc == 77).all() and (Tcw == 77).all() and (flags == 77).all() and (chi2 == 77).all() and (info == 77).all()

    def code(**kw):
        a = list(base)
        for name, v in kw.items():
            a[order.index(name)] = v
        return _raw(ctx, *a)

    for name in ("p3", "p2", "T0", "Twc", "flags", "chi2", "info"):                           # a null pointer with a positive count
        assert code(**{name: None}) == mvo.MVO_ERR_INVALID, name
    assert code(n=-1) == mvo.MVO_ERR_INVALID
    for v in (np.nan, np.inf):                                                                # a non-finite pose, a singular pose
        Tb = T0.copy()
        Tb[1, 3] = v
        assert code(T0=Tb) == mvo.MVO_ERR_INVALID
    Tb = T0.copy()
    Tb[:3, :3] = 0
    assert code(T0=Tb) == mvo.MVO_ERR_INVALID
    for bad in ([0.0, k[1], k[2], k[3]], [k[0], 0.0, k[2], k[3]], [k[0], k[1], np.nan, k[3]], [np.inf, k[1], k[2], k[3]],
                [k[0], k[1], k[2], -np.inf]):
        assert code(k=bad) == mvo.MVO_ERR_INVALID
    for v in (np.nan, np.inf, -np.inf):                                                       # a non-finite point or pixel
        for name, a in (("p3", s["p3"]), ("p2", s["p2"])):
            b = a.copy()
            b[n - 1, 1] = v
            assert code(**{name: b}) == mvo.MVO_ERR_INVALID
    for v in (-1e-6, np.nan, np.inf):                                                         # a negative or non-finite weight
        b = s["sigma"].copy()
        b[n - 1] = v
        assert code(sg=b) == mvo.MVO_ERR_INVALID
    d = float(np.sqrt(5.991))
    for bad in ((0, 10, 10, 5.991, d, 1e-6), (9, 10, 10, 5.991, d, 1e-6), (4, 0, 10, 5.991, d, 1e-6), (4, 65, 10, 5.991, d, 1e-6),
                (4, 10, 5, 5.991, d, 1e-6), (4, 10, 4097, 5.991, d, 1e-6), (4, 10, 10, 0.0, d, 1e-6), (4, 10, 10, np.inf, d, 1e-6),
                (4, 10, 10, np.nan, d, 1e-6), (4, 10, 10, 5.991, 0.0, 1e-6), (4, 10, 10, 5.991, -1.0, 1e-6),
                (4, 10, 10, 5.991, np.inf, 1e-6), (4, 10, 10, 5.991, np.nan, 1e-6), (4, 10, 10, 5.991, d, -1e-9),
                (4, 10, 10, 5.991, d, np.inf), (4, 10, 10, 5.991, d, np.nan)):
        assert code(params=C.byref(mvo.PoseOptimizeParams(*bad))) == mvo.MVO_ERR_INVALID, bad
    with pytest.raises(mvo.MvoError) as e:
        ctx.optimize_pose(s["p3"], s["p2"], T0, K, rounds=0)
    assert e.value.code == mvo.MVO_ERR_INVALID
    assert untouched()
    # MVO_ERR_CAPACITY: 4097 observations
    big3, big2 = np.ones((4097, 3), np.float32), np.ones((4097, 2), np.float32)
    assert code(p3=big3, p2=big2, sg=None, n=4097, flags=np.full(4097, 77, np.uint8)) == mvo.MVO_ERR_CAPACITY
    with pytest.raises(mvo.MvoError) as e:
        ctx.optimize_pose(big3, big2, T0, K)
    assert e.value.code == mvo.MVO_ERR_CAPACITY
    assert untouched()
    # T_c_w is optional; explicit default parameters are the defaults
    assert code(Tcw=None, params=C.byref(mvo.PoseOptimizeParams(4, 10, 10, 5.991, d, 1e-6))) == mvo.MVO_OK
    assert (Tcw == 77).all()
    for g, w in zip((Twc, flags, chi2, info), (want[0], want[2], want[3], want[4])):
        assert g.tobytes() == np.ascontiguousarray(w).tobytes()
    # n == 0 succeeds without a launch: status 2, the pose as given; the rows of the debug getter stay those of the last launch
    got = ctx.optimize_pose(np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32), T0, K)
    empty = R.optimize_pose(np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32), None, T0, K)
    assert_equal(got, empty[:5], "no observations")
    assert got[4].tolist() == [2, 0, 0, 0, 0, 0] and got[0].tobytes() == T0.tobytes()
    assert ctx.pose_optimize_debug_get().tobytes() == np.ascontiguousarray(want[5]).tobytes()
    assert _raw(ctx, None, None, None, 0, T0, k, None, Twc, None, None, chi2, info) == mvo.MVO_OK


def test_the_debug_getter_before_the_first_call(mvo):
    c = mvo.Context(0)
    try:
        with pytest.raises(mvo.MvoError) as e:
            c.pose_optimize_debug_get()
        assert e.value.code == mvo.MVO_ERR_STATE
    finally:
        c.close()
