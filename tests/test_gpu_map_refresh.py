"""The map-point refresh on the MI355X (csrc/map_refresh_kernels.hip, csrc/map_refresh_host.cpp) against its numpy
transcription (tests/map_refresh_numpy.py; known answers of its own in tests/test_map_refresh_numpy.py), bit for bit: the chosen
observation, the descriptors reported and the descriptors resident in HBM, the normals; over the workgroup's four waves, every
observation count from 0 to 64, ties decided by the index; moved positions, a repeated refresh, the matcher that reads the
refreshed descriptors, every error code.  tests/test_map_refresh_sim.py runs the same functions on the emulated build."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import map_refresh_numpy as R
import projection_numpy as P

pytestmark = pytest.mark.gpu

MAP_SIZES = [1, 3, 4, 5, 65, 257]
FLIP_RATES = [0.08, 0.02]
COLS, ROWS = 640, 480


@contextlib.contextmanager
def resident(ctx, pos, desc):
    m = ctx.map_create()
    try:
        ctx.map_upload(m, pos, desc)
        yield m
    finally:
        ctx.map_release(m)


def observations(rng, counts, flip, duplicate_every=5):
    """Per point a random base descriptor; every observation is the base with `flip` of its bits flipped; every fifth point
    (with two observations or more) gets one observation duplicated.  Camera centres around the origin."""
    obs_desc, start = [], [0]
    for i, m in enumerate(counts):
        base = rng.randint(0, 2, 256).astype(np.uint8)
        rows = [np.packbits(base ^ (rng.uniform(size=256) < flip).astype(np.uint8)) for _ in range(m)]
        if i % duplicate_every == duplicate_every - 1 and m >= 2:
            a, b = rng.choice(m, 2, replace=False)
            rows[a] = rows[b].copy()
        obs_desc += rows
        start.append(start[-1] + m)
    n_obs = start[-1]
    obs_desc = np.array(obs_desc, np.uint8).reshape(n_obs, 32)
    obs_cam = rng.uniform(-0.5, 0.5, (n_obs, 3))
    return obs_desc, obs_cam, np.array(start, np.int32)


def points_in_view(rng, n):
    """Points in front of a camera at the identity pose, well inside a 640 x 480 frame of the TUM fr1 intrinsics."""
    z = rng.uniform(2.0, 6.0, n)
    return np.stack([rng.uniform(-0.4, 0.4, n) * z, rng.uniform(-0.3, 0.3, n) * z, z], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(n, flip, counts=None):
    """Inputs and the transcription's answer.  Computed once, read-only."""
    rng = np.random.RandomState(100 * n + int(1000 * flip) + (sum(counts) if counts else 0))
    if counts is None:
        counts = rng.randint(0, 21, n)
        counts[6::7] = 63 + (np.arange(len(counts[6::7])) % 2)      # every seventh point: 63, 64, 63 ...
    pos = points_in_view(rng, n)
    desc = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    obs_desc, obs_cam, start = observations(rng, list(counts), flip)
    want = R.refresh(pos, desc, obs_desc, obs_cam, start)
    for a in (pos, desc, obs_desc, obs_cam, start) + want:
        a.setflags(write=False)
    return pos, desc, obs_desc, obs_cam, start, want


def assert_refresh_equal(got, want, what):
    for name, g, w in zip(("choice", "desc", "norm"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s is %s %s" % (what, name, g.dtype, g.shape)
    bad = np.nonzero(got[0] != want[0])[0]
    assert len(bad) == 0, "%s: choice differs at %d points, first %d: %d vs %d" % (what, len(bad), bad[0], got[0][bad[0]], want[0][bad[0]])
    assert got[1].tobytes() == want[1].tobytes(), "%s: desc_out differs" % what
    bad = [i for i in range(len(want[2])) if not R.same_f64(got[2][i], want[2][i])]
    assert not bad, "%s: norm_out differs by its bits at %d points, first %d: %r vs %r" % (what, len(bad), bad[0], got[2][bad[0]], want[2][bad[0]])


@pytest.mark.parametrize("flip", FLIP_RATES)
@pytest.mark.parametrize("n", MAP_SIZES)
def test_refresh_bit_exact(ctx, n, flip):
    pos, desc, obs_desc, obs_cam, start, want = case(n, flip)
    m_i = np.diff(start)
    if n >= 65:    # the case is not vacuous
        assert (want[0] > 0).any(), "no medoid other than observation 0"
        assert any(R.tie_decided(obs_desc, start, i) and want[0][i] >= 0 for i in range(n)), "no tie decided by the index"
        assert (m_i == 0).any() and (m_i == 64).any() and (m_i == 63).any()
    with resident(ctx, pos, desc) as m:
        got = ctx.map_refresh(m, obs_desc, obs_cam, start)
        assert_refresh_equal(got, want, "%d points, flip %g" % (n, flip))
        rpos, rdesc = ctx.map_debug_get(m)
        assert rpos.tobytes() == pos.tobytes(), "the resident positions changed"
        assert rdesc.tobytes() == want[1].tobytes(), "the resident descriptors are not the chosen observations"
        unseen = m_i == 0
        assert rdesc[unseen].tobytes() == desc[unseen].tobytes()


@pytest.mark.parametrize("m_obs", [1, 2, 64])
def test_a_single_point_with_1_2_64_observations(ctx, m_obs):
    pos, desc, obs_desc, obs_cam, start, want = case(1, 0.08, (m_obs,))
    assert want[0][0] == 0 if m_obs <= 2 else want[0][0] >= 0
    with resident(ctx, pos, desc) as m:
        assert_refresh_equal(ctx.map_refresh(m, obs_desc, obs_cam, start), want, "one point, %d observations" % m_obs)
        assert ctx.map_debug_get(m)[1].tobytes() == want[1].tobytes()


def test_a_camera_at_the_point_gives_nan_written_as_it_comes(ctx):
    pos, desc, obs_desc, obs_cam, start, _ = case(5, 0.08)
    i = int(np.argmax(np.diff(start) >= 2))
    assert np.diff(start)[i] >= 2
    cam = obs_cam.copy()
    cam[start[i] + 1] = pos[i].astype(np.float64)          # the second observation of point i was taken AT the point
    want = R.refresh(pos, desc, obs_desc, cam, start)
    assert np.isnan(want[2][i]).all() and np.isfinite(np.delete(want[2], i, 0)).all()
    with resident(ctx, pos, desc) as m:
        assert_refresh_equal(ctx.map_refresh(m, obs_desc, cam, start), want, "a camera at the point")


def test_moved_positions_are_what_the_next_refresh_uses(ctx):
    pos, desc, obs_desc, obs_cam, start, want = case(65, 0.08)
    moved = pos.copy()
    moved[10:30] += np.float32([0.25, -0.125, 0.5])
    want_moved = R.refresh(moved, desc, obs_desc, obs_cam, start)
    assert not R.same_f64(want_moved[2], want[2])
    with resident(ctx, pos, desc) as m:
        assert_refresh_equal(ctx.map_refresh(m, obs_desc, obs_cam, start), want, "before the move")
        ctx.map_update_positions(m, moved[10:30], first=10)
        assert_refresh_equal(ctx.map_refresh(m, obs_desc, obs_cam, start), want_moved, "after the move")
        assert ctx.map_debug_get(m)[0].tobytes() == moved.tobytes()


def test_a_second_refresh_with_the_same_observations_changes_nothing(ctx):
    pos, desc, obs_desc, obs_cam, start, want = case(257, 0.02)
    with resident(ctx, pos, desc) as m:
        first = ctx.map_refresh(m, obs_desc, obs_cam, start)
        held = ctx.map_debug_get(m)
        second = ctx.map_refresh(m, obs_desc, obs_cam, start)
        assert_refresh_equal(second, first, "second refresh")
        assert_refresh_equal(second, want, "second refresh")
        again = ctx.map_debug_get(m)
        assert again[0].tobytes() == held[0].tobytes() and again[1].tobytes() == held[1].tobytes()


def test_the_projection_matcher_finds_the_chosen_descriptors_at_distance_0(ctx):
    """The matcher of tracking by projection reads the same resident array: frame keypoints placed on the points' projections
    and carrying the chosen descriptors are found at Hamming distance 0, which the descriptors uploaded at first are not."""
    pos, desc, obs_desc, obs_cam, start, want = case(65, 0.08)
    seen = np.diff(start) > 0
    T = np.eye(4)
    u, v, in_view = P.project_map(pos, T, P.FR1_K, COLS, ROWS)
    assert in_view.all()
    txy = np.stack([u, v], 1).astype(np.float32)
    with resident(ctx, pos, desc) as m:
        _, idx, dist, _ = ctx.map_match_knn2_projection(m, T, P.FR1_K, COLS, ROWS, want[1], txy, 0.5)
        assert (dist[seen, 0] > 0).all(), "before the refresh the map holds the descriptors as uploaded"
        ctx.map_refresh(m, obs_desc, obs_cam, start)
        _, idx, dist, _ = ctx.map_match_knn2_projection(m, T, P.FR1_K, COLS, ROWS, want[1], txy, 0.5)
        assert (dist[:, 0] == 0).all() and (want[1][idx[:, 0]] == want[1]).all()


def _raw(ctx, m, obs_desc, obs_cam, start, n_obs, choice, desc_out, norm):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return ctx.lib.mvo_map_refresh(ctx.h, m, p(obs_desc), p(obs_cam), p(start), int(n_obs), p(choice), p(desc_out), p(norm))


def test_errors(mvo, ctx):
    pos, desc, obs_desc, obs_cam, start, want = case(5, 0.08)
    n, n_obs = 5, len(obs_desc)
    assert n_obs > 0
    choice, out, norm = np.full(n, 77, np.int32), np.full((n, 32), 77, np.uint8), np.full((n, 3), 77.0)

    def untouched():
        return (choice == 77).all() and (out == 77).all() and (norm == 77.0).all()

    with resident(ctx, pos, desc) as m:
        args = (obs_desc, obs_cam, start, n_obs, choice, out, norm)
        assert _raw(ctx, None, *args) == mvo.MVO_ERR_INVALID                                   # a null map
        for k in (0, 1, 2, 4, 6):                                                              # a null pointer with a positive count
            a = list(args)
            a[k] = None
            assert _raw(ctx, m, *a) == mvo.MVO_ERR_INVALID, k
        assert _raw(ctx, m, obs_desc, obs_cam, start, -1, choice, out, norm) == mvo.MVO_ERR_INVALID
        for bad in (start + 1, np.r_[start[:-1], start[-1] - 1], np.r_[start[:-1], start[-1] + 1]):
            assert _raw(ctx, m, obs_desc, obs_cam, np.ascontiguousarray(bad, np.int32), n_obs, choice, out, norm) == mvo.MVO_ERR_INVALID
        decreasing = np.array([0, 3, 2, n_obs, n_obs, n_obs], np.int32)
        assert _raw(ctx, m, obs_desc, obs_cam, decreasing, n_obs, choice, out, norm) == mvo.MVO_ERR_INVALID
        for v in (np.nan, np.inf, -np.inf):
            cam = obs_cam.copy()
            cam[n_obs - 1, 2] = v
            with pytest.raises(mvo.MvoError) as e:
                ctx.map_refresh(m, obs_desc, cam, start)
            assert e.value.code == mvo.MVO_ERR_INVALID
        assert untouched() and ctx.map_debug_get(m)[1].tobytes() == desc.tobytes()
        # a point with 65 observations: MVO_ERR_CAPACITY, nothing is written -- neither the outputs nor the resident array
        rng = np.random.RandomState(3)
        d65, c65, s65 = observations(rng, [2, 65, 3, 0, 1], 0.08)
        assert _raw(ctx, m, d65, c65, s65, len(d65), choice, out, norm) == mvo.MVO_ERR_CAPACITY
        assert untouched() and ctx.map_debug_get(m)[1].tobytes() == desc.tobytes()
        with pytest.raises(mvo.MvoError) as e:
            ctx.map_refresh(m, d65, c65, s65)
        assert e.value.code == mvo.MVO_ERR_CAPACITY
        # desc_out is optional
        assert _raw(ctx, m, obs_desc, obs_cam, start, n_obs, choice, None, norm) == mvo.MVO_OK
        assert np.array_equal(choice, want[0]) and R.same_f64(norm, want[2]) and (out == 77).all()
        assert ctx.map_debug_get(m)[1].tobytes() == want[1].tobytes()
        # n_obs == 0 succeeds: every choice -1, the descriptors stay, the normals are 0
        got = ctx.map_refresh(m, np.zeros((0, 32), np.uint8), np.zeros((0, 3)), np.zeros(n + 1, np.int32))
        assert (got[0] == -1).all() and got[1].tobytes() == want[1].tobytes() and not got[2].any()
        assert _raw(ctx, m, None, None, np.zeros(n + 1, np.int32), 0, choice, out, norm) == mvo.MVO_OK
    # an empty map succeeds (without a launch: there is nothing to write)
    with resident(ctx, np.zeros((0, 3), np.float32), np.zeros((0, 32), np.uint8)) as m:
        got = ctx.map_refresh(m, np.zeros((0, 32), np.uint8), np.zeros((0, 3)), np.zeros(1, np.int32))
        assert [len(a) for a in got] == [0, 0, 0]
        assert _raw(ctx, m, None, None, None, 0, None, None, None) == mvo.MVO_OK
        pos0, desc0 = ctx.map_debug_get(m)
        assert len(pos0) == 0 and len(desc0) == 0
