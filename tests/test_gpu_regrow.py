"""Device buffers that grow on demand (DevBuf, csrc/mvo_internal.h), through the calls that own them.  What a regrow can get
wrong is a stale pointer kept across the free, a capacity stored in the wrong unit, or one buffer of a group left at its old
size; so every test runs ONE context of its own through small -> grown -> regrown -> small again and holds every call to the
comparison its module already uses (the oracle or the restatement, bit for bit).

The sizes come from the floors, not from the workload.  Per-match buffers have a floor of 4096 entries: 64 stays below it, 4097 is
the first size that grows (to 4097 + 2048 = 6145 entries), 6146 the first that grows again.  tests/test_kernels_sim.py,
test_init_sim.py and test_init_finish_sim.py run the same functions through the emulated build.

The calls that stage one upload through csrc/staged_call.h (map refresh, map refine, map fusion, window triangulation, pose
optimisation) size their d_in in BYTES, with a floor of 2^20 (2^16 for the pose optimisation): the *_in_bytes functions below
restate each layout (blocks padded to 64 bytes, the last one not), and staged_sizes() takes the steps from them.
tests/sim/staged_call_check.cpp runs the same sequence under the sanitizers on the CPU, the scratch of the per-frame launches
included (64 queries never take it past its floors here)."""
import numpy as np
import pytest

import finish_restate as FR
import h_restate as HR
import map_fuse_numpy as MF
import test_gpu_init as T_init
import test_gpu_init_finish as T_fin
import test_gpu_keyframe as T_kf
import test_gpu_map_fuse as T_fuse
import test_gpu_map_refine as T_refine
import test_gpu_map_refresh as T_refresh
import test_gpu_pose_optimize as T_pose
import test_gpu_track as T_track
import test_gpu_window_triangulate as T_win
import window_triangulate_numpy as W

PER_MATCH = (64, 4097, 6146, 64)


def own_ctx(mvo, steps, body):
    c = mvo.Context(0)
    try:
        for step in steps:
            body(c, step)
    finally:
        c.close()


def triangulate_steps(mvo, O, steps=PER_MATCH):
    """d_tri_in (4 n floats) and d_tri_out (6 n floats)."""
    own_ctx(mvo, steps, lambda c, n: T_kf.test_triangulate_points_bit_exact(mvo, O, c, n, 21, {}))


def essential_steps(mvo, O, steps=PER_MATCH):
    """d_emq (4 n doubles) and d_em_mask (n bytes)."""
    own_ctx(mvo, steps, lambda c, n: T_kf.test_find_essential_inliers_matches_the_oracle(mvo, O, c, n, 8, {}))


def homography_steps(mvo, R, steps=PER_MATCH):
    """d_hpts (4 n floats) and d_h_mask (n bytes)."""
    def body(c, n):
        pr = HR.two_view(n, 4, planar=True, noise=0.5, outlier_frac=0.3)
        assert T_init.check_find_homography(c, R, pr["src"], pr["dst"])[0]["H"] is not None
    own_ctx(mvo, steps, body)


def map_steps(mvo, O, steps=PER_MATCH):
    """ONE resident map uploaded at every size: d_pos (3 n floats), d_desc (32 n bytes) and the ctx's d_view_desc (32 n bytes).
    The gathered descriptors are read back through the matcher, as vo.cpp:281-289 uses them."""
    c = mvo.Context(0)
    m = c.map_create()
    try:
        for n_map in steps:
            pr = mvo.synth.tracking_problem(n_map=n_map, seed=3)
            c.map_upload(m, pr["map_pos"], pr["map_desc"])
            idx, px, d_desc = c.map_points_in_view(m, pr["T_w_c"], pr["K"], pr["cols"], pr["rows"], cap=n_map)
            io, po = O.map_in_view(pr["map_pos"], pr["T_w_c"], pr["K"], pr["cols"], pr["rows"])
            assert len(io) > 0 and np.array_equal(idx, io) and np.array_equal(px, po)
            cur = mvo.synth.match_inputs("perturbed", 300, 300, seed=3)[1]
            i2, d2 = c.match_knn2_dev(d_desc, len(idx), T_track._to_device(cur).data_ptr(), len(cur))
            i2o, d2o = O.match_knn2(pr["map_desc"][io], cur)
            assert np.array_equal(i2, i2o) and np.array_equal(d2, d2o)
    finally:
        c.map_release(m)
        c.close()


# (n, iterations).  The per-hypothesis buffers have a floor of 128 hypotheses: 129 is the first count past it (to 193), 200 the
# next that grows.  The masks (n x iterations bytes) have a floor of 2^20: 4097 x 129 = 528 513 stays below it, 6146 x 200 =
# 1 229 200 passes it.  The per-pair buffers follow PER_MATCH.
PNP_STEPS = ((64, 100), (4097, 129), (6146, 200), (64, 100))


def pnp_steps(mvo, O, steps=PNP_STEPS):
    pr = mvo.synth.tracking_problem(n_map=20000, seed=18)
    assert len(pr["pts3d"]) >= max(n for n, _ in steps)

    def body(c, step):
        n, iters = step
        p3, p2, K = pr["pts3d"][:n], pr["pts2d"][:n], pr["K"]
        got = c.solve_pnp_ransac(p3, p2, K, iterations=iters)
        dbg = c.debug_pnp()
        ref = O.solve_pnp_ransac(p3, p2, K, iters=iters)
        run = ref["iters_run"]
        assert got["ok"] and ref["ok"]
        assert dbg["n_hyp"] == iters and dbg["iters_run"] == run and dbg["best_iter"] == ref["best_iter"]
        assert np.array_equal(dbg["counts"][:run], ref["counts"][:run])
        assert T_track._same_models(dbg["models"][:run], ref["models"][:run])
        assert np.array_equal(got["inliers"], ref["inliers"])
        assert dbg["dlt"] == ref["dlt"] and dbg["lm_iters"] == ref["lm_iters"]
        assert np.abs(got["rvec"] - ref["rvec"]).max() < 1e-8 and np.abs(got["tvec"] - ref["tvec"]).max() < 1e-8
    own_ctx(mvo, steps, body)


# n matches through mvo_estimate_possible_relative_poses + mvo_init_two_view.  d_ip_pts holds 15 n floats above a floor of
# 65536: 4400 is past 4370, the first n that grows (to 99000 floats), 9000 grows again.  d_sc_in holds 16 n bytes plus 4 per list
# entry above a floor of 65536 bytes: 70400 + 4 L at 4400, which 144000 bytes of matches alone pass again at 9000 as long as
# 1.5 (70400 + 4 L) < 144000, that is L < 6400 entries at 4400.  d_sc_kept (floor 4096 entries) grows at 4400 when the two
# lists hold more than 4096 entries, and regrows at 9000 when they hold more than one and a half times what they held at 4400.
INIT_STEPS = (64, 4400, 9000, 64)


def init_chain_steps(mvo, F, O, steps=INIT_STEPS):
    lists = {}

    def body(c, n):
        pr = T_fin.scene("thick", n, 36, 0.1)
        got, _ = T_fin.check_init(c, F, O, pr["src"], pr["dst"], pr["K"])
        lists[n] = len(got["poses"]["inliers_e"]) + len(got["poses"]["inliers_h"])
    own_ctx(mvo, steps, body)
    # the preconditions on the synthetic scene under which every list-sized buffer did regrow
    if 9000 in lists and 4400 in lists:
        assert lists[9000] > 3600
        assert 4096 < lists[4400] < 6400 and lists[9000] > lists[4400] + lists[4400] // 2, lists


def a64(b):
    return (b + 63) // 64 * 64


def staged_sizes(in_bytes, floor=1 << 20):
    """(grown, regrown): the smallest size whose upload exceeds the floor (d_in then holds one and a half times its bytes), and the
    smallest whose upload exceeds that."""
    grown = 1
    while in_bytes(grown) <= floor:
        grown += 1
    cap = in_bytes(grown) + in_bytes(grown) // 2
    regrown = grown
    while in_bytes(regrown) <= cap:
        regrown += 1
    return grown, regrown


def refresh_in_bytes(n):
    """n map points with 64 observations each (the most a point holds, so the fewest points): camera centres, descriptors, starts."""
    return a64(64 * n * 24) + a64(64 * n * 32) + (n + 1) * 4


def refresh_steps(mvo, steps=None):
    grown, regrown = staged_sizes(refresh_in_bytes)
    assert (grown, regrown) == (293, 440)

    def body(c, n):
        pos, desc, obs_desc, obs_cam, start, want = T_refresh.case(n, 0.08, (64,) * n)
        with T_refresh.resident(c, pos, desc) as m:
            T_refresh.assert_refresh_equal(c.map_refresh(m, obs_desc, obs_cam, start), want, "%d points of 64 observations" % n)
            assert c.map_debug_get(m)[1].tobytes() == want[1].tobytes()
    own_ctx(mvo, steps or (3, grown, regrown, 3), body)


REFINE_FRAMES = 64


def refine_in_bytes(n):
    """n map points with 64 observations each over 64 frames: poses, pixels, frame indices, starts."""
    return a64(REFINE_FRAMES * 96) + a64(64 * n * 8) + a64(64 * n * 4) + (n + 1) * 4


def refine_inputs(n):
    """The 64 points of one scene, each seen in all 64 frames, repeated up to n points: the restatement takes the points one by
    one, and what it costs is its scene, one projection in Python per observation."""
    rng = np.random.RandomState(64)
    _, pos, T, frame, uv, start, _ = T_refine.R.scene(rng, [64] * 64, REFINE_FRAMES, 0.5, 5, K=T_refine.K, step=0.57 / 63, yaw=0.19 / 63)
    reps = -(-n // 64)
    return dict(pos=np.tile(pos, (reps, 1))[:n], T=T, frame=np.tile(frame, reps)[:64 * n], uv=np.tile(uv, (reps, 1))[:64 * n],
                start=(64 * np.arange(n + 1)).astype(np.int32))


def refine_steps(mvo, steps=None):
    grown, regrown = staged_sizes(refine_in_bytes)
    assert (grown, regrown) == (1351, 2031)

    def body(c, n):
        s = refine_inputs(n)
        want = T_refine.R.refine(s["pos"], s["T"], T_refine.K, s["frame"], s["uv"], s["start"], {}, {})
        assert (want[2][:, 0] == 0).all() and (n < 5 or want[3].any())      # every point refined, the moved observations flagged
        with T_refine.resident(c, s["pos"]) as m:
            T_refine.assert_equal(T_refine.call(c, m, s), want, "%d points of 64 observations" % n)
            assert c.map_debug_get(m)[0].tobytes() == want[0].tobytes()
    own_ctx(mvo, steps or (3, grown, regrown, 3), body)


def thirds(total):
    return [total // 3, total // 3, total - 2 * (total // 3)]


def fuse_in_bytes(total, n_map=64, n_frames=3):
    """A 64-point map against 3 frames of `total` keypoints in all: frame table (128 bytes a row), seen masks, (x, y, tol2), descriptors."""
    return a64(n_frames * 128) + a64(n_map * 8) + a64(total * 24) + total * 32


def fuse_steps(mvo, steps=None):
    grown, regrown = staged_sizes(fuse_in_bytes)
    assert (grown, regrown) == (18709, 28072) and fuse_in_bytes(2 * 64, n_frames=2) < 1 << 20

    def body(c, kp):
        s = MF.scene(np.random.RandomState(sum(kp)), 64, kp, K=T_fuse.K, cols=T_fuse.COLS, rows=T_fuse.ROWS)
        raw = MF.search(s["pos"], s["desc"], s["frames"], T_fuse.K, T_fuse.COLS, T_fuse.ROWS, MF.DEFAULT_MAX_PX)
        want = MF.resolve(64, s["frames"], raw[0], raw[1], MF.DEFAULT_MAX_HAMMING)
        assert want[2][0] > 0 and want[2][3] > 0      # candidates, additions
        what = "%r keypoints" % (kp,)
        with T_fuse.resident(c, s["pos"], s["desc"]) as m:
            T_fuse.assert_same(c.map_fuse_search(m, s["frames"], T_fuse.K, T_fuse.COLS, T_fuse.ROWS, MF.DEFAULT_MAX_PX), raw, T_fuse.RAW, what)
            T_fuse.assert_same(c.map_fuse(m, s["frames"], T_fuse.K, T_fuse.COLS, T_fuse.ROWS), want, T_fuse.RULE, what)
    own_ctx(mvo, steps or ([64, 64], thirds(grown), thirds(regrown), [64, 64]), body)


def window_in_bytes(total, nq=64, n_frames=3):
    """64 keypoints of curr against 3 frames of `total` keypoints in all: frame table (200 bytes a row), curr's free flags, pixels
    and descriptors, then (u, v, tol2) and the descriptors of the frames."""
    return a64(n_frames * 200) + a64(nq) + a64(nq * 8) + a64(nq * 32) + a64(total * 24) + total * 32


def window_steps(mvo, steps=None):
    grown, regrown = staged_sizes(window_in_bytes)
    assert (grown, regrown) == (18667, 28031) and window_in_bytes(2 * 64, n_frames=2) < 1 << 20

    def body(c, kp):
        s = W.scene(np.random.RandomState(sum(kp)), 64, kp, K=T_win.K)
        points, pairs, counts, raw = W.window_triangulate(s["curr"], s["frames"], T_win.K)
        assert len(points) > 0 and len(pairs) > len(points)
        T_win.run(c, dict(s, raw=raw, want=(points, pairs, counts), params={}), "%r keypoints" % (kp,))
    own_ctx(mvo, steps or ([64, 64], thirds(grown), thirds(regrown), [64, 64]), body)


def pose_in_bytes(n):
    return a64(n * 12) + a64(n * 8) + n * 4      # pts3d, pts2d, inv_sigma2


def pose_optimize_steps(mvo, steps=(64, 2800, 64)):
    """d_in has a floor of 2^16 bytes and PO_MAX_OBS = 4096 observations of 24 bytes end at 98304: past the floor (2729 is the
    first count that passes it; 2800 grows d_in to 100800 bytes) nothing under the capacity can grow it a second time, so there
    are three steps and not four."""
    assert pose_in_bytes(64) < 1 << 16 < pose_in_bytes(2800) and pose_in_bytes(4096) < pose_in_bytes(2800) * 3 // 2

    def body(c, n):
        want, _ = T_pose.answer(n, True)
        assert want[4][0] == T_pose.R.OPTIMISED
        T_pose.assert_equal(T_pose.call(c, T_pose.scene(n), True, {}), want, "%d observations" % n)
    own_ctx(mvo, steps, body)


@pytest.fixture(scope="module")
def R():
    return HR.Restatement()


@pytest.fixture(scope="module")
def F():
    return FR.Restatement()


@pytest.mark.gpu
def test_triangulation_buffers_regrow(mvo, O):
    triangulate_steps(mvo, O)


@pytest.mark.gpu
def test_essential_buffers_regrow(mvo, O):
    essential_steps(mvo, O)


@pytest.mark.gpu
def test_homography_buffers_regrow(mvo, R):
    homography_steps(mvo, R)


@pytest.mark.gpu
def test_resident_map_and_view_buffers_regrow(mvo, O):
    map_steps(mvo, O)


@pytest.mark.gpu
def test_pnp_buffers_regrow(mvo, O):
    pnp_steps(mvo, O)


@pytest.mark.gpu
def test_initialisation_buffers_regrow(mvo, F, O):
    init_chain_steps(mvo, F, O)


@pytest.mark.gpu
def test_map_refresh_upload_regrows(mvo):
    refresh_steps(mvo)


@pytest.mark.gpu
def test_map_refine_upload_regrows(mvo):
    refine_steps(mvo)


@pytest.mark.gpu
def test_map_fuse_upload_regrows(mvo):
    fuse_steps(mvo)


@pytest.mark.gpu
def test_window_triangulate_upload_regrows(mvo):
    window_steps(mvo)


@pytest.mark.gpu
def test_pose_optimize_upload_regrows(mvo):
    pose_optimize_steps(mvo)
