"""Device buffers that grow on demand (DevBuf, csrc/mvo_internal.h), through the calls that own them.  What a regrow can get
wrong is a stale pointer kept across the free, a capacity stored in the wrong unit, or one buffer of a group left at its old
size; so every test runs ONE context of its own through small -> grown -> regrown -> small again and holds every call to the
comparison its module already uses (the oracle or the restatement, bit for bit).

The sizes come from the floors, not from the workload.  Per-match buffers have a floor of 4096 entries: 64 stays below it, 4097 is
the first size that grows (to 4097 + 2048 = 6145 entries), 6146 the first that grows again.  tests/test_kernels_sim.py,
test_init_sim.py and test_init_finish_sim.py run the same functions through the emulated build."""
import numpy as np
import pytest

import finish_restate as FR
import h_restate as HR
import test_gpu_init as T_init
import test_gpu_init_finish as T_fin
import test_gpu_keyframe as T_kf
import test_gpu_track as T_track

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
