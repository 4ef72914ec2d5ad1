"""The ORB-SLAM style detector on the device (csrc/orb_distribute_kernels.hip, orb_distribute_host.cpp)
against its numpy transcription (tests/orb_distribute_numpy.py): the candidates in their declared order and the key points in
all seven fields, bit for bit.  tests/test_orb_distribute_sim.py runs the same functions on the emulated build without a GPU.
The transcription of an image is computed once and shared by the tests that need it."""
import ctypes as C

import numpy as np
import pytest

import orb_distribute_numpy as D
import orb_numpy as N

pytestmark = pytest.mark.gpu

# grid selection cuts nothing unless a case says so: the comparisons are about the detector
BASE = dict(nfeatures=300, scale_factor=1.2, nlevels=4, fast_threshold=20, pyramid_interpolation=1, grid_size=16,
            max_keypoints=1 << 20, grid_max_per_cell=1 << 20)


def _to_device(a):
    import torch
    t = torch.from_numpy(np.array(a)).cuda()
    torch.cuda.synchronize()
    return t


# ------------------------------------------------------------------------------------------------ inputs
def textured(w, h, seed):
    """Corner-rich texture: blocky noise at a few scales."""
    rng = np.random.RandomState(seed)
    img = np.zeros((h, w))
    for cell in (1, 3, 7):
        blk = rng.uniform(0, 1, ((h + cell - 1) // cell, (w + cell - 1) // cell))
        img += np.kron(blk, np.ones((cell, cell)))[:h, :w]
    return (img / 3 * 255).astype(np.uint8)


def texture_frame(mvo, quarter):
    """A 640 x 480 crop of the world texture, at full contrast or compressed to a quarter of it around mid-gray."""
    t = mvo.synth.world_texture()[700:1180, 600:1240]
    if quarter:
        t = 128 + (t - 128) / 4
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


def _image(mvo, name):
    if name == "one_cell":
        return textured(62, 62, 1)
    if name == "clamped":
        return textured(93, 70, 2)
    if name in ("small4", "levels8"):
        return mvo.synth.small_test_image(3, 160, 120)
    if name == "texture":
        return texture_frame(mvo, False)
    if name == "texture_quarter":
        return texture_frame(mvo, True)
    if name == "constant":
        return np.full((120, 160), 77, np.uint8)
    if name == "widest_cell":
        return textured(95, 95, 4)
    if name == "noise":
        return np.random.RandomState(5).randint(0, 256, (100, 131)).astype(np.uint8)
    raise KeyError(name)


# name -> (ORB parameters over BASE, detector parameters over the defaults)
CASES = {
    "one_cell": (dict(nlevels=1, nfeatures=40), {}),
    "clamped": (dict(nlevels=1, nfeatures=100), {}),
    "small4": ({}, {}),
    "small4_e31": ({}, dict(edge_threshold=31)),
    "small4_grid": (dict(max_keypoints=60, grid_max_per_cell=2), {}),
    "texture": (dict(nfeatures=2000), {}),
    "texture_e31": (dict(nfeatures=2000), dict(edge_threshold=31)),
    "texture_quarter": (dict(nfeatures=2000), {}),
    "constant": ({}, {}),
    # thresholds 1 / 1: every strict maximum of the noise is a candidate (cell slots at capacity), the quota binds hard
    "noise": (dict(nlevels=2, nfeatures=150), dict(ini_threshold=1, min_threshold=1)),
    "noise_cell8": (dict(nlevels=1, nfeatures=500), dict(ini_threshold=1, min_threshold=1, cell_size=8)),
    "noise_cell32": (dict(nlevels=2, nfeatures=150), dict(ini_threshold=40, min_threshold=3, cell_size=32, edge_threshold=24)),
    # levels 4 to 7 (77 x 58 and smaller: 58 - 2 * 19 + 6 = 26 < 30 rows) have no cell
    "levels8": (dict(nlevels=8), {}),
    # the widest cell a configuration can make: one cell of 57 x 57 scored pixels (cell_size 32, 95 - 2 * 19 + 6 = 63 < 2 * 32)
    "widest_cell": (dict(nlevels=1, nfeatures=120), dict(cell_size=32, min_threshold=2)),
}
_IMG_OF = {"small4_e31": "small4", "small4_grid": "small4", "texture_e31": "texture", "noise_cell8": "noise",
           "noise_cell32": "noise"}
_REF = {}


def case(mvo, name):
    """(image, ORB parameters, detector parameters, reference candidates, reference key points), made once."""
    if name not in _REF:
        orb, dist = CASES[name]
        p = dict(BASE)
        p.update(orb)
        img = _image(mvo, _IMG_OF.get(name, name))
        ref = D.OrbDistribute(**p, **dist)
        pyr = ref.pyramid(img)
        cand = ref.candidates(img, pyr)
        _REF[name] = (img, p, dist, cand, ref.detect(img, pyr, cand))
    return _REF[name]


def configure(ctx, p, dist):
    ctx.orb_configure(**p)
    ctx.orb_distribute_configure(**dist)


def assert_candidates_equal(got, ref, what):
    g = np.stack([got[f].astype(np.int64) for f in ("x", "y", "level", "score")], axis=1).reshape(-1, 4)
    assert len(g) == len(ref), "%s: %d vs %d candidates" % (what, len(g), len(ref))
    bad = np.nonzero((g != ref).any(axis=1))[0]
    assert len(bad) == 0, "%s: %d of %d candidates differ, first at %d: %r vs %r" % (what, len(bad), len(g), bad[0], g[bad[0]],
                                                                                   ref[bad[0]])


def assert_keypoints_equal(got, ref, what):
    assert len(got) == len(ref), "%s: %d vs %d key points" % (what, len(got), len(ref))
    for f in N.KEYPOINT_DTYPE.names:
        a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(ref[f])
        if a.dtype.kind == "f":
            a, b = a.view(np.uint32), b.view(np.uint32)
        bad = np.nonzero(a != b)[0]
        assert len(bad) == 0, "%s: field %s differs at %d of %d, first at %d: %r vs %r" % (what, f, len(bad), len(a), bad[0],
                                                                                          got[bad[0]], ref[bad[0]])


@pytest.fixture(scope="module")
def dctx(mvo):
    """A context of this module's own (the cases reconfigure it)."""
    c = mvo.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("name", sorted(CASES))
def test_candidates_and_keypoints_bit_exact(mvo, dctx, name):
    img, p, dist, cand, kps = case(mvo, name)
    configure(dctx, p, dist)
    got = dctx.calc_keypoints_distributed(img, cap=len(kps) + 64)
    print("%s: %d candidates, %d key points, per level %s" % (name, len(cand), len(kps),
                                                              np.bincount(kps["octave"], minlength=p["nlevels"]).tolist()))
    assert_candidates_equal(dctx.debug_distribute_candidates(), cand, name)
    assert_keypoints_equal(got, kps, name)
    if name == "constant":
        assert len(cand) == 0 and len(got) == 0
    if name == "levels8":
        assert kps["octave"].max() == 3 and len(kps) > 0


def test_descriptors_of_the_distributed_keypoints(mvo, dctx):
    for name in ("small4", "texture_quarter"):
        img, p, dist, _, kps = case(mvo, name)
        configure(dctx, p, dist)
        got = dctx.calc_keypoints_distributed(img, cap=len(kps) + 64)
        k2, d2 = dctx.calc_descriptors(img, got, reuse_pyramid=True)
        rk, rd = N.Orb(**p).compute(img, kps)
        assert_keypoints_equal(k2, rk, name + " described")
        assert np.array_equal(d2, rd), name
        assert 0 < len(rk) <= len(kps)


def test_padded_stride_bgra_and_the_device_pointer_form(mvo, dctx):
    img, p, dist, cand, kps = case(mvo, "small4")
    configure(dctx, p, dist)
    h, w = img.shape[:2]
    cap = len(kps) + 64
    # BGRA in rows 700 bytes apart, the padding filled with noise
    stride = 700
    buf = np.random.RandomState(9).randint(0, 256, (h, stride)).astype(np.uint8)
    bgra = np.concatenate([img, np.full((h, w, 1), 200, np.uint8)], axis=2)
    buf[:, :4 * w] = bgra.reshape(h, 4 * w)
    out, n = np.zeros(cap, mvo.KEYPOINT_DTYPE), C.c_int()
    r = dctx.lib.mvo_calc_keypoints_distributed(dctx.h, buf.ctypes.data_as(C.c_void_p), w, h, stride, 4,
                                                out.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    assert r == 0, dctx.last_error()
    assert_candidates_equal(dctx.debug_distribute_candidates(), cand, "padded BGRA")
    assert_keypoints_equal(out[:n.value], kps, "padded BGRA")
    d = _to_device(buf)
    got = dctx.calc_keypoints_distributed_dev(d.data_ptr(), w, h, stride, 4, cap=cap)
    assert_keypoints_equal(got, kps, "device pointer form")
    d3 = _to_device(img)
    got = dctx.calc_keypoints_distributed_dev(d3.data_ptr(), w, h, 3 * w, 3, cap=cap)
    assert_candidates_equal(dctx.debug_distribute_candidates(), cand, "device pointer form, BGR")
    assert_keypoints_equal(got, kps, "device pointer form, BGR")


@pytest.mark.parametrize("mode", ["latency", "throughput"])
def test_latency_and_throughput_contexts(mvo, mode):
    c = mvo.Context(0)
    try:
        c.ba_set_mode(mode)
        for name in ("small4", "texture_quarter"):
            img, p, dist, cand, kps = case(mvo, name)
            configure(c, p, dist)
            got = c.calc_keypoints_distributed(img, cap=len(kps) + 64)
            assert_candidates_equal(c.debug_distribute_candidates(), cand, name)
            assert_keypoints_equal(got, kps, name)
            k2, d2 = c.calc_descriptors(img, got, reuse_pyramid=True)
            rk, rd = N.Orb(**p).compute(img, kps)
            assert_keypoints_equal(k2, rk, name)
            assert np.array_equal(d2, rd), name
    finally:
        c.close()


def test_the_existing_detector_is_untouched_by_a_distributed_call(mvo):
    img, p, dist, _, kps = case(mvo, "small4")
    fresh = mvo.Context(0, **p)
    want = fresh.calc_keypoints(img, cap=4096)
    want_c = fresh.debug_candidates()
    fresh.close()
    c = mvo.Context(0, **p)
    try:
        before = c.calc_keypoints(img, cap=4096)
        c.orb_distribute_configure(**dist)
        mid = c.calc_keypoints_distributed(img, cap=len(kps) + 64)
        after = c.calc_keypoints(img, cap=4096)
        assert len(want) > 0
        assert before.tobytes() == want.tobytes() and after.tobytes() == want.tobytes()
        assert c.debug_candidates().tobytes() == want_c.tobytes()
        assert_keypoints_equal(mid, kps, "between two calc_keypoints")
    finally:
        c.close()


def test_reconfiguration_and_errors(mvo, dctx):
    img, p, dist, cand, kps = case(mvo, "small4")
    configure(dctx, p, dict(edge_threshold=31))
    dctx.calc_keypoints_distributed(img, cap=4096)
    configure(dctx, p, dist)       # the same geometry with other detector parameters: the cell table is rebuilt
    assert_keypoints_equal(dctx.calc_keypoints_distributed(img, cap=4096), kps, "after reconfiguration")
    for bad in (dict(ini_threshold=6, min_threshold=7), dict(min_threshold=0), dict(ini_threshold=256), dict(cell_size=7),
                dict(cell_size=33), dict(edge_threshold=18), dict(edge_threshold=32)):
        with pytest.raises(mvo.MvoError) as e:
            dctx.orb_distribute_configure(**bad)
        assert e.value.code == mvo.MVO_ERR_INVALID, bad
    assert_keypoints_equal(dctx.calc_keypoints_distributed(img, cap=4096), kps, "a refused configuration changes nothing")
    assert dctx.lib.mvo_orb_distribute_configure(dctx.h, None) == 0   # NULL = the defaults
    with pytest.raises(mvo.MvoError) as e:
        dctx.calc_keypoints_distributed(img, cap=3)
    assert e.value.code == mvo.MVO_ERR_CAPACITY
