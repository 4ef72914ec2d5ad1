"""The HIP ORB path against the independent numpy transcription (tests/orb_numpy.py), and against the oracle where it exposes the
stage, on the inputs where extraction kernels go wrong: saturated and periodic images, extreme settings, level sizes on exact
halves, tile-edge and border-edge sizes, hand-made keypoint lists whose taps reach the unblurred frame.  Bit-exact throughout.
tests/test_orb_numpy.py runs a subset of these functions on the emulated build (tests/sim) without a GPU."""
import ctypes as C

import numpy as np
import pytest

import orb_numpy as N

pytestmark = pytest.mark.gpu

DEFAULTS = dict(nfeatures=8000, scale_factor=1.2, nlevels=4, fast_threshold=20, pyramid_interpolation=1, grid_size=16,
                # grid selection cuts nothing: the comparisons are about cv::ORB itself
                max_keypoints=1 << 20, grid_max_per_cell=1 << 20)
FT_TILE_CAP = 256          # csrc/mvo_internal.h: record slots per 64 x 16 detection tile


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


# ------------------------------------------------------------------------------------------------ inputs
def adversarial_images(w, h, seed=0):
    """Saturated, periodic and sparse images (u8 saturation in resize and blur, NMS ties, retainBest ties)."""
    rng = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    out = [("zeros", np.zeros((h, w), np.uint8)), ("ones255", np.full((h, w), 255, np.uint8))]
    for p in range(1, 6):
        out.append(("checker%d" % p, (((xs // p + ys // p) & 1) * 255).astype(np.uint8)))
    dots = np.zeros((h, w), np.uint8)
    dots[7::11, 5::13] = 255
    out.append(("dots", dots))
    out.append(("holes", 255 - dots))
    out.append(("noise", rng.randint(0, 256, (h, w)).astype(np.uint8)))
    out.append(("noise_bgr", rng.randint(0, 256, (h, w, 3)).astype(np.uint8)))
    return out


ADVERSARIAL_SETTINGS = [dict(), dict(fast_threshold=1), dict(fast_threshold=254), dict(nfeatures=0), dict(nfeatures=1),
                        dict(nlevels=1), dict(nlevels=8), dict(scale_factor=1.1), dict(scale_factor=1.5),
                        dict(scale_factor=2.0, nlevels=3)]
ADVERSARIAL_SIZE = (200, 160)      # every level of every setting above is >= 8 px (the device's limit)

# level sizes on exact halves of the float quotient: 486 / 1.44f = 337.5 (level 2), 177 / 1.2f = 147.5 and 126 / 1.44f = 87.5
HALF_SHAPES = [(486, 270), (177, 126), (270, 486)]
# tile edges (64 x 16 detection tiles): w = 1 / 63 mod 64 and h = 1 / 15 mod 16 at level 0 or 1; the 2 * 31 border at 62 / 63 / 64
EDGE_SHAPES = [(193, 145), (255, 111), (229, 175), (62, 100), (63, 63), (64, 80), (100, 64)]


def textured(w, h, seed, channels=1):
    """Corner-rich texture: blocky noise at a few scales (many FAST corners, few exact ties)."""
    rng = np.random.RandomState(seed)
    img = np.zeros((h, w))
    for cell in (1, 3, 7):
        blk = rng.uniform(0, 1, ((h + cell - 1) // cell, (w + cell - 1) // cell))
        img += np.kron(blk, np.ones((cell, cell)))[:h, :w]
    img = (img / 3 * 255).astype(np.uint8)
    return np.repeat(img[:, :, None], channels, axis=2) if channels > 1 else img


def handmade_keypoints(w, h):
    """Point 4 of the issue: half-integer coordinates (cvRound half-to-even), points that round to exactly 31 or w - 31 in
    the border filter, and angles whose sine / cosine land on exact or near-zero values."""
    rows = []
    angles = [0.0, 30.0, 90.0, 180.0, 270.0, 359.999, 360.0, 720.0, -1.0]
    for i, a in enumerate(angles):
        rows.append((w / 2 + i - 4.5, h / 2 + 0.5, a, 0))                    # half-integers, both parities
    for x in (30.5, 31.0, 31.5, 30.49, w - 31.5, w - 31.0, w - 32.5, w - 30.5):
        rows.append((x, h / 2, 45.0, 0))
    for y in (30.5, 31.5, h - 31.5, h - 32.5):
        rows.append((w / 2, y, 135.0, 1))
    return _kp(rows)


def border_keypoints(w, h, nlevels=8):
    """Point 1: keypoints at octaves 0..nlevels-1 placed on the level-0 border (rounded coordinate 31 or w - 32), at angles
    that send the taps towards it.  From octave 3 on their taps read blurred pixels whose blur reads the frame, from octave 4
    on they read the raw frame itself (tests/test_orb_numpy.py asserts both)."""
    rows = []
    for o in range(nlevels):
        for x, y, a in ((31.0, 31.0, 225.0), (w - 32.0, h - 32.0, 45.0), (31.0, h / 2, 180.0), (w / 2, 31.0, 270.0),
                        (w - 32.0, 31.0, 315.0), (31.0, h - 32.0, 0.0)):
            rows.append((x, y, a, o))
    return _kp(rows)


def _kp(rows):
    k = np.zeros(len(rows), N.KEYPOINT_DTYPE)
    for i, (x, y, a, o) in enumerate(rows):
        k[i] = (x, y, 31 * 1.2 ** o, a, 0.0, o, -1)
    return k


# ------------------------------------------------------------------------------------------------ checks
def _configure(ctx, kw):
    ctx.orb_configure(**params(**kw))
    return N.Orb(**params(**kw))


def _cand_struct(gc):
    return dict(x=gc["x"].astype(np.int64), y=gc["y"].astype(np.int64), level=(gc["level_score"] >> 16).astype(np.int64),
                fast_score=(gc["level_score"] & 0xffff).astype(np.int64), harris=gc["harris"], angle=gc["angle"])


def assert_candidates_equal(got, ref, what):
    assert len(got["x"]) == len(ref["x"]), "%s: %d vs %d candidates" % (what, len(got["x"]), len(ref["x"]))
    for f in N.CANDIDATE_FIELDS:
        g, r = np.asarray(got[f]), np.asarray(ref[f])
        if f in ("harris", "angle"):
            g, r = g.astype(np.float32).view(np.uint32), r.astype(np.float32).view(np.uint32)
        bad = np.nonzero(g != r)[0]
        assert len(bad) == 0, "%s: candidate field %s differs at %d of %d, first at %d" % (what, f, len(bad), len(g), bad[0])


def sorted_kp(k):
    return np.sort(np.asarray(k, N.KEYPOINT_DTYPE), order=["octave", "y", "x"])


def tile_survivor_max(cand):
    """The largest number of NMS survivors in one 64 x 16 detection tile of one level."""
    if len(cand["x"]) == 0:
        return 0
    key = (np.asarray(cand["level"]) << 40) + ((np.asarray(cand["y"]) // 16) << 20) + np.asarray(cand["x"]) // 64
    return int(np.unique(key, return_counts=True)[1].max())


def check_detection(mvo, O, ctx, img, kw, what, levels=True):
    """calc_keypoints on the device: every raw and blurred level, the candidate list and the keypoint set against the
    transcription, the keypoints against the oracle as well.  Leaves the ctx's pyramid cached; returns (transcription,
    its candidates, the device's keypoints)."""
    orb = _configure(ctx, kw)
    pyr = orb.pyramid(img)
    k = ctx.calc_keypoints(img, cap=1 << 17)
    ref = orb.detect(img, pyr)
    assert k.tobytes() == O.calc_keypoints(img, O.default_params(**ctx.params), cap=1 << 19).astype(k.dtype).tobytes(), \
        "%s: keypoints differ from the oracle" % what
    assert sorted_kp(k).tobytes() == ref.tobytes(), "%s: keypoint set differs from the transcription (%d vs %d)" % (
        what, len(k), len(ref))
    if levels:
        for l in range(orb.nlevels):
            for bl in (False, True):
                g = ctx.debug_level(l, bl)
                r = pyr.blur(l) if bl else pyr.raw[l]
                assert g.shape == r.shape, (what, l, g.shape, r.shape)
                bad = np.argwhere(g != r)
                assert len(bad) == 0, "%s: level %d blurred=%d: %d px differ, first %s" % (what, l, bl, len(bad), bad[0])
    cand = orb.candidates(img, pyr)
    assert_candidates_equal(_cand_struct(ctx.debug_candidates()), cand, what)
    return orb, cand, k


def check_descriptors(mvo, O, ctx, orb, img, kps, what, reuse):
    """calc_descriptors of a given keypoint list against the transcription and the oracle (which keypoints survive, their
    order, every descriptor bit).  reuse=True describes from the pyramid the ctx's last calc_keypoints built of `img`."""
    kg, dg = ctx.calc_descriptors(img, kps, reuse_pyramid=reuse)
    kr, dr = orb.compute(img, kps)
    ko, do = O.calc_descriptors(img, kps, O.default_params(**ctx.params))
    assert kg.tobytes() == kr.tobytes() == ko.astype(kg.dtype).tobytes(), "%s: kept keypoints differ" % what
    assert np.array_equal(dr, do), "%s: transcription and oracle differ in %d rows" % (what, (dr != do).any(1).sum())
    bad = np.nonzero((dg != dr).any(1))[0]
    assert len(bad) == 0, "%s: %d descriptors differ, first keypoint %r" % (what, len(bad), kg[bad[0]])
    return kg, dg


def contexts(mvo, kw):
    """A latency-mode ctx (windows blurred inside k_brief) and a throughput-mode ctx (whole levels blurred, k_brief_sample)."""
    out = []
    for mode in ("latency", "throughput"):
        c = mvo.Context(0, **params(**kw))
        c.ba_set_mode(mode)
        out.append((mode, c))
    return out


def check_keypoint_lists(mvo, O, w, h, flavours=(1, 0), reuse_modes=(False, True)):
    img = textured(w, h, w * 7 + h, channels=3)
    kps = np.concatenate([handmade_keypoints(w, h), border_keypoints(w, h)])
    for interp in flavours:
        kw = dict(nlevels=8, pyramid_interpolation=interp)
        for mode, c in contexts(mvo, kw):
            orb = N.Orb(**c.params)
            try:
                for reuse in reuse_modes:
                    if reuse:
                        c.calc_keypoints(img, cap=1 << 17)
                    check_descriptors(mvo, O, c, orb, img, kps, "%dx%d %s interp=%d reuse=%d" % (w, h, mode, interp, reuse), reuse)
            finally:
                c.close()


def check_adversarial(mvo, O, ctx, name, img, kw):
    orb, cand, k = check_detection(mvo, O, ctx, img, kw, "%s %r" % (name, kw))
    check_descriptors(mvo, O, ctx, orb, img, k, "%s %r" % (name, kw), reuse=True)
    assert tile_survivor_max(cand) <= FT_TILE_CAP


def check_shape(mvo, O, ctx, img, kw, what):
    orb, cand, k = check_detection(mvo, O, ctx, img, kw, what)
    for reuse in (True, False):
        check_descriptors(mvo, O, ctx, orb, img, k, "%s reuse=%d" % (what, reuse), reuse)


def check_too_small(mvo, O, ctx):
    """DESIGN.md section 2, deviation (6): a frame whose smallest pyramid level is under 8 px is refused with MVO_ERR_INVALID;
    cv::ORB (the oracle, the transcription) returns no keypoints for it.  So is a frame more than 8192 px wide."""
    for (w, h), kw in (((9, 9), {}), ((40, 30), dict(nlevels=8, scale_factor=1.5)), ((12, 100), {})):
        img = textured(w, h, 3)
        orb = _configure(ctx, kw)
        assert min(min(s) for s in orb.pyramid(img).sizes) < 8
        assert len(orb.detect(img)) == 0
        assert len(O.calc_keypoints(img, O.default_params(**ctx.params))) == 0
        with pytest.raises(mvo.MvoError) as e:
            ctx.calc_keypoints(img)
        assert e.value.code == mvo.MVO_ERR_INVALID and "too small" in ctx.last_error()
    # the smallest accepted frame: its last level is exactly 8 px (and far too small for a keypoint)
    _configure(ctx, {})
    assert N.level_size(14, 14, 1.2, 3)[:2] == (8, 8)
    assert len(ctx.calc_keypoints(textured(14, 14, 4))) == 0
    _configure(ctx, dict(nlevels=1))
    with pytest.raises(mvo.MvoError) as e:
        ctx.calc_keypoints(np.zeros((40, 8193), np.uint8))
    assert e.value.code == mvo.MVO_ERR_INVALID and "too wide" in ctx.last_error()


# ------------------------------------------------------------------------------------------------ the MI355X tests
@pytest.fixture(autouse=True)
def _restore_shared_ctx(request):
    """These tests reconfigure the session's shared ctx; later test files get it back as they left it."""
    if "ctx" not in request.fixturenames:
        yield
        return
    c = request.getfixturevalue("ctx")
    saved = dict(c.params)
    yield
    c.orb_configure(**saved)


@pytest.mark.parametrize("kw", ADVERSARIAL_SETTINGS, ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()) or "default")
def test_adversarial_images(mvo, O, ctx, kw):
    w, h = ADVERSARIAL_SIZE
    for name, img in adversarial_images(w, h):
        check_adversarial(mvo, O, ctx, name, img, kw)


@pytest.mark.parametrize("w,h", HALF_SHAPES + EDGE_SHAPES)
@pytest.mark.parametrize("interp", [1, 0])
def test_half_and_edge_shapes(mvo, O, ctx, w, h, interp):
    kw = dict(pyramid_interpolation=interp, fast_threshold=10)
    for ch in (1, 3):
        img = textured(w, h, w + 3 * h + ch, channels=ch)
        check_shape(mvo, O, ctx, img, kw, "%dx%dx%d" % (w, h, ch))


def test_keypoint_lists_reach_the_frame(mvo, O):
    check_keypoint_lists(mvo, O, 320, 240)
    check_keypoint_lists(mvo, O, 177, 126, flavours=(1,))


def test_padded_stride_and_bgra(mvo, O, ctx):
    w, h = 193, 145
    img = textured(w, h, 11, channels=3)
    orb = _configure(ctx, dict(fast_threshold=10))
    ref = orb.detect(img)
    for ch, stride in ((3, 640), (4, 4 * w), (4, 1024), (1, 256)):
        src = img if ch == 3 else (np.concatenate([img, np.full((h, w, 1), 77, np.uint8)], 2) if ch == 4 else img[:, :, 0])
        buf = np.zeros((h, stride), np.uint8)
        buf[:, :w * ch] = src.reshape(h, w * ch)
        want = ref if ch != 1 else orb.detect(src)
        out = np.zeros(1 << 14, mvo.KEYPOINT_DTYPE)
        n = C.c_int()
        r = ctx.lib.mvo_calc_keypoints(ctx.h, buf.ctypes.data_as(C.c_void_p), w, h, stride, ch, out.ctypes.data_as(C.c_void_p),
                                       len(out), C.byref(n))
        assert r == 0
        assert sorted_kp(out[:n.value]).tobytes() == want.tobytes(), (ch, stride)
        assert np.array_equal(ctx.debug_level(0), N.Pyramid(buf, w=w, h=h, stride=stride, channels=ch).raw[0])


def test_device_resident_entry_points_on_an_adversarial_image(mvo, O, ctx):
    import torch
    w, h = ADVERSARIAL_SIZE
    img = dict(adversarial_images(w, h))["noise_bgr"]
    kw = dict(fast_threshold=1, nfeatures=3000)
    orb = _configure(ctx, kw)
    t = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    k = ctx.calc_keypoints_dev(t.data_ptr(), w, h, w * 3, 3, cap=1 << 15)
    assert sorted_kp(k).tobytes() == orb.detect(img).tobytes()
    k2, d, dptr = ctx.calc_descriptors_dev(k)
    assert len(k2) > 100
    kr, dr = orb.compute(img, k)
    assert k2.tobytes() == kr.tobytes() and np.array_equal(d, dr) and dptr


def test_full_hd_noise_at_threshold_one(mvo, O, ctx):
    """The densest detection there is: 1920x1080 uniform noise at fast_threshold 1 (NMS survivors at their per-tile peak)."""
    img = np.random.RandomState(1080).randint(0, 256, (1080, 1920)).astype(np.uint8)
    kw = dict(fast_threshold=1, nfeatures=20000)
    orb, cand, k = check_detection(mvo, O, ctx, img, kw, "1920x1080 noise", levels=False)
    peak = tile_survivor_max(cand)
    assert 0 < peak <= FT_TILE_CAP, "largest survivor count of a 64x16 tile: %d (FT_TILE_CAP %d)" % (peak, FT_TILE_CAP)
    assert peak > FT_TILE_CAP // 4, "the frame should crowd its tiles: peak %d of FT_TILE_CAP %d" % (peak, FT_TILE_CAP)
    check_descriptors(mvo, O, ctx, orb, img, k, "1920x1080 noise", reuse=True)


def test_input_limits(mvo, O, ctx):
    check_too_small(mvo, O, ctx)
