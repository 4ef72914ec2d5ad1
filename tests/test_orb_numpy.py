"""The oracle's ORB restatement against a second, independent transcription (tests/orb_numpy.py: numpy, no code shared with
oracle/ or csrc/), stage by stage and bit for bit, on the inputs where a restatement of cv::ORB can slip: saturated and periodic
images, extreme settings, level sizes on exact halves, tile-edge and border-edge shapes, padded strides, BGRA, hand-made keypoint
lists whose taps reach the unblurred 32-px frame.  Independent float64 bounds for the two float stages (Harris, IC angle), the
rBRIEF table pinned by its hash, and a subset of tests/test_gpu_orb_numpy.py on the emulated build (tests/sim).

Where the two transcriptions could disagree, the published upstream rule decides (none disagreed when this was written):
level sizes are cvRound of the FLOAT quotient (ORB_Impl::detectAndCompute: Size(cvRound(image.cols / scale), cvRound(image.rows /
scale)) with an int and a float operand); NMS keeps a corner only if its score is STRICTLY above all eight neighbours (cv::FAST_t); the
descriptor centre is cvRound (half to even) of the float product pt * (1/scale); the 32-px frame of a blurred level is the raw
BORDER_REFLECT_101 frame (cv::ORB::compute blurs each level's ROI in place: GaussianBlur(workingMat(ROI), ...)); retainBest keeps
every keypoint whose response ties the n-th (KeyPointsFilter::retainBest)."""
import ctypes as C
import hashlib
import math

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as st

import orb_numpy as N
import test_gpu_orb_numpy as G
from conftest import ROOT
from test_kernels_sim import simctx, simlib, simmvo  # noqa: F401  (fixtures)

PATTERN_SHA256 = "2164181aea6ff9ac426ca512d5130d15e1f6e3cd47b1cbdd568bbe1e55d49023"


def oparams(O, kw):
    return O.default_params(**G.params(**kw))


def compare_with_oracle(O, img, kw, what="", descriptors=True):
    """Every stage the oracle exposes against the transcription: raw and blurred levels with their frames, the candidate
    list, the quotas, the keypoint set after both retainBest cuts, the descriptors of the detected keypoints."""
    p = oparams(O, kw)
    orb = N.Orb(**G.params(**kw))
    pyr = orb.pyramid(img)
    assert N.feature_quota(orb.nfeatures, orb.scale_factor, orb.nlevels) == O.feature_quota(p), what
    for l in range(orb.nlevels):
        assert N.level_size(img.shape[1], img.shape[0], orb.scale_factor, l) == O.level_size(img.shape[1], img.shape[0], p, l)
        for bl in (False, True):
            o = O.pyramid_level(img, p, l, bl)
            r = pyr.blur(l) if bl else pyr.raw[l]
            assert o.shape == r.shape and np.array_equal(o, r), "%s: level %d blurred=%d: %s px differ" % (
                what, l, bl, (o != r).sum() if o.shape == r.shape else "shape")
    oc = O.candidates(img, p, cap=1 << 20)
    cand = orb.candidates(img, pyr)
    G.assert_candidates_equal({f: oc[f] for f in N.CANDIDATE_FIELDS}, cand, what)
    k = orb.detect(img, pyr)
    ko = O.calc_keypoints(img, p, cap=1 << 20)
    assert G.sorted_kp(ko).tobytes() == k.tobytes(), "%s: keypoint set %d vs %d" % (what, len(ko), len(k))
    if descriptors:
        kr, dr = orb.compute(img, ko)
        ko2, do = O.calc_descriptors(img, ko, p)
        assert kr.tobytes() == ko2.tobytes() and np.array_equal(dr, do), what
    return orb, cand, k


# ------------------------------------------------------------------------------------------------ stage by stage
@pytest.mark.parametrize("w,h,ch,seed", [(320, 240, 3, 1), (160, 120, 1, 2), (333, 251, 3, 3)])
@pytest.mark.parametrize("interp", [1, 0])
def test_synthetic_frames(O, mvo, w, h, ch, seed, interp):
    img = mvo.synth.small_test_image(seed, w, h, channels=ch)
    _, cand, k = compare_with_oracle(O, img, dict(pyramid_interpolation=interp), "synthetic %dx%d" % (w, h))
    assert len(k) > 50 and len(set(cand["level"].tolist())) == 4


def test_sequence_frame(O, mvo):
    img = mvo.synth.Sequence(640, 480, 2, seed=1234, tex_size=1024).frame(1)
    _, _, k = compare_with_oracle(O, img, {}, "S640")
    assert len(k) > 1500


@pytest.mark.parametrize("kw", G.ADVERSARIAL_SETTINGS, ids=lambda kw: ",".join("%s=%s" % i for i in kw.items()) or "default")
def test_adversarial_images(O, kw):
    w, h = G.ADVERSARIAL_SIZE
    for name, img in G.adversarial_images(w, h):
        compare_with_oracle(O, img, kw, "%s %r" % (name, kw))


def test_adversarial_inputs_reach_their_targets(O):
    """The adversarial set exercises what it is there for: saturated levels, NMS plateaus cut to nothing, retainBest ties."""
    w, h = G.ADVERSARIAL_SIZE
    imgs = dict(G.adversarial_images(w, h))
    orb = N.Orb(**G.params())
    assert (orb.pyramid(imgs["ones255"]).blur(2) == 255).all()               # u8 saturation through resize and blur
    c1 = orb.candidates(imgs["checker1"])
    assert (c1["level"] == 0).sum() == 0 and len(c1["x"]) > 0                 # level 0 a plateau, resized levels are not
    # identical dots: equal FAST scores and equal Harris responses, so retainBest's cuts keep every tie beyond the quota
    dots = orb.candidates(imgs["dots"])
    s0 = dots["fast_score"][dots["level"] == 0]
    assert len(s0) > 60 and (s0 == s0.max()).sum() > 60
    q = N.feature_quota(50, 1.2, 4)
    k = N.Orb(**G.params(nfeatures=50)).detect(imgs["dots"])
    assert 2 * q[0] < len(s0) and (k["octave"] == 0).sum() > q[0]
    assert len(N.Orb(**G.params(nfeatures=1)).detect(imgs["noise"])) >= 1


@pytest.mark.parametrize("w,h", G.HALF_SHAPES)
@pytest.mark.parametrize("interp", [1, 0])
def test_level_sizes_on_exact_halves(O, mvo, w, h, interp):
    """cvRound(w / scale) takes a FLOAT quotient; on these shapes it is exactly x.5 at some level and rounds (half to even)
    to a size the DOUBLE quotient would not give."""
    hits = 0
    for l in range(1, 4):
        for n in (w, h):
            s = N.level_scale(1.2, l)
            q = np.float32(n) / s
            if q == np.floor(q) + np.float32(0.5):
                hits += int(np.rint(q)) != int(round(n / float(s)))
    assert hits > 0
    img = G.textured(w, h, w + h, channels=3)
    compare_with_oracle(O, img, dict(pyramid_interpolation=interp, fast_threshold=10), "%dx%d" % (w, h))


@pytest.mark.parametrize("w,h", G.EDGE_SHAPES)
def test_tile_and_border_edge_shapes(O, w, h):
    img = G.textured(w, h, 5 * w + h)
    compare_with_oracle(O, img, dict(fast_threshold=10), "%dx%d" % (w, h))


def test_edge_shapes_cover_the_tile_edges():
    sizes = set()
    for w, h in G.EDGE_SHAPES:
        for l in range(2):
            lw, lh, _ = N.level_size(w, h, 1.2, l)
            sizes.add(("w", lw % 64))
            sizes.add(("h", lh % 16))
    assert {("w", 1), ("w", 63), ("h", 1), ("h", 15)} <= sizes
    assert {62, 63, 64} <= {n for s in G.EDGE_SHAPES for n in s}


def _oracle_level(O, buf, w, h, stride, ch, p, level, blurred):
    lw, lh, _ = O.level_size(w, h, p, level)
    out = np.zeros((lh + 64, lw + 64), np.uint8)
    r = O.lib().orc_orb_pyramid_level(buf.ctypes.data_as(C.c_void_p), w, h, stride, ch, C.byref(p), level, int(blurred),
                                      out.ctypes.data_as(C.c_void_p))
    assert r == out.size
    return out


def test_padded_strides_and_channel_counts(O):
    """BGR2GRAY in 14-bit fixed point for 1, 3 and 4 channels and any row stride (the oracle called with the padded buffer)."""
    w, h = 193, 145
    rng = np.random.RandomState(9)
    bgra = rng.randint(0, 256, (h, w, 4)).astype(np.uint8)
    p = oparams(O, {})
    for ch in (1, 3, 4):
        src = bgra[:, :, :ch]
        for stride in (w * ch, w * ch + 3, 1024):
            buf = np.zeros((h, stride), np.uint8)
            buf[:, :w * ch] = src.reshape(h, w * ch)
            pyr = N.Pyramid(buf, w=w, h=h, stride=stride, channels=ch)
            for l in (0, 1, 3):
                assert np.array_equal(pyr.raw[l], _oracle_level(O, buf, w, h, stride, ch, p, l, False)), (ch, stride, l)
            assert np.array_equal(pyr.blur(1), _oracle_level(O, buf, w, h, stride, ch, p, 1, True)), (ch, stride)
    # alpha is ignored; one channel is copied
    g = N.gray(bgra)
    assert np.array_equal(g, N.gray(np.ascontiguousarray(bgra[:, :, :3])))
    assert np.array_equal(N.gray(bgra[:, :, :1]), bgra[:, :, 0])
    compare_with_oracle(O, np.ascontiguousarray(bgra), dict(fast_threshold=40), "BGRA")


@settings(max_examples=30, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
@given(w=st.integers(70, 200), h=st.integers(70, 200), nlevels=st.integers(1, 8),
       sf=st.sampled_from([1.1, 1.2, 1.25, 1.5, 2.0]), thr=st.integers(1, 60), interp=st.sampled_from([0, 1]),
       nfeatures=st.sampled_from([0, 1, 50, 500, 8000]), seed=st.integers(0, 2 ** 31 - 1))
def test_random_small_images(O, w, h, nlevels, sf, thr, interp, nfeatures, seed):
    img = G.textured(w, h, seed, channels=1 + 2 * (seed & 1))
    compare_with_oracle(O, img, dict(nlevels=nlevels, scale_factor=sf, fast_threshold=thr, pyramid_interpolation=interp,
                                     nfeatures=nfeatures), "random %dx%d" % (w, h))


# ------------------------------------------------------------------------------------------------ independent float checks
def test_harris_against_float64(mvo):
    """The float32 response against the same formula in float64 from the same integer sums.  Each of a b, c^2 and
    k (a+b)^2 goes through at most five float32 roundings (the operands' conversions, the products, k itself), the two
    subtractions and the scale^4 factor (four roundings) add theirs: |err| <= 16 u (|a b| + c^2 + k (a+b)^2) scale^4,
    u = 2^-24.  The integer sums are checked against a direct 7x7 loop."""
    img = mvo.synth.small_test_image(4, 320, 240, channels=1)
    pyr = N.Pyramid(img)
    c = N.level_candidates(pyr.raw[0], 20)
    assert len(c["x"]) > 200
    F = pyr.raw[0].astype(np.int64)
    for i in range(0, len(c["x"]), max(1, len(c["x"]) // 15)):
        x, y = c["x"][i] + N.BORDER, c["y"][i] + N.BORDER
        a = b = cc = 0
        for yy in range(y - 3, y + 4):
            for xx in range(x - 3, x + 4):
                ix = 2 * (F[yy, xx + 1] - F[yy, xx - 1]) + F[yy - 1, xx + 1] - F[yy - 1, xx - 1] + F[yy + 1, xx + 1] - F[yy + 1, xx - 1]
                iy = 2 * (F[yy + 1, xx] - F[yy - 1, xx]) + F[yy + 1, xx - 1] - F[yy - 1, xx - 1] + F[yy + 1, xx + 1] - F[yy - 1, xx + 1]
                a, b, cc = a + ix * ix, b + iy * iy, cc + ix * iy
        assert (a, b, cc) == (c["a"][i], c["b"][i], c["c"][i])
    a, b, cc = (c[k].astype(np.float64) for k in ("a", "b", "c"))
    s4 = (1.0 / (4 * 7 * 255)) ** 4
    r64 = (a * b - cc * cc - 0.04 * (a + b) ** 2) * s4
    bound = 16 * 2.0 ** -24 * (np.abs(a * b) + cc * cc + 0.04 * (a + b) ** 2) * s4
    err = np.abs(c["harris"].astype(np.float64) - r64)
    assert (err <= bound).all(), (err / bound).max()
    assert np.median(err / bound) < 0.5


def test_angle_against_float64_atan2(mvo):
    img = mvo.synth.small_test_image(6, 320, 240)
    pyr = N.Pyramid(img)
    c = N.level_candidates(pyr.raw[0], 10)
    assert len(c["x"]) > 200
    ref = np.degrees(np.arctan2(c["m01"].astype(np.float64), c["m10"].astype(np.float64))) % 360
    d = np.abs((c["angle"].astype(np.float64) - ref + 180) % 360 - 180)
    assert d.max() < 0.01, d.max()


def test_harris_and_angle_on_analytic_patterns():
    """A straight edge (one gradient direction: a b = c^2) gives a negative response -k (a+b)^2; a corner a positive one;
    a linear ramp I = 128 + 3 (x cos t + y sin t) has its intensity centroid in direction t."""
    F = np.full((80, 80), 40, np.uint8)
    F[:, 40:] = 200
    edge = N.with_frame(F)
    xs, ys = np.array([40, 39, 41]), np.array([40, 30, 50])
    a, b, c = N.gradient_sums(edge, xs, ys)
    assert (b == 0).all() and (c == 0).all() and (a > 0).all()
    assert (N.harris_from_sums(a, b, c) < 0).all()
    corner = np.full((80, 80), 40, np.uint8)
    corner[40:, 40:] = 200
    a, b, c = N.gradient_sums(N.with_frame(corner), np.array([40]), np.array([40]))
    assert N.harris_from_sums(a, b, c)[0] > 0
    yy, xx = np.mgrid[-40:40, -40:40]
    for t in (0, 30, 45, 90, 135, 200, 270, 315, 359):
        r = 128 + 3 * (xx * math.cos(math.radians(t)) + yy * math.sin(math.radians(t)))
        ramp = N.with_frame(np.rint(r).astype(np.uint8))
        m10, m01 = N.moments(ramp, np.array([40]), np.array([40]))
        ang = float(N.fast_atan2(np.float32(m01[0]), np.float32(m10[0])))
        assert abs((ang - t + 180) % 360 - 180) < 0.5, (t, ang)


def test_umax_disc_and_blur_kernel_are_derived():
    assert N.umax_table() == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]
    assert len(N.DISC) == 749
    assert N.GAUSS7.tolist() == [18, 34, 48, 56, 48, 34, 18]
    # the disc is symmetric under transposition (the point of the mirrored umax)
    assert set(map(tuple, N.DISC)) == set(map(tuple, N.DISC[:, ::-1]))


# ------------------------------------------------------------------------------------------------ keypoint lists (points 1, 4)
@pytest.mark.parametrize("w,h", [(320, 240), (177, 126)])
@pytest.mark.parametrize("interp", [1, 0])
def test_keypoint_lists_against_the_oracle(O, w, h, interp):
    img = G.textured(w, h, w * 7 + h, channels=3)
    kw = dict(nlevels=8, pyramid_interpolation=interp)
    orb = N.Orb(**G.params(**kw))
    kps = np.concatenate([G.handmade_keypoints(w, h), G.border_keypoints(w, h)])
    kr, dr, taps = orb.compute(img, kps, want_taps=True)
    ko, do = O.calc_descriptors(img, kps, oparams(O, kw))
    assert kr.tobytes() == ko.tobytes()
    bad = np.nonzero((dr != do).any(1))[0]
    assert len(bad) == 0, "%d descriptors differ, first keypoint %r" % (len(bad), kr[bad[0]] if len(bad) else None)
    # the border filter: rounds half to even, keeps [31, w - 31)
    hm = G.handmade_keypoints(w, h)
    kept = set(map(tuple, kr[["x", "y"]].tolist()))
    for x, y in hm[["x", "y"]].tolist():
        xi, yi = int(np.rint(np.float32(x))), int(np.rint(np.float32(y)))
        assert ((x, y) in kept) == (31 <= xi < w - 31 and 31 <= yi < h - 31), (x, y)
    assert (30.5, h / 2) not in kept and (31.5, h / 2) in kept and (w - 30.5, h / 2) not in kept
    assert ((w - 31.5, h / 2) in kept) == (w % 2 == 0)                     # w - 31.5 rounds to the even neighbour
    # every octave's border keypoints are kept and reach what they are there for
    pyr = orb.pyramid(img, nlevels=8)
    reach = {}
    for (l, tx, ty) in taps:
        lw, lh = pyr.sizes[l]
        near = tx.min() < 3 or ty.min() < 3 or tx.max() >= lw - 3 or ty.max() >= lh - 3
        inside = tx.min() < 0 or ty.min() < 0 or tx.max() >= lw or ty.max() >= lh
        r = reach.setdefault(l, [False, False])
        r[0] |= bool(near)
        r[1] |= bool(inside)
    assert sorted(reach) == list(range(8))
    for l in range(3, 8):
        assert reach[l][0], "octave %d: no tap reads a pixel whose blur reads the frame" % l
    for l in range(4, 8):
        assert reach[l][1], "octave %d: no tap reads the raw frame" % l
    assert not reach[0][1] and not reach[1][1]


def test_brief_table_is_pinned():
    """The 256 rBRIEF pairs of both copies hash to the value computed from an independent copy of the published table
    (scikit-image's orb_descriptor_positions.txt).  |coordinate| <= 13 and the largest tap radius rounds to 18 px, so a rotated
    tap lands within 18 px of the centre; orb_describe_device accepts centres in [-12, L.w + 11], which keeps every tap in
    [-30, L.w + 29] -- inside the 32-px frame."""
    for path in (N.PATTERN_HEADER, ROOT + "/oracle/orb_pattern_31.h"):
        pat = N.load_pattern(path)
        assert hashlib.sha256(pat.astype(np.int8).tobytes()).hexdigest() == PATTERN_SHA256, path
    assert np.abs(pat).max() <= 13
    radius = np.hypot(pat[:, 0::2].astype(float), pat[:, 1::2].astype(float)).max()
    assert round(radius) == 18
    # dense angles through the device's own arithmetic: float32 products, cvRound
    p = pat.astype(np.float32)
    reach = 0
    for deg in np.linspace(0, 360, 2001):
        ang = np.float32(np.float32(deg) * np.float32(math.pi / 180))
        a, b = np.float32(math.cos(float(ang))), np.float32(math.sin(float(ang)))
        reach = max(reach, np.abs(np.rint(p[:, 0::2] * a - p[:, 1::2] * b)).max(), np.abs(np.rint(p[:, 0::2] * b + p[:, 1::2] * a)).max())
    assert reach <= round(radius) == 18
    lo, hi_margin = -12, 11                      # orb_host.cpp: cx < -12 || cx > L.w + 11 is refused
    assert lo - reach >= -N.BORDER and hi_margin + reach <= N.BORDER - 1


# ------------------------------------------------------------------------------------------------ the emulated build
def test_adversarial_images_on_the_emulated_build(simmvo, O, simctx):
    w, h = G.ADVERSARIAL_SIZE
    imgs = G.adversarial_images(w, h)
    for kw in (dict(), dict(fast_threshold=1), dict(nfeatures=1), dict(nlevels=8)):
        for name, img in imgs:
            G.check_adversarial(simmvo, O, simctx, name, img, kw)


@pytest.mark.parametrize("w,h", G.HALF_SHAPES[:2])
def test_half_shapes_on_the_emulated_build(simmvo, O, simctx, w, h):
    G.check_shape(simmvo, O, simctx, G.textured(w, h, w + 3 * h + 3, channels=3), dict(fast_threshold=10), "%dx%d" % (w, h))


def test_keypoint_lists_on_the_emulated_build(simmvo, O):
    """Taps in and next to the raw frame, latency mode (k_brief: window blur, frame rule) and throughput mode (k_blur +
    k_brief_sample), both pyramid flavours."""
    G.check_keypoint_lists(simmvo, O, 320, 240)


def test_input_limits_on_the_emulated_build(simmvo, O, simctx):
    G.check_too_small(simmvo, O, simctx)
