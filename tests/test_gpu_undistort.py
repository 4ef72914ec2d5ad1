"""Undistortion on the MI355X (csrc/undistort_kernels.hip, csrc/undistort_host.cpp) against tests/undistort_numpy.py, the
independent numpy transcription of the declared arithmetic: map and image bit for bit, no tolerance
anywhere.  The shapes are the smallest at which the kernels can go wrong (tests/test_undistort_numpy.py counts what each of
them reaches): A 67 x 35, no multiple of a wave, every border branch; B the barrel sign with every tap inside; C 160 x 120 x 4
with padded rows on both sides; D the real configuration, 640 x 480 x 3 with the TUM fr1 calibration, once.  Then the wiring of
host/driver/run_vo (`camera_info.k1 .. k3` in the dataset section).  The bodies are shared with tests/test_undistort_sim.py,
which runs them on the emulated build without a GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import run_vo_init_body as B
import undistort_numpy as U
import vo_chain
from test_undistort_numpy import CASE_A, CASE_B, CASE_C, CASE_D

pytestmark = pytest.mark.gpu

CASES = dict(A=CASE_A, B=CASE_B, C=CASE_C, D=CASE_D)
SENTINEL = 0xA5


def _to_device(a):
    import torch
    t = torch.from_numpy(np.array(a)).cuda()                # (a copy: the shared images are read-only)
    torch.cuda.synchronize()
    return t


def _to_host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def image(w, h, ch, seed=0):
    """seeded random u8, not a constant: a wrong tap cannot hide"""
    img = np.random.RandomState(1000 * seed + 10 * w + ch).randint(0, 256, (h, w, ch)).astype(np.uint8)
    img = img[:, :, 0].copy() if ch == 1 else img
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def reference(name, ch):
    """(map, image) of the transcription for a case, computed once and shared"""
    K, dist, w, h = CASES[name]
    m = U.undistort_map(K, dist, w, h)
    out = U.remap(image(w, h, ch), *m)
    for a in m + (out,):
        a.setflags(write=False)
    return m, out


def assert_map_equal(got, want, what):
    for g, t, n in zip(got, want, ("ix", "iy", "ax", "ay")):
        assert g.dtype == t.dtype and g.shape == t.shape, (what, n, g.dtype, g.shape)
        bad = np.argwhere(g != t)
        assert len(bad) == 0, "%s: %s differs at %d pixels, first at %s: %d, transcription %d" % (
            what, n, len(bad), bad[0], g[tuple(bad[0])], t[tuple(bad[0])])


def assert_image_equal(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d values differ, first at %s: %d, transcription %d" % (
        what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("name,ch", [("A", 1), ("A", 3), ("B", 1), ("D", 3)])
def test_map_and_image_equal_the_transcription(ctx, name, ch):
    K, dist, w, h = CASES[name]
    want_map, want = reference(name, ch)
    ctx.undistort_configure(K, dist, w, h)
    assert_map_equal(ctx.debug_undistort_map(), want_map, "case " + name)
    assert_image_equal(ctx.undistort(image(w, h, ch)), want, "case %s, %d channels" % (name, ch))


def padded(img, stride, fill=SENTINEL):
    """rows of `stride` bytes, the padding filled with the sentinel"""
    h = img.shape[0]
    buf = np.full((h, stride), fill, np.uint8)
    buf[:, :img[0].size] = img.reshape(h, -1)
    return buf


def test_four_channels_with_padded_rows(ctx):
    """Case C: source stride 4 w + 12, output stride 4 w + 20; the bytes of the output padding stay untouched."""
    K, dist, w, h = CASES["C"]
    want_map, want = reference("C", 4)
    stride, out_stride = 4 * w + 12, 4 * w + 20
    src = padded(image(w, h, 4), stride, fill=0x3C)      # (a padding byte read as a tap would show in the image)
    out = np.full((h, out_stride), SENTINEL, np.uint8)
    ctx.undistort_configure(K, dist, w, h)
    assert_map_equal(ctx.debug_undistort_map(), want_map, "case C")
    ctx._chk(ctx.lib.mvo_undistort(ctx.h, C.c_void_p(src.ctypes.data), w, h, stride, 4, C.c_void_p(out.ctypes.data), out_stride))
    assert_image_equal(out[:, :4 * w].reshape(h, w, 4), want, "case C")
    assert (out[:, 4 * w:] == SENTINEL).all(), "the padding of the output rows was written"


def test_device_pointer_form_equals_the_host_form(ctx):
    """mvo_undistort_dev on case C's padded rows (the kernel itself honours both strides) and packed on case A."""
    for name, ch, pad_in, pad_out in (("C", 4, 12, 20), ("A", 3, 0, 0), ("A", 1, 5, 3)):
        K, dist, w, h = CASES[name]
        _, want = reference(name, ch)
        stride, out_stride = w * ch + pad_in, w * ch + pad_out
        ctx.undistort_configure(K, dist, w, h)
        host = ctx.undistort(image(w, h, ch))
        assert_image_equal(host, want, "host form, case " + name)
        d_in = _to_device(padded(image(w, h, ch), stride, fill=0x3C))
        d_out = _to_device(np.full((h, out_stride), SENTINEL, np.uint8))
        ctx.undistort_dev(d_in.data_ptr(), d_out.data_ptr(), w, h, stride, ch, out_stride)
        ctx.synchronize()
        got = _to_host(d_out)
        assert_image_equal(got[:, :w * ch].reshape(host.shape), host, "device form, case %s, %d channels" % (name, ch))
        assert (got[:, w * ch:] == SENTINEL).all(), "the padding of the device output rows was written"


def test_eight_coefficients_map(ctx):
    K, dist, w, h = CASES["A"]
    dist8 = tuple(dist) + (0.02, -0.01, 0.003)
    ctx.undistort_configure(K, dist8, w, h)
    got = ctx.debug_undistort_map()
    assert_map_equal(got, U.undistort_map(K, dist8, w, h), "8 coefficients")
    assert not np.array_equal(got[0], reference("A", 1)[0][0])     # (k4..k6 do change the map)


def test_zero_coefficients_return_the_input(ctx):
    K, _, w, h = CASES["A"]
    for ch, dist in ((1, (0, 0, 0, 0)), (3, (0, 0, 0, 0, 0))):
        ctx.undistort_configure(K, dist, w, h)
        ix, iy, ax, ay = ctx.debug_undistort_map()
        jj, ii = np.meshgrid(np.arange(w), np.arange(h))
        assert np.array_equal(ix, jj) and np.array_equal(iy, ii) and not ax.any() and not ay.any()
        assert_image_equal(ctx.undistort(image(w, h, ch)), image(w, h, ch), "zero coefficients")   # last row and column too


def test_configure_again_replaces_the_map(ctx):
    K, dist, w, h = CASES["A"]
    K2 = dict(K, fx=37.5, cx=30.0)
    img = image(w, h, 3)
    ctx.undistort_configure(K, dist, w, h)
    first = ctx.undistort(img)
    ctx.undistort_configure(K2, dist, w, h)
    assert_map_equal(ctx.debug_undistort_map(), U.undistort_map(K2, dist, w, h), "second configuration")
    second = ctx.undistort(img)
    assert_image_equal(second, U.undistort(img, K2, dist), "second configuration")
    assert not np.array_equal(first, second)
    ctx.undistort_configure(K2, dist, w, h)               # the same values again: the map stays
    assert_image_equal(ctx.undistort(img), second, "configured twice with the same values")
    ctx.undistort_configure(K, dist, w, h)                # and back
    assert_image_equal(ctx.undistort(img), reference("A", 3)[1], "first configuration again")
    # another size rebuilds the map as well
    Kb, distb, wb, hb = CASES["B"]
    ctx.undistort_configure(Kb, distb, wb + 4, hb - 2)
    assert_map_equal(ctx.debug_undistort_map(), U.undistort_map(Kb, distb, wb + 4, hb - 2), "another size")


def errors(mvo, c):
    """every error with its code, on a context `c` that has never been configured"""
    K, dist, w, h = CASES["A"]
    img = image(w, h, 3)

    def code(fn, *a):
        with pytest.raises(mvo.MvoError) as e:
            fn(*a)
        return e.value.code

    def raw(src, ww, hh, stride, ch, out_stride):
        out = np.zeros(max(hh * out_stride, 1), np.uint8)
        c._chk(c.lib.mvo_undistort(c.h, C.c_void_p(src.ctypes.data), ww, hh, stride, ch, C.c_void_p(out.ctypes.data), out_stride))

    def raw_dev(d_in, d_out, ww, hh, stride, ch, out_stride):
        c.undistort_dev(d_in.data_ptr(), d_out.data_ptr(), ww, hh, stride, ch, out_stride)

    flat = np.ascontiguousarray(img).reshape(-1)
    d_in, d_out = _to_device(img), _to_device(np.zeros_like(img))
    # before a configuration
    assert code(c.undistort, img) == mvo.MVO_ERR_STATE
    assert code(raw_dev, d_in, d_out, w, h, 3 * w, 3, 3 * w) == mvo.MVO_ERR_STATE
    n = w * h
    bufs = [np.zeros(n, t) for t in (np.int32, np.int32, np.uint8, np.uint8)]
    ptrs = [C.c_void_p(b.ctypes.data) for b in bufs]
    assert c.lib.mvo_debug_get_undistort_map(c.h, *ptrs, n) == mvo.MVO_ERR_STATE
    # configurations that are refused leave the context unconfigured
    assert code(c.undistort_configure, K, [0.0] * 12, w, h) == mvo.MVO_ERR_INVALID      # thin prism model
    assert code(c.undistort_configure, K, [0.0] * 14, w, h) == mvo.MVO_ERR_INVALID      # tilt model
    assert code(c.undistort_configure, K, [0.0] * 3, w, h) == mvo.MVO_ERR_INVALID
    assert code(c.undistort_configure, dict(K, fx=0.0), dist, w, h) == mvo.MVO_ERR_INVALID
    assert code(c.undistort_configure, dict(K, fy=0.0), dist, w, h) == mvo.MVO_ERR_INVALID
    assert code(c.undistort_configure, dict(K, cx=float("nan")), dist, w, h) == mvo.MVO_ERR_INVALID
    assert code(c.undistort_configure, K, dist, 8193, h) == mvo.MVO_ERR_INVALID
    assert code(c.undistort_configure, K, dist, 0, h) == mvo.MVO_ERR_INVALID
    assert code(c.undistort, img) == mvo.MVO_ERR_STATE
    c.undistort_configure(K, dist, w, h)
    assert_image_equal(c.undistort(img), reference("A", 3)[1], "after the refused configurations")
    # a size other than the configured one
    assert code(c.undistort, image(w + 1, h, 3)) == mvo.MVO_ERR_STATE
    assert code(c.undistort, image(w, h - 1, 3)) == mvo.MVO_ERR_STATE
    assert code(raw_dev, d_in, d_out, w - 1, h, 3 * w, 3, 3 * w) == mvo.MVO_ERR_STATE
    # bad arguments
    assert code(raw, flat, w, h, 2 * w, 2, 2 * w) == mvo.MVO_ERR_INVALID                # channels = 2
    assert code(raw, flat, w, h, 3 * w - 1, 3, 3 * w) == mvo.MVO_ERR_INVALID            # source stride too small
    assert code(raw, flat, w, h, 3 * w, 3, 3 * w - 1) == mvo.MVO_ERR_INVALID            # output stride too small
    assert code(raw_dev, d_in, d_out, w, h, 3 * w, 2, 3 * w) == mvo.MVO_ERR_INVALID
    assert code(raw_dev, d_in, d_in, w, h, 3 * w, 3, 3 * w) == mvo.MVO_ERR_INVALID      # d_out must not alias d_image
    assert c.lib.mvo_undistort(c.h, None, w, h, 3 * w, 3, ptrs[2], 3 * w) == mvo.MVO_ERR_INVALID
    # the debug getter with too small a buffer
    assert c.lib.mvo_debug_get_undistort_map(c.h, *ptrs, n - 1) == mvo.MVO_ERR_CAPACITY
    assert c.lib.mvo_debug_get_undistort_map(c.h, *ptrs, n) == mvo.MVO_OK
    assert np.array_equal(bufs[0].reshape(h, w), reference("A", 1)[0][0])
    # a refused configuration keeps the one in force
    assert code(c.undistort_configure, K, [0.0] * 12, w, h) == mvo.MVO_ERR_INVALID
    assert_image_equal(c.undistort(img), reference("A", 3)[1], "after a refused configuration")


def test_errors(mvo):
    c = mvo.Context(0)
    try:
        errors(mvo, c)
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ run_vo
N_RUN = 3                                              # frames per run: the first keyframe and two initialisation frames
RUN_DIST = dict(k1=-0.21, k2=0.06, p1=0.0012, p2=-0.0021, k3=0.011)
DIST_KEYS = ("k1", "k2", "p1", "p2", "k3")


def write_run_images(tmp_path):
    from PIL import Image
    data = tmp_path / "dataset"
    data.mkdir()
    for i in range(N_RUN):
        Image.fromarray(B.sequence()[1][i][:, :, ::-1]).save(data / ("rgb_%05d.png" % i))
    return data


def start_runs(tmp_path, data, timeout=300):
    """Three runs of host/driver/run_vo from images alone on the same files: with camera_info.k1 .. k3 set, with the five
    keys present and 0, and without the keys."""
    runs = {}
    for name, dist in (("distorted", RUN_DIST), ("zeros", dict.fromkeys(DIST_KEYS, 0.0)), ("plain", None)):
        log = tmp_path / (name + ".log")
        ds = "" if dist is None else "".join("  camera_info.%s: %r\n" % (k, dist[k]) for k in DIST_KEYS)
        cfg, traj = B.write_config(tmp_path, data, name, dataset_extra=ds, extra="max_num_imgs_to_proc: %d\ninit_from_images: 1\n"
                                   "save_frame_log_to: %s\n%s" % (N_RUN, log, B.INIT_YAML % B.INIT_PARAMS))
        runs[name] = B.Run(cfg, traj, log, timeout)
    return runs


def run_vo_wiring(mvo, runs, data):
    from PIL import Image
    K = B.sequence()[0].K
    files = [np.ascontiguousarray(np.asarray(Image.open(data / ("rgb_%05d.png" % i)).convert("RGB"))[:, :, ::-1]) for i in range(N_RUN)]
    logs = {}
    for name, r in runs.items():
        r.wait()
        logs[name] = vo_chain.read_frame_log(r.log)
        assert len(logs[name]) == N_RUN, name
    said = "undistorting every image"
    assert said in runs["distorted"].stdout and said in runs["zeros"].stdout
    assert said not in runs["plain"].stdout               # no keys: no call, no message

    def extract(c, img):
        k = c.calc_keypoints(img)
        k, d = c.calc_descriptors(img, k, reuse_pyramid=True)
        return k, d

    c = mvo.Context(0, max_keypoints=B.MAX_KEYPOINTS)       # (a context of its own: the grid is latched from the first image)
    try:
        h, w = files[0].shape[:2]
        c.undistort_configure(K, [RUN_DIST[k] for k in DIST_KEYS], w, h)
        n_changed = 0
        for i, img in enumerate(files):
            # (a) the frame holds the undistorted image: keypoints and descriptors are those of Context.undistort + extraction
            und = c.undistort(img)
            assert_image_equal(und, U.undistort(img, K, [RUN_DIST[k] for k in DIST_KEYS]), "frame %d" % i)
            k, d = extract(c, und)
            rec = logs["distorted"][i]
            assert rec["KPTS"] == k.tobytes(), "frame %d: keypoints of the undistorted run" % i
            assert rec["DESC"] == d.tobytes(), "frame %d: descriptors of the undistorted run" % i
            # (c) without the keys nothing is undistorted
            k0, d0 = extract(c, img)
            assert logs["plain"][i]["KPTS"] == k0.tobytes() and logs["plain"][i]["DESC"] == d0.tobytes(), "frame %d: the run without the keys" % i
            n_changed += rec["KPTS"] != logs["plain"][i]["KPTS"]
        assert n_changed == N_RUN                          # (the distortion does change what is extracted)
    finally:
        c.close()
    # (b) five keys that are 0: the identity map, the frame log is that of the run without the keys byte for byte
    assert runs["zeros"].log.read_bytes() == runs["plain"].log.read_bytes()
    assert runs["zeros"].traj.read_text() == runs["plain"].traj.read_text()
    assert runs["distorted"].log.read_bytes() != runs["plain"].log.read_bytes()


def test_run_vo_undistorts_when_the_config_asks_for_it(mvo, tmp_path):
    data = write_run_images(tmp_path)
    run_vo_wiring(mvo, start_runs(tmp_path, data), data)
