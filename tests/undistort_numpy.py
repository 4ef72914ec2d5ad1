"""TEST AID: cv::undistort(src, dst, K, distCoeffs) with newCameraMatrix = K, transcribed to numpy from the declared
arithmetic of DESIGN.md section 13 -- initUndistortRectifyMap to 1/32 px fixed-point maps, then remap(INTER_LINEAR,
BORDER_CONSTANT, 0).  Vectorised f64 and int64; it shares no code with the product (csrc/undistort_kernels.hip,
csrc/undistort_host.cpp) and is what the MI355X and the emulated build are compared with, bit for bit.  Its own known
answers are in tests/test_undistort_numpy.py."""
import numpy as np

FR1_K = dict(fx=517.3, fy=516.5, cx=325.1, cy=249.7)                  # TUM fr1 (python_tools/undistort_all_images.py)
FR1_DIST = (0.2624, -0.9531, -0.0054, 0.0026, 1.1633)


def coefficients(coeffs):
    """k1, k2, p1, p2, k3, k4, k5, k6 from a vector of 4, 5 or 8 in OpenCV's order; the missing ones are 0."""
    c = [float(v) for v in coeffs]
    if len(c) not in (4, 5, 8):
        raise ValueError("4, 5 or 8 distortion coefficients")
    return c + [0.0] * (8 - len(c))


def cv_round_i32(a):
    """cvRound to int32: nearest, halves to even; beyond the int32 range the conversion saturates, NaN gives 0."""
    r = np.rint(np.asarray(a, np.float64))
    r = np.where(np.isnan(r), 0.0, r)
    return np.clip(r, -2147483648.0, 2147483647.0).astype(np.int64).astype(np.int32)


def fixed_point_coordinates(K, coeffs, w, h):
    """(iu, iv) = cvRound(32 u), cvRound(32 v) per output pixel, h x w int32."""
    k1, k2, p1, p2, k3, k4, k5, k6 = coefficients(coeffs)
    fx, fy, cx, cy = float(K["fx"]), float(K["fy"]), float(K["cx"]), float(K["cy"])
    j = np.arange(w, dtype=np.float64)[None, :]
    i = np.arange(h, dtype=np.float64)[:, None]
    x = np.broadcast_to((j - cx) * (1.0 / fx), (h, w))
    y = np.broadcast_to((i - cy) * (1.0 / fy), (h, w))
    x2 = x * x
    y2 = y * y
    r2 = x2 + y2
    _2xy = 2 * x * y
    with np.errstate(all="ignore"):
        kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
        u = fx * (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)) + cx
        v = fy * (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy) + cy
        return cv_round_i32(u * 32), cv_round_i32(v * 32)


def split(iu):
    """integer coordinate (arithmetic shift) and 1/32 px fraction (mask) of a fixed-point coordinate"""
    iu = np.asarray(iu, np.int32)
    return iu >> 5, (iu & 31).astype(np.uint8)


def undistort_map(K, coeffs, w, h):
    """-> ix, iy (int32), ax, ay (uint8), each h x w"""
    iu, iv = fixed_point_coordinates(K, coeffs, w, h)
    ix, ax = split(iu)
    iy, ay = split(iv)
    return ix, iy, ax, ay


def taps_inside(ix, iy, w, h):
    """[4, ...] bool: which of the taps (iy, ix), (iy, ix+1), (iy+1, ix), (iy+1, ix+1) lie inside a w x h source"""
    ix, iy = np.asarray(ix, np.int64), np.asarray(iy, np.int64)
    return np.stack([(yy >= 0) & (yy < h) & (xx >= 0) & (xx < w) for yy, xx in ((iy, ix), (iy, ix + 1), (iy + 1, ix), (iy + 1, ix + 1))])


def remap(src, ix, iy, ax, ay):
    """remap(INTER_LINEAR, BORDER_CONSTANT, 0) of a u8 image (h x w or h x w x c) through maps of any shape"""
    src = np.asarray(src, np.uint8)
    img = src[:, :, None] if src.ndim == 2 else src
    h, w = img.shape[:2]
    ix, iy = np.asarray(ix, np.int64), np.asarray(iy, np.int64)
    ax, ay = np.asarray(ax, np.int64), np.asarray(ay, np.int64)
    inside = taps_inside(ix, iy, w, h)
    weights = (32 * (32 - ay) * (32 - ax), 32 * (32 - ay) * ax, 32 * ay * (32 - ax), 32 * ay * ax)
    acc = np.zeros(ix.shape + (img.shape[2],), np.int64)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        yy, xx = np.clip(iy + dy, 0, h - 1), np.clip(ix + dx, 0, w - 1)
        tap = np.where(inside[k][..., None], img[yy, xx].astype(np.int64), 0)
        acc += weights[k][..., None] * tap
    out = ((acc + 16384) >> 15).astype(np.uint8)
    return out[..., 0] if src.ndim == 2 else out


def undistort(img, K, coeffs):
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    return remap(img, *undistort_map(K, coeffs, w, h))
