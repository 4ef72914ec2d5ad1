"""mvo_amd -- MI355X-native per-frame VO hot path (ORB extract + Hamming match + sliding-window BA).

This package is plumbing around ``csrc/libmvo_hip.so`` (hand-written HIP kernels behind the C-ABI declared
in ``include/mvo_hip.h``).  The Python layer only mirrors the reference's *interface* for this path
(``my_slam::geometry`` / ``my_slam::optimization`` free functions, same names and argument meaning) so that
tests read like the reference's own call sites; the product host code for a C++ caller is the header-only
adapter under ``host/include/my_slam``.

There is NO CPU fallback: if the HIP library is missing or no GPU is visible, construction fails loudly.
The directory name contains a '-', so import it through ``__graft_entry__.load_package()`` (module name
``mvo_amd``).
"""
import ctypes as C
import os

import numpy as np

from . import synth  # noqa: F401  (synthetic workloads)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libmvo_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "mvo_hip.h")

MVO_OK, MVO_ERR_INVALID, MVO_ERR_NO_DEVICE, MVO_ERR_CAPACITY, MVO_ERR_HIP, MVO_ERR_STATE = 0, -1, -2, -3, -4, -5

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])   # cv::KeyPoint
DMATCH_DTYPE = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
CANDIDATE_DTYPE = np.dtype([("x", "<i2"), ("y", "<i2"), ("level_score", "<i4"), ("harris", "<f4"), ("angle", "<f4")])
DISTRIBUTE_CANDIDATE_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("level", "<i4"), ("score", "<i4")])


class OrbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("fast_threshold", C.c_int32), ("max_keypoints", C.c_int32), ("grid_size", C.c_int32),
                ("grid_max_per_cell", C.c_int32), ("pyramid_interpolation", C.c_int32)]


class OrbDistributeParams(C.Structure):
    _fields_ = [("ini_threshold", C.c_int32), ("min_threshold", C.c_int32), ("cell_size", C.c_int32),
                ("edge_threshold", C.c_int32)]


class BaProblem(C.Structure):
    _fields_ = [("n_poses", C.c_int32), ("n_points", C.c_int32), ("n_edges", C.c_int32),
                ("pose_T_w_c", C.c_void_p), ("points", C.c_void_p), ("edge_pose", C.c_void_p),
                ("edge_point", C.c_void_p), ("edge_uv", C.c_void_p), ("focal", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double), ("info", C.c_double * 4),
                ("huber_delta", C.c_double), ("fix_points", C.c_int32), ("pose_fixed", C.c_void_p),
                ("max_iterations", C.c_int32)]


class BaStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("trials", C.c_int32), ("terminated", C.c_int32), ("failed_solves", C.c_int32),
                ("chi2_initial", C.c_double), ("chi2_final", C.c_double), ("lambda_final", C.c_double),
                ("stale_steps", C.c_int32), ("reserved_", C.c_int32)]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int64), ("total_ms", C.c_double)]


class MvoError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libmvo_hip error %d: %s" % (code, msg))
        self.code = code


class UndistortParams(C.Structure):
    """mvo_undistort_params (include/mvo_hip.h)."""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("coeffs", C.c_double * 8), ("n_coeffs", C.c_int32)]


class MapRefineParams(C.Structure):
    """mvo_map_refine_params (include/mvo_hip.h)."""
    _fields_ = [("max_trials", C.c_int32), ("min_observations", C.c_int32), ("huber_delta", C.c_double), ("rel_tolerance", C.c_double)]


class FuseFrame(C.Structure):
    """mvo_fuse_frame (include/mvo_hip.h)."""
    _fields_ = [("desc", C.c_void_p), ("xy", C.c_void_p), ("scale", C.c_void_p), ("conn", C.c_void_p), ("n", C.c_int32),
                ("T_w_c", C.c_double * 16)]


class MapFuseParams(C.Structure):
    """mvo_map_fuse_params (include/mvo_hip.h)."""
    _fields_ = [("max_px", C.c_double), ("max_hamming", C.c_int32)]


FUSE_OBSERVATION_DTYPE = np.dtype([("frame", np.int32), ("keypoint", np.int32), ("point", np.int32)])


class WindowTriangulateParams(C.Structure):
    """mvo_window_triangulate_params (include/mvo_hip.h)."""
    _fields_ = [("max_line_px", C.c_double), ("lowe_ratio", C.c_double), ("max_hamming", C.c_int32), ("max_cos_parallax", C.c_double),
                ("max_reproj_chi2", C.c_double), ("ratio_factor", C.c_double), ("min_baseline", C.c_double)]


WINDOW_TRIANGULATE_DEFAULTS = dict(max_line_px=2.0, lowe_ratio=0.8, max_hamming=64, max_cos_parallax=0.9998, max_reproj_chi2=5.991,
                                   ratio_factor=1.8, min_baseline=0.0)
# mvo_window_pair, mvo_window_point (include/mvo_hip.h), with the padding the C compiler puts in front of the double
WINDOW_PAIR_DTYPE = np.dtype([("frame", np.int32), ("keypoint", np.int32), ("train", np.int32), ("hamming", np.int32),
                              ("status", np.int32), ("p_curr", np.float32, 3), ("p_frame", np.float32, 3), ("cos2", np.float64)],
                             align=True)
WINDOW_POINT_DTYPE = np.dtype([("keypoint", np.int32), ("frame", np.int32), ("train", np.int32), ("hamming", np.int32),
                               ("p_curr", np.float32, 3), ("cos2", np.float64)], align=True)
assert WINDOW_PAIR_DTYPE.itemsize == 56 and WINDOW_POINT_DTYPE.itemsize == 40


class PoseOptimizeParams(C.Structure):
    """mvo_pose_optimize_params (include/mvo_hip.h)."""
    _fields_ = [("rounds", C.c_int32), ("iterations", C.c_int32), ("min_inliers", C.c_int32), ("chi2_threshold", C.c_double),
                ("huber_delta", C.c_double), ("rel_tolerance", C.c_double)]


class LocalMapParams(C.Structure):
    """mvo_local_map_params (include/mvo_hip.h)."""
    _fields_ = [("min_view_cos", C.c_double), ("radius_near", C.c_double), ("radius_far", C.c_double), ("near_cos", C.c_double),
                ("radius_scale", C.c_double), ("lowe_ratio", C.c_double), ("max_hamming", C.c_int32), ("pad", C.c_int32)]


LOCAL_MAP_DEFAULTS = dict(min_view_cos=0.5, radius_near=2.5, radius_far=4.0, near_cos=0.998, radius_scale=1.0, lowe_ratio=0.8,
                          max_hamming=100)


class InitPoses(C.Structure):
    """mvo_init_poses (include/mvo_hip.h)."""
    _fields_ = [("inliers_e", C.c_void_p), ("inliers_h", C.c_void_p), ("cap_inliers", C.c_int), ("pts3d", C.c_void_p),
                ("cap_pts", C.c_int), ("E", C.c_double * 9), ("H", C.c_double * 9), ("found_e", C.c_int),
                ("found_h", C.c_int), ("n_inliers_e", C.c_int), ("n_inliers_h", C.c_int), ("n_slots", C.c_int),
                ("present", C.c_int32 * 5), ("h_candidate", C.c_int32 * 5), ("pts_offset", C.c_int32 * 5),
                ("pts_count", C.c_int32 * 5), ("R", C.c_double * 45), ("t", C.c_double * 15), ("normal", C.c_double * 15),
                ("score_e", C.c_double), ("score_h", C.c_double), ("ratio", C.c_double), ("best", C.c_int)]


class InitParams(C.Structure):
    """mvo_init_params (include/mvo_hip.h)."""
    _fields_ = [("min_triang_angle", C.c_double), ("max_ratio_to_median", C.c_double), ("assumed_mean_depth", C.c_double),
                ("min_inlier_matches", C.c_int), ("min_pixel_dist", C.c_double),
                ("min_median_triangulation_angle", C.c_double)]


class InitResult(C.Structure):
    """mvo_init_result (include/mvo_hip.h)."""
    _fields_ = [("matches_for_3d", C.c_void_p), ("pts3d_in_curr", C.c_void_p), ("angles", C.c_void_p), ("cap", C.c_int),
                ("slot", C.c_int), ("n_slot_inliers", C.c_int), ("n_kept", C.c_int), ("scaled", C.c_int),
                ("R", C.c_double * 9), ("t", C.c_double * 3), ("T_w_c", C.c_double * 16), ("mean_depth", C.c_double),
                ("scale", C.c_double), ("mean_pixel_dist", C.c_double), ("mean_angle", C.c_double),
                ("median_angle", C.c_double), ("min_angle", C.c_double), ("max_angle", C.c_double),
                ("criteria", C.c_int * 3), ("good", C.c_int)]


_lib = None


def load_library():
    """Loads csrc/libmvo_hip.so.  Fails loudly when the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("HIP extension %s is missing -- run __graft_entry__.build() (hipcc, gfx950). "
                          "There is no CPU fallback." % LIB_PATH)
    try:
        # torch bundles its own libamdhip64; when both end up in one process the FIRST one loaded must be
        # torch's (otherwise torch.cuda reports "No HIP GPUs are available"), so import it before dlopen.
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    lib.mvo_last_error.restype = C.c_char_p
    lib.mvo_destroy.restype = None
    _lib = lib
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _image_args(img):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.ndim == 2:
        h, w = img.shape
        ch = 1
    else:
        h, w, ch = img.shape
    return img, w, h, w * ch, ch


class Context:
    """One mvo_ctx (= one HIP stream).  Not thread-safe; use one per host thread."""

    def __init__(self, device=0, **orb_params):
        self.lib = load_library()
        h = C.c_void_p()
        r = self.lib.mvo_create(C.byref(h), int(device))
        if r != MVO_OK:
            raise MvoError(r, "mvo_create failed (no usable HIP device?) -- there is no CPU fallback")
        self.h = h
        self.device = int(device)
        self.params = dict(nfeatures=8000, scale_factor=1.2, nlevels=4, fast_threshold=20, max_keypoints=1500,
                           grid_size=16, grid_max_per_cell=8,  # config/config.yaml:65-69,94-95
                           pyramid_interpolation=1)             # cv::ORB of OpenCV >= 3.4: INTER_LINEAR_EXACT
        if orb_params:
            self.orb_configure(**orb_params)

    def sibling(self):
        """A second context of this host thread on THIS context's stream (mvo_create_sibling); close it before its parent."""
        c = Context.__new__(Context)
        c.lib = self.lib
        h = C.c_void_p()
        r = self.lib.mvo_create_sibling(self.h, C.byref(h))
        if r != MVO_OK:
            raise MvoError(r, "mvo_create_sibling failed")
        c.h, c.device, c.params = h, self.device, dict(self.params)
        c._parent = self   # (keeps the parent alive as long as the sibling)
        return c

    def close(self):
        if getattr(self, "h", None):
            self.lib.mvo_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, r):
        if r != MVO_OK:
            raise MvoError(r, (self.lib.mvo_last_error(self.h) or b"").decode())

    # ---- extraction
    def orb_configure(self, **kw):
        new = dict(self.params)
        new.update(kw)
        p = OrbParams(**new)
        self._chk(self.lib.mvo_orb_configure(self.h, C.byref(p)))
        self.params = new

    def calc_keypoints(self, image, cap=None):
        """geometry::calcKeyPoints (feature_match.cpp:11-36)."""
        img, w, h, stride, ch = _image_args(image)
        self._w, self._h = w, h
        cap = cap or (self.params["max_keypoints"] + 16)
        out = np.zeros(cap, KEYPOINT_DTYPE)
        n = C.c_int()
        self._chk(self.lib.mvo_calc_keypoints(self.h, _p(img), w, h, stride, ch, _p(out), cap, C.byref(n)))
        return out[:n.value].copy()

    def calc_keypoints_dev(self, d_ptr, w, h, stride, ch, cap=None):
        self._w, self._h = w, h
        cap = cap or (self.params["max_keypoints"] + 16)
        out = np.zeros(cap, KEYPOINT_DTYPE)
        n = C.c_int()
        self._chk(self.lib.mvo_calc_keypoints_dev(self.h, C.c_void_p(d_ptr), w, h, stride, ch, _p(out), cap, C.byref(n)))
        return out[:n.value].copy()

    def orb_distribute_configure(self, ini_threshold=20, min_threshold=7, cell_size=30, edge_threshold=19):
        """Parameters of calc_keypoints_distributed (mvo_orb_distribute_configure)."""
        p = OrbDistributeParams(int(ini_threshold), int(min_threshold), int(cell_size), int(edge_threshold))
        self._chk(self.lib.mvo_orb_distribute_configure(self.h, C.byref(p)))

    def calc_keypoints_distributed(self, image, cap=None):
        """The ORB-SLAM style detector: cell-wise FAST with two thresholds and a quadtree spread per level."""
        img, w, h, stride, ch = _image_args(image)
        self._w, self._h = w, h
        cap = cap or (self.params["max_keypoints"] + 16)
        out = np.zeros(cap, KEYPOINT_DTYPE)
        n = C.c_int()
        self._chk(self.lib.mvo_calc_keypoints_distributed(self.h, _p(img), w, h, stride, ch, _p(out), cap, C.byref(n)))
        return out[:n.value].copy()

    def calc_keypoints_distributed_dev(self, d_ptr, w, h, stride, ch, cap=None):
        self._w, self._h = w, h
        cap = cap or (self.params["max_keypoints"] + 16)
        out = np.zeros(cap, KEYPOINT_DTYPE)
        n = C.c_int()
        self._chk(self.lib.mvo_calc_keypoints_distributed_dev(self.h, C.c_void_p(d_ptr), w, h, stride, ch, _p(out), cap,
                                                              C.byref(n)))
        return out[:n.value].copy()

    def debug_distribute_candidates(self):
        """The candidates of the last calc_keypoints_distributed* in their declared order."""
        n = C.c_int()
        self._chk(self.lib.mvo_debug_get_distribute_candidates(self.h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), DISTRIBUTE_CANDIDATE_DTYPE)
        self._chk(self.lib.mvo_debug_get_distribute_candidates(self.h, _p(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def calc_descriptors(self, image, kps, reuse_pyramid=False, want_rgb=False):
        """geometry::calcDescriptors (feature_match.cpp:38-49): returns (keypoints', descriptors[, rgb])."""
        kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE).copy()
        n = C.c_int(len(kps))
        desc = np.zeros((max(len(kps), 1), 32), np.uint8)
        rgb = np.zeros((max(len(kps), 1), 3), np.uint8) if want_rgb else None
        if image is None:
            img, w, h, stride, ch = None, self._w, self._h, 0, 1
        else:
            img, w, h, stride, ch = _image_args(image)
        self._chk(self.lib.mvo_calc_descriptors(self.h, _p(img), w, h, stride, ch, int(reuse_pyramid), _p(kps),
                                                C.byref(n), _p(desc), _p(rgb)))
        if want_rgb:
            return kps[:n.value].copy(), desc[:n.value].copy(), rgb[:n.value].copy()
        return kps[:n.value].copy(), desc[:n.value].copy()

    def calc_descriptors_dev(self, kps, want_host=True):
        kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE).copy()
        n = C.c_int(len(kps))
        desc = np.zeros((max(len(kps), 1), 32), np.uint8) if want_host else None
        dptr = C.c_void_p()
        self._chk(self.lib.mvo_calc_descriptors_dev(self.h, _p(kps), C.byref(n), _p(desc), C.byref(dptr)))
        return kps[:n.value].copy(), (desc[:n.value].copy() if want_host else None), dptr.value

    def select_uniform_kpts_by_grid(self, kps, image_rows, image_cols):
        kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE).copy()
        n = C.c_int(len(kps))
        self._chk(self.lib.mvo_select_uniform_kpts_by_grid(self.h, _p(kps), C.byref(n), image_rows, image_cols))
        return kps[:n.value].copy()

    # ---- undistortion (python_tools/undistort_all_images.py:11-37)
    def undistort_configure(self, K, coeffs, width, height):
        """mvo_undistort_configure: K = dict(fx, fy, cx, cy), coeffs in OpenCV's order k1, k2, p1, p2[, k3[, k4, k5, k6]]."""
        c = np.ascontiguousarray(coeffs, np.float64).reshape(-1)
        p = UndistortParams(float(K["fx"]), float(K["fy"]), float(K["cx"]), float(K["cy"]))
        for i, v in enumerate(c[:8]):
            p.coeffs[i] = v
        p.n_coeffs = len(c)   # (a count the library does not support is the library's to reject)
        self._chk(self.lib.mvo_undistort_configure(self.h, C.byref(p), int(width), int(height)))
        self._undist_hw = (int(height), int(width))

    def undistort(self, image):
        """cv2.undistort(image, K, dist) with the configured K / dist -> ndarray of the same shape and dtype."""
        img, w, h, stride, ch = _image_args(image)
        out = np.zeros_like(img)
        self._chk(self.lib.mvo_undistort(self.h, _p(img), w, h, stride, ch, _p(out), stride))
        return out

    def undistort_dev(self, d_in, d_out, w, h, stride, ch, out_stride):
        """mvo_undistort_dev: device pointers; d_out is the caller's, must not overlap d_in and stays alive until the ctx
        stream has run the call (synchronize())."""
        self._chk(self.lib.mvo_undistort_dev(self.h, C.c_void_p(d_in), int(w), int(h), int(stride), int(ch), C.c_void_p(d_out),
                                             int(out_stride)))

    def debug_undistort_map(self):
        """Map of the last undistort_configure -> (ix, iy int32, ax, ay uint8), each height x width."""
        h, w = getattr(self, "_undist_hw", (0, 0))
        n = h * w
        ix, iy = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        ax, ay = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
        self._chk(self.lib.mvo_debug_get_undistort_map(self.h, _p(ix), _p(iy), _p(ax), _p(ay), n))
        return tuple(a[:n].reshape(h, w) for a in (ix, iy, ax, ay))

    # ---- matching
    def match_knn2(self, q, t):
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        idx = np.zeros((len(q), 2), np.int32)
        dist = np.zeros((len(q), 2), np.int32)
        self._chk(self.lib.mvo_match_knn2(self.h, _p(q), len(q), _p(t), len(t), _p(idx), _p(dist)))
        return idx, dist

    def match_knn2_dev(self, d_q, nq, d_t, nt):
        idx = np.zeros((nq, 2), np.int32)
        dist = np.zeros((nq, 2), np.int32)
        self._chk(self.lib.mvo_match_knn2_dev(self.h, C.c_void_p(d_q), nq, C.c_void_p(d_t), nt, _p(idx), _p(dist)))
        return idx, dist

    def match_radius_l1(self, q, qxy, t, txy, max_px):
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        qxy = np.ascontiguousarray(qxy, np.float32).reshape(-1, 2)
        txy = np.ascontiguousarray(txy, np.float32).reshape(-1, 2)
        idx = np.zeros(len(q), np.int32)
        s = np.zeros(len(q), np.int32)
        self._chk(self.lib.mvo_match_radius_l1(self.h, _p(q), _p(qxy), len(q), _p(t), _p(txy), len(t),
                                               C.c_float(max_px), _p(idx), _p(s)))
        return idx, s

    def match_features(self, d1, d2, method=1, xiang_gao_ratio=2.0, lowe_ratio=1.0, xy1=None, xy2=None, max_px=0.0):
        """geometry::matchFeatures (feature_match.cpp:126-239); ratios as the reference latches them."""
        d1 = np.ascontiguousarray(d1, np.uint8).reshape(-1, 32)
        d2 = np.ascontiguousarray(d2, np.uint8).reshape(-1, 32)
        if xy1 is not None:
            xy1 = np.ascontiguousarray(xy1, np.float32).reshape(-1, 2)
            xy2 = np.ascontiguousarray(xy2, np.float32).reshape(-1, 2)
        out = np.zeros(max(len(d1), 1), DMATCH_DTYPE)
        n = C.c_int()
        r = self.lib.mvo_match_features(self.h, _p(d1), len(d1), _p(d2), len(d2), int(method),
                                        C.c_double(xiang_gao_ratio), C.c_double(lowe_ratio), _p(xy1), _p(xy2),
                                        C.c_float(max_px), _p(out), len(out), C.byref(n))
        if r == MVO_ERR_INVALID and method not in (1, 2, 3):
            # the reference throws std::runtime_error here (feature_match.cpp:225)
            raise RuntimeError("feature_match.cpp::matchFeatures: wrong method index.")
        self._chk(r)
        return out[:n.value].copy()

    def match_features_dev(self, d_d1, n1, d_d2, n2, method=2, xiang_gao_ratio=2.0, lowe_ratio=1.0):
        out = np.zeros(max(n1, 1), DMATCH_DTYPE)
        n = C.c_int()
        self._chk(self.lib.mvo_match_features_dev(self.h, C.c_void_p(d_d1), n1, C.c_void_p(d_d2), n2, int(method),
                                                  C.c_double(xiang_gao_ratio), C.c_double(lowe_ratio), _p(out),
                                                  len(out), C.byref(n)))
        return out[:n.value].copy()

    # ---- pose-guided matching (README.md:212, README.md:272 of the reference: named there, not implemented)
    @staticmethod
    def _epipolar_args(qxy, txy, t_scale, F):
        qxy = np.ascontiguousarray(qxy, np.float32).reshape(-1, 2)
        txy = np.ascontiguousarray(txy, np.float32).reshape(-1, 2)
        if t_scale is not None:
            t_scale = np.ascontiguousarray(t_scale, np.float32).reshape(-1)
            if len(t_scale) != len(txy):
                raise ValueError("t_scale needs one entry per train keypoint")
        return qxy, txy, t_scale, np.ascontiguousarray(F, np.float64).reshape(9)

    def match_knn2_epipolar(self, q, qxy, t, txy, F, max_line_px, t_scale=None):
        """mvo_match_knn2_epipolar: the two nearest trains within t_scale[j] * max_line_px of each query's epipolar line
        (x2^T F x1 = 0, query = frame 1) -> (idx nq x 2, dist nq x 2, n_candidates nq)."""
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        qxy, txy, t_scale, F = self._epipolar_args(qxy, txy, t_scale, F)
        if len(qxy) != len(q) or len(txy) != len(t):
            raise ValueError("one keypoint position per descriptor")
        idx, dist = np.zeros((len(q), 2), np.int32), np.zeros((len(q), 2), np.int32)
        cnt = np.zeros(len(q), np.int32)
        self._chk(self.lib.mvo_match_knn2_epipolar(self.h, _p(q), _p(qxy), len(q), _p(t), _p(txy), _p(t_scale), len(t), _p(F),
                                                   C.c_double(max_line_px), _p(idx), _p(dist), _p(cnt)))
        return idx, dist, cnt

    def match_knn2_epipolar_dev(self, d_q, qxy, d_t, txy, F, max_line_px, t_scale=None):
        """The same with the descriptors in HBM (device pointers); the counts come from qxy / txy."""
        qxy, txy, t_scale, F = self._epipolar_args(qxy, txy, t_scale, F)
        nq, nt = len(qxy), len(txy)
        idx, dist, cnt = np.zeros((nq, 2), np.int32), np.zeros((nq, 2), np.int32), np.zeros(nq, np.int32)
        self._chk(self.lib.mvo_match_knn2_epipolar_dev(self.h, C.c_void_p(d_q), _p(qxy), nq, C.c_void_p(d_t), _p(txy), _p(t_scale),
                                                       nt, _p(F), C.c_double(max_line_px), _p(idx), _p(dist), _p(cnt)))
        return idx, dist, cnt

    def match_features_epipolar(self, d1, xy1, d2, xy2, F, max_line_px, lowe_ratio, max_hamming, scale2=None, cap=None):
        """mvo_match_features_epipolar: the raw call, the ceiling / ratio filter, one query per train -> DMATCH_DTYPE
        sorted by trainIdx."""
        d1 = np.ascontiguousarray(d1, np.uint8).reshape(-1, 32)
        d2 = np.ascontiguousarray(d2, np.uint8).reshape(-1, 32)
        xy1, xy2, scale2, F = self._epipolar_args(xy1, xy2, scale2, F)
        if len(xy1) != len(d1) or len(xy2) != len(d2):
            raise ValueError("one keypoint position per descriptor")
        cap = min(len(d1), len(d2)) if cap is None else int(cap)
        out = np.zeros(max(cap, 1), DMATCH_DTYPE)
        n = C.c_int()
        self._chk(self.lib.mvo_match_features_epipolar(self.h, _p(d1), _p(xy1), len(d1), _p(d2), _p(xy2), _p(scale2), len(d2),
                                                       _p(F), C.c_double(max_line_px), C.c_double(lowe_ratio), int(max_hamming),
                                                       _p(out), cap, C.byref(n)))
        return out[:n.value].copy()

    # ---- tracking by projection (README.md:212 of the reference; the step of vo.cpp:267-289)
    @staticmethod
    def _projection_args(T_w_c, K, txy, t_scale):
        T = np.ascontiguousarray(T_w_c, np.float64).reshape(16)
        txy = np.ascontiguousarray(txy, np.float32).reshape(-1, 2)
        if t_scale is not None:
            t_scale = np.ascontiguousarray(t_scale, np.float32).reshape(-1)
            if len(t_scale) != len(txy):
                raise ValueError("t_scale needs one entry per frame keypoint")
        k = [C.c_double(K[name]) for name in ("fx", "fy", "cx", "cy")]
        return T, k, txy, t_scale

    def _map_size(self, m):
        """Number of points of the resident map (the outputs of the projection calls have one row each)."""
        n = C.c_int()
        self._chk(self.lib.mvo_map_size(self.h, m, C.byref(n)))
        return n.value

    def map_match_knn2_projection(self, m, T_w_c, K, cols, rows, t, txy, max_px, t_scale=None):
        """mvo_map_match_knn2_projection: per map point its pixel under T_w_c and the two nearest frame keypoints within
        t_scale[j] * max_px of it -> (px n_map x 2 f32, idx n_map x 2, dist n_map x 2, n_candidates n_map; -1: not in view)."""
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        T, k, txy, t_scale = self._projection_args(T_w_c, K, txy, t_scale)
        if len(txy) != len(t):
            raise ValueError("one keypoint position per descriptor")
        n = self._map_size(m)
        px, idx, dist = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.int32), np.zeros((n, 2), np.int32)
        cnt = np.zeros(n, np.int32)
        self._chk(self.lib.mvo_map_match_knn2_projection(self.h, m, _p(T), *k, int(cols), int(rows), _p(t), _p(txy), _p(t_scale),
                                                         len(t), C.c_double(max_px), _p(px), _p(idx), _p(dist), _p(cnt)))
        return px, idx, dist, cnt

    def map_match_knn2_projection_dev(self, m, T_w_c, K, cols, rows, d_t, txy, max_px, t_scale=None):
        """The same with the frame's descriptors in HBM (a device pointer); the count comes from txy."""
        T, k, txy, t_scale = self._projection_args(T_w_c, K, txy, t_scale)
        n = self._map_size(m)
        px, idx, dist = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.int32), np.zeros((n, 2), np.int32)
        cnt = np.zeros(n, np.int32)
        self._chk(self.lib.mvo_map_match_knn2_projection_dev(self.h, m, _p(T), *k, int(cols), int(rows), C.c_void_p(d_t), _p(txy),
                                                             _p(t_scale), len(txy), C.c_double(max_px), _p(px), _p(idx), _p(dist),
                                                             _p(cnt)))
        return px, idx, dist, cnt

    def map_match_features_projection(self, m, T_w_c, K, cols, rows, t, txy, max_px, lowe_ratio, max_hamming, t_scale=None,
                                      cap=None):
        """mvo_map_match_features_projection: the raw call, the ceiling / ratio filter, one map point per keypoint ->
        (DMATCH_DTYPE sorted by trainIdx with queryIdx = map index, px n_map x 2, in_view n_map bool)."""
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        T, k, txy, t_scale = self._projection_args(T_w_c, K, txy, t_scale)
        if len(txy) != len(t):
            raise ValueError("one keypoint position per descriptor")
        n = self._map_size(m)
        cap = min(n, len(t)) if cap is None else int(cap)
        out = np.zeros(max(cap, 1), DMATCH_DTYPE)
        px, in_view = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
        cnt = C.c_int()
        self._chk(self.lib.mvo_map_match_features_projection(self.h, m, _p(T), *k, int(cols), int(rows), _p(t), _p(txy), _p(t_scale),
                                                             len(t), C.c_double(max_px), C.c_double(lowe_ratio), int(max_hamming),
                                                             _p(px), _p(in_view), _p(out), cap, C.byref(cnt)))
        return out[:cnt.value].copy(), px, in_view.astype(bool)

    # ---- tracking the local map (ORB-SLAM's Tracking::SearchLocalPoints)
    def map_upload_view(self, m, normal, max_dist):
        """mvo_map_upload_view: the mean normals (n x 3 f32) and largest distances (n f32) of the resident map points."""
        n = self._map_size(m)
        normal = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
        max_dist = np.ascontiguousarray(max_dist, np.float32).reshape(-1)
        if len(normal) != n or len(max_dist) != n:
            raise ValueError("one normal and one max_dist per resident map point")
        self._chk(self.lib.mvo_map_upload_view(self.h, m, _p(normal), _p(max_dist)))

    def _local_args(self, m, T_w_c, K, txy, t_level, skip, level_scale, params):
        if not hasattr(self.lib, "mvo_map_match_knn2_local"):
            raise MvoError(MVO_ERR_STATE, "this libmvo_hip.so has no mvo_map_match_knn2_local")
        T, k, txy, _ = self._projection_args(T_w_c, K, txy, None)
        t_level = np.ascontiguousarray(t_level, np.int32).reshape(-1)
        if len(t_level) != len(txy):
            raise ValueError("one level per frame keypoint")
        n = self._map_size(m)
        if skip is not None:
            skip = np.ascontiguousarray(skip, np.uint8).reshape(-1)
            if len(skip) != n:
                raise ValueError("one skip flag per resident map point")
        ls = np.ascontiguousarray(level_scale, np.float64).reshape(-1)
        pp = None
        if params:
            v = dict(LOCAL_MAP_DEFAULTS, **params)
            pp = C.byref(LocalMapParams(float(v["min_view_cos"]), float(v["radius_near"]), float(v["radius_far"]), float(v["near_cos"]),
                                        float(v["radius_scale"]), float(v["lowe_ratio"]), int(v["max_hamming"]), 0))
        return n, T, k, txy, t_level, skip, ls, pp

    def _local_raw(self, fn, m, T_w_c, K, cols, rows, t, txy, t_level, level_scale, skip, params):
        n, T, k, txy, t_level, skip, ls, pp = self._local_args(m, T_w_c, K, txy, t_level, skip, level_scale, params)
        px, idx, dist = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.int32), np.zeros((n, 2), np.int32)
        cnt, lv, vc = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float64)
        self._chk(fn(self.h, m, _p(T), *k, int(cols), int(rows), t, _p(txy), _p(t_level), len(txy), _p(skip), _p(ls), len(ls), pp,
                     _p(px), _p(idx), _p(dist), _p(cnt), _p(lv), _p(vc)))
        return px, idx, dist, cnt, lv, vc

    def map_match_knn2_local(self, m, T_w_c, K, cols, rows, t, txy, t_level, level_scale, skip=None, params=None):
        """mvo_map_match_knn2_local: per map point that faces the camera within its range under T_w_c, its pixel and the two
        nearest frame keypoints of its predicted level (or the one below) within its radius -> (px n_map x 2 f32, idx n_map x 2,
        dist n_map x 2, n_candidates n_map, level n_map, view_cos n_map f64; n_candidates -1: not active).  t_level: the octave
        per keypoint or -2 (taken); skip: n_map flags or None; params: a dict over LOCAL_MAP_DEFAULTS or None."""
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        if len(t) != len(np.asarray(txy).reshape(-1, 2)):
            raise ValueError("one keypoint position per descriptor")
        return self._local_raw(self.lib.mvo_map_match_knn2_local, m, T_w_c, K, cols, rows, _p(t), txy, t_level, level_scale, skip, params)

    def map_match_knn2_local_dev(self, m, T_w_c, K, cols, rows, d_t, txy, t_level, level_scale, skip=None, params=None):
        """The same with the frame's descriptors in HBM (a device pointer); the count comes from txy."""
        return self._local_raw(self.lib.mvo_map_match_knn2_local_dev, m, T_w_c, K, cols, rows, C.c_void_p(d_t), txy, t_level,
                               level_scale, skip, params)

    def map_match_features_local(self, m, T_w_c, K, cols, rows, t, txy, t_level, level_scale, skip=None, params=None, cap=None):
        """mvo_map_match_features_local: the raw call, ORB-SLAM's acceptance rule, one map point per keypoint ->
        (DMATCH_DTYPE sorted by trainIdx with queryIdx = map index, px n_map x 2, level n_map)."""
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        n, T, k, txy, t_level, skip, ls, pp = self._local_args(m, T_w_c, K, txy, t_level, skip, level_scale, params)
        if len(txy) != len(t):
            raise ValueError("one keypoint position per descriptor")
        cap = min(n, len(t)) if cap is None else int(cap)
        out = np.zeros(max(cap, 1), DMATCH_DTYPE)
        px, lv = np.zeros((n, 2), np.float32), np.zeros(n, np.int32)
        cnt = C.c_int()
        self._chk(self.lib.mvo_map_match_features_local(self.h, m, _p(T), *k, int(cols), int(rows), _p(t), _p(txy), _p(t_level), len(t),
                                                        _p(skip), _p(ls), len(ls), pp, _p(px), _p(lv), _p(out), cap, C.byref(cnt)))
        return out[:cnt.value].copy(), px, lv

    def map_refresh(self, m, obs_desc, obs_cam, obs_start):
        """mvo_map_refresh: every map point takes the medoid of its observations' descriptors (in HBM) and the mean of their
        unit viewing directions -> (choice n int32, -1: no observation; desc n x 32, the resident descriptors after the call;
        norm n x 3 f64).  Observations of point i: rows obs_start[i] .. obs_start[i + 1] - 1."""
        if not hasattr(self.lib, "mvo_map_refresh"):
            raise MvoError(MVO_ERR_STATE, "this libmvo_hip.so has no mvo_map_refresh")
        obs_desc = np.ascontiguousarray(obs_desc, np.uint8).reshape(-1, 32)
        obs_cam = np.ascontiguousarray(obs_cam, np.float64).reshape(-1, 3)
        obs_start = np.ascontiguousarray(obs_start, np.int32).reshape(-1)
        if len(obs_desc) != len(obs_cam):
            raise ValueError("one camera centre per observation descriptor")
        n = self._map_size(m)
        if len(obs_start) != n + 1:
            raise ValueError("obs_start needs one entry per map point and one more")
        choice, desc, norm = np.zeros(n, np.int32), np.zeros((n, 32), np.uint8), np.zeros((n, 3), np.float64)
        self._chk(self.lib.mvo_map_refresh(self.h, m, _p(obs_desc), _p(obs_cam), _p(obs_start), len(obs_desc), _p(choice), _p(desc),
                                           _p(norm)))
        return choice, desc, norm

    def map_refine_positions(self, m, T_w_c, K, obs_frame, obs_uv, obs_start, max_trials=None, min_observations=None,
                             huber_delta=None, rel_tolerance=None):
        """mvo_map_refine_positions: every map point's position re-estimated from all its observations with the poses fixed
        (Huber-weighted Levenberg-Marquardt per point, in HBM) -> (pos n x 3 f32, the resident positions after the call; chi2
        n x 2 f64: before, after; info n x 3 int32: status, accepted steps, trials; outlier n_obs uint8).  Status 0: refined,
        1: too few observations, 2: behind a camera at the start, 3: no trial accepted.  T_w_c: n_frames x 4 x 4; observations
        of point i: rows obs_start[i] .. obs_start[i + 1] - 1 of obs_frame (index into T_w_c) and obs_uv (pixels).  The keyword
        arguments default to the library's (20, 2, sqrt(5.991), 1e-6)."""
        if not hasattr(self.lib, "mvo_map_refine_positions"):
            raise MvoError(MVO_ERR_STATE, "this libmvo_hip.so has no mvo_map_refine_positions")
        T = np.ascontiguousarray(T_w_c, np.float64).reshape(-1, 16)
        obs_frame = np.ascontiguousarray(obs_frame, np.int32).reshape(-1)
        obs_uv = np.ascontiguousarray(obs_uv, np.float32).reshape(-1, 2)
        obs_start = np.ascontiguousarray(obs_start, np.int32).reshape(-1)
        if len(obs_frame) != len(obs_uv):
            raise ValueError("one frame index per observed pixel")
        n = self._map_size(m)
        if len(obs_start) != n + 1:
            raise ValueError("obs_start needs one entry per map point and one more")
        params = None
        if not (max_trials is None and min_observations is None and huber_delta is None and rel_tolerance is None):
            params = MapRefineParams(20 if max_trials is None else int(max_trials), 2 if min_observations is None else int(min_observations),
                                     float(np.sqrt(np.float64(5.991))) if huber_delta is None else float(huber_delta),
                                     1e-6 if rel_tolerance is None else float(rel_tolerance))
            params = C.byref(params)
        pos, chi2, info = np.zeros((n, 3), np.float32), np.zeros((n, 2), np.float64), np.zeros((n, 3), np.int32)
        outlier = np.zeros(len(obs_uv), np.uint8)
        k = [C.c_double(K[name]) for name in ("fx", "fy", "cx", "cy")]
        self._chk(self.lib.mvo_map_refine_positions(self.h, m, _p(T), len(T), *k, _p(obs_frame), _p(obs_uv), _p(obs_start), len(obs_uv),
                                                    params, _p(pos), _p(chi2), _p(info), _p(outlier)))
        return pos, chi2, info, outlier

    # ---- duplicate map points fused over the buffered frames (ORB-SLAM's ORBmatcher::Fuse / MapPoint::Replace)
    @staticmethod
    def _fuse_frames(frames):
        """frames: a sequence of dicts with desc (n x 32), xy (n x 2), conn (n), T (4 x 4, camera to world) and optionally
        scale (n) -> (the mvo_fuse_frame array, the keypoint counts, the arrays it points into)."""
        arr, counts, keep = (FuseFrame * max(len(frames), 1))(), [], []
        for f, fr in enumerate(frames):
            desc = np.ascontiguousarray(fr["desc"], np.uint8).reshape(-1, 32)
            xy = np.ascontiguousarray(fr["xy"], np.float32).reshape(-1, 2)
            conn = np.ascontiguousarray(fr["conn"], np.int32).reshape(-1)
            scale = fr.get("scale")
            if scale is not None:
                scale = np.ascontiguousarray(scale, np.float32).reshape(-1)
            if len(xy) != len(desc) or len(conn) != len(desc) or (scale is not None and len(scale) != len(desc)):
                raise ValueError("frame %d: one position, one connection (and one scale) per descriptor" % f)
            keep.append((desc, xy, conn, scale))
            arr[f].desc, arr[f].xy, arr[f].conn = desc.ctypes.data, xy.ctypes.data, conn.ctypes.data
            arr[f].scale = None if scale is None else scale.ctypes.data
            arr[f].n = len(desc)
            arr[f].T_w_c[:] = [float(x) for x in np.asarray(fr["T"], np.float64).reshape(16)]
            counts.append(len(desc))
        return arr, counts, keep

    def map_fuse_search(self, m, frames, K, cols, rows, max_px):
        """mvo_map_fuse_search: every map point against every keypoint of every frame in one launch -> (idx F x n_map x 2,
        dist F x n_map x 2, n_candidates F x n_map, px F x n_map x 2 f32), per frame the rows of map_match_knn2_projection; a
        point not in view of the frame or already connected in it: idx -1, dist INT32_MAX, n_candidates -1, px (0, 0)."""
        if not hasattr(self.lib, "mvo_map_fuse_search"):
            raise MvoError(MVO_ERR_STATE, "this libmvo_hip.so has no mvo_map_fuse_search")
        arr, _, keep = self._fuse_frames(frames)
        n, F = self._map_size(m), len(frames)
        idx, dist = np.zeros((F, n, 2), np.int32), np.zeros((F, n, 2), np.int32)
        cnt, px = np.zeros((F, n), np.int32), np.zeros((F, n, 2), np.float32)
        k = [C.c_double(K[name]) for name in ("fx", "fy", "cx", "cy")]
        self._chk(self.lib.mvo_map_fuse_search(self.h, m, arr, F, *k, int(cols), int(rows), C.c_double(max_px), _p(idx), _p(dist),
                                               _p(cnt), _p(px)))
        del keep
        return idx, dist, cnt, px

    def map_fuse(self, m, frames, K, cols, rows, max_px=None, max_hamming=None, cap_added=None):
        """mvo_map_fuse: the search, then one claimant per keypoint, the merges and the additions -> (replaced_by n_map int32:
        the row that stands for each point from now on; added, FUSE_OBSERVATION_DTYPE: the observations gained, `point` a
        surviving row; counts 6 int32: candidates, merges accepted, merges refused, observations added, observations refused,
        points replaced).  The resident map is not changed.  max_px / max_hamming default to the library's (3.0, 50)."""
        if not hasattr(self.lib, "mvo_map_fuse"):
            raise MvoError(MVO_ERR_STATE, "this libmvo_hip.so has no mvo_map_fuse")
        arr, counts_kp, keep = self._fuse_frames(frames)
        n, F = self._map_size(m), len(frames)
        params = None
        if not (max_px is None and max_hamming is None):
            params = C.byref(MapFuseParams(3.0 if max_px is None else float(max_px), 50 if max_hamming is None else int(max_hamming)))
        cap = sum(counts_kp) if cap_added is None else int(cap_added)
        replaced_by, added = np.zeros(n, np.int32), np.zeros(max(cap, 1), FUSE_OBSERVATION_DTYPE)
        n_added, counts = C.c_int(), np.zeros(6, np.int32)
        k = [C.c_double(K[name]) for name in ("fx", "fy", "cx", "cy")]
        self._chk(self.lib.mvo_map_fuse(self.h, m, arr, F, *k, int(cols), int(rows), params, _p(replaced_by), _p(added), cap,
                                        C.byref(n_added), _p(counts)))
        del keep
        return replaced_by, added[:n_added.value].copy(), counts

    # ---- new map points triangulated against every buffered frame (ORB-SLAM's LocalMapping::CreateNewMapPoints)
    def window_triangulate_search(self, curr, frames, K, max_line_px=2.0, min_baseline=0.0):
        """mvo_window_triangulate_search: every free keypoint of curr against every free keypoint of every frame along its epipolar
        line, in one launch -> (idx F x n x 2, dist F x n x 2, n_candidates F x n), per frame the rows of match_knn2_epipolar; a
        keypoint that is not free, or a frame that fails the baseline test: idx -1, dist INT32_MAX, n_candidates -1.  curr and
        the frames are dicts as map_fuse takes them; only conn == -1 matters."""
        if not hasattr(self.lib, "mvo_window_triangulate_search"):
            raise MvoError(MVO_ERR_STATE, "this libmvo_hip.so has no mvo_window_triangulate_search")
        carr, (n,), ckeep = self._fuse_frames([curr])
        arr, _, keep = self._fuse_frames(frames)
        F = len(frames)
        idx, dist, cnt = np.zeros((F, n, 2), np.int32), np.zeros((F, n, 2), np.int32), np.zeros((F, n), np.int32)
        k = [C.c_double(K[name]) for name in ("fx", "fy", "cx", "cy")]
        self._chk(self.lib.mvo_window_triangulate_search(self.h, carr, arr, F, *k, C.c_double(max_line_px), C.c_double(min_baseline),
                                                         _p(idx), _p(dist), _p(cnt)))
        del keep, ckeep
        return idx, dist, cnt

    def window_triangulate(self, curr, frames, K, cap_points=None, cap_pairs=None, **params):
        """mvo_window_triangulate: the search, the filter, the verification of every pair, the choice -> (points,
        WINDOW_POINT_DTYPE, sorted by keypoint: one new point per keypoint of curr that has an accepted pair, in the camera of
        curr; pairs, WINDOW_PAIR_DTYPE, ordered by (frame, train): every pair after the filter with its status; counts 12 int32:
        free keypoints, active frames, rows with a neighbour, pairs, pairs failing each of the six bits, accepted pairs, new
        points).  params: the fields of mvo_window_triangulate_params; none given passes NULL (the library's defaults)."""
        if not hasattr(self.lib, "mvo_window_triangulate"):
            raise MvoError(MVO_ERR_STATE, "this libmvo_hip.so has no mvo_window_triangulate")
        unknown = set(params) - set(WINDOW_TRIANGULATE_DEFAULTS)
        if unknown:
            raise TypeError("window_triangulate: unknown parameters %r" % sorted(unknown))
        carr, (n,), ckeep = self._fuse_frames([curr])
        arr, counts_kp, keep = self._fuse_frames(frames)
        P = None
        if params:
            d = dict(WINDOW_TRIANGULATE_DEFAULTS, **params)
            P = C.byref(WindowTriangulateParams(float(d["max_line_px"]), float(d["lowe_ratio"]), int(d["max_hamming"]),
                                                float(d["max_cos_parallax"]), float(d["max_reproj_chi2"]), float(d["ratio_factor"]),
                                                float(d["min_baseline"])))
        capp = n if cap_points is None else int(cap_points)
        capq = sum(counts_kp) if cap_pairs is None else int(cap_pairs)
        points, pairs = np.zeros(max(capp, 1), WINDOW_POINT_DTYPE), np.zeros(max(capq, 1), WINDOW_PAIR_DTYPE)
        n_points, n_pairs, counts = C.c_int(), C.c_int(), np.zeros(12, np.int32)
        k = [C.c_double(K[name]) for name in ("fx", "fy", "cx", "cy")]
        self._chk(self.lib.mvo_window_triangulate(self.h, carr, arr, len(frames), *k, P, _p(points), capp, C.byref(n_points), _p(pairs),
                                                  capq, C.byref(n_pairs), _p(counts)))
        del keep, ckeep
        return points[:n_points.value].copy(), pairs[:n_pairs.value].copy(), counts

    def map_debug_get(self, m):
        """mvo_debug_get_map: the resident arrays -> (pos n x 3 f32, desc n x 32)."""
        n = self._map_size(m)
        pos, desc = np.zeros((n, 3), np.float32), np.zeros((n, 32), np.uint8)
        cnt = C.c_int()
        self._chk(self.lib.mvo_debug_get_map(self.h, m, _p(pos), _p(desc), n, C.byref(cnt)))
        assert cnt.value == n
        return pos, desc

    def optimize_pose(self, pts3d, pts2d, T_w_c_init, K, inv_sigma2=None, rounds=None, iterations=None, min_inliers=None,
                      chi2_threshold=None, huber_delta=None, rel_tolerance=None):
        """mvo_optimize_pose: the pose from a robust motion-only Levenberg-Marquardt over all matches, from the predicted pose
        T_w_c_init (ORB-SLAM's PoseOptimization; one launch) -> (T_w_c 4 x 4, T_c_w 4 x 4, outlier n uint8, chi2 2 f64: start of
        round 0, end of the last round; info 6 int32: status, rounds run, trials, accepted steps, inliers, observations in front
        at the start).  Status 0: optimised, 1: the inliers fell below min_inliers, 2: too few observations in front at the
        start, 3: no trial accepted.  pts3d: n x 3 world, pts2d: n x 2 pixels, inv_sigma2: n weights or None.  The keyword
        arguments default to the library's (4, 10, 10, 5.991, sqrt(5.991), 1e-6)."""
        if not hasattr(self.lib, "mvo_optimize_pose"):
            raise MvoError(MVO_ERR_STATE, "this libmvo_hip.so has no mvo_optimize_pose")
        p3 = np.ascontiguousarray(pts3d, np.float32).reshape(-1, 3)
        p2 = np.ascontiguousarray(pts2d, np.float32).reshape(-1, 2)
        if len(p3) != len(p2):
            raise ValueError("one pixel per point")
        sg = None if inv_sigma2 is None else np.ascontiguousarray(inv_sigma2, np.float32).reshape(-1)
        if sg is not None and len(sg) != len(p3):
            raise ValueError("one weight per observation")
        T0 = np.ascontiguousarray(T_w_c_init, np.float64).reshape(16)
        given = (rounds, iterations, min_inliers, chi2_threshold, huber_delta, rel_tolerance)
        params = None
        if any(v is not None for v in given):
            dflt = (4, 10, 10, 5.991, float(np.sqrt(np.float64(5.991))), 1e-6)
            v = [d if g is None else g for g, d in zip(given, dflt)]
            params = PoseOptimizeParams(int(v[0]), int(v[1]), int(v[2]), float(v[3]), float(v[4]), float(v[5]))
            params = C.byref(params)
        n = len(p3)
        Twc, Tcw, outlier = np.zeros((4, 4), np.float64), np.zeros((4, 4), np.float64), np.zeros(n, np.uint8)
        chi2, info = np.zeros(2, np.float64), np.zeros(6, np.int32)
        k = [C.c_double(K[name]) for name in ("fx", "fy", "cx", "cy")]
        self._chk(self.lib.mvo_optimize_pose(self.h, _p(p3), _p(p2), None if sg is None else _p(sg), n, _p(T0), *k, params, _p(Twc),
                                             _p(Tcw), _p(outlier), _p(chi2), _p(info)))
        return Twc, Tcw, outlier, chi2, info

    def pose_optimize_debug_get(self):
        """mvo_debug_get_pose_optimize: one row per round of the last mvo_optimize_pose that launched -> rounds x 6 f64 (inliers
        going in, chi2 at the start, chi2 at the end, trials, accepted steps, inliers coming out)."""
        rows, cnt = np.zeros((8, 6), np.float64), C.c_int()
        self._chk(self.lib.mvo_debug_get_pose_optimize(self.h, _p(rows), 8, C.byref(cnt)))
        return rows[:cnt.value].copy()

    # ---- bundle adjustment
    def _ba_problem(self, poses, points, edge_pose, edge_point, edge_uv, focal, cx, cy, info, huber_delta,
                    fix_points, pose_fixed, max_iterations):
        keep = dict(poses=np.ascontiguousarray(poses, np.float64).reshape(-1, 16).copy(),
                    points=np.ascontiguousarray(points, np.float64).reshape(-1, 3).copy(),
                    ep=np.ascontiguousarray(edge_pose, np.int32), el=np.ascontiguousarray(edge_point, np.int32),
                    uv=np.ascontiguousarray(edge_uv, np.float64).reshape(-1, 2),
                    pf=None if pose_fixed is None else np.ascontiguousarray(pose_fixed, np.uint8))
        pr = BaProblem()
        pr.n_poses, pr.n_points, pr.n_edges = len(keep["poses"]), len(keep["points"]), len(keep["ep"])
        pr.pose_T_w_c, pr.points = keep["poses"].ctypes.data, keep["points"].ctypes.data
        pr.edge_pose, pr.edge_point, pr.edge_uv = keep["ep"].ctypes.data, keep["el"].ctypes.data, keep["uv"].ctypes.data
        pr.focal, pr.cx, pr.cy = focal, cx, cy
        pr.info = (C.c_double * 4)(*np.asarray(info, np.float64).ravel())
        pr.huber_delta = huber_delta
        pr.fix_points = int(bool(fix_points))
        pr.pose_fixed = None if keep["pf"] is None else keep["pf"].ctypes.data
        pr.max_iterations = int(max_iterations)
        return pr, keep

    def ba_prepare(self, poses, points, edge_pose, edge_point, edge_uv, focal, cx, cy, info=(1, 0, 0, 1),
                   huber_delta=1.0, fix_points=False, pose_fixed=None, max_iterations=50):
        """Uploads a window once; returns an opaque handle for ba_solve_resident / ba_fetch / ba_release."""
        pr, keep = self._ba_problem(poses, points, edge_pose, edge_point, edge_uv, focal, cx, cy, info, huber_delta,
                                    fix_points, pose_fixed, max_iterations)
        h = C.c_void_p()
        self._chk(self.lib.mvo_ba_prepare(self.h, C.byref(pr), C.byref(h)))
        return (h, pr.n_poses, pr.n_points)

    def ba_solve_resident(self, handle):
        self._chk(self.lib.mvo_ba_solve_resident(self.h, handle[0]))

    def ba_fetch(self, handle, want_points=True):
        h, F, L = handle
        poses = np.zeros((F, 16))
        points = np.zeros((L, 3)) if want_points else None
        st = BaStats()
        self._chk(self.lib.mvo_ba_fetch(self.h, h, _p(poses), _p(points), C.byref(st)))
        return poses.reshape(-1, 4, 4), points, {k: getattr(st, k) for k, _ in BaStats._fields_}

    def ba_release(self, handle):
        self.lib.mvo_ba_release.restype = None
        self.lib.mvo_ba_release(self.h, handle[0])

    def bundle_adjustment(self, poses, points, edge_pose, edge_point, edge_uv, focal, cx, cy, info=(1, 0, 0, 1),
                          huber_delta=1.0, fix_points=False, pose_fixed=None, max_iterations=50):
        """optimization::bundleAdjustment on flattened arrays.  Returns (poses [F,4,4], points [L,3], stats)."""
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 16).copy()
        points = np.ascontiguousarray(points, np.float64).reshape(-1, 3).copy()
        ep = np.ascontiguousarray(edge_pose, np.int32)
        el = np.ascontiguousarray(edge_point, np.int32)
        uv = np.ascontiguousarray(edge_uv, np.float64).reshape(-1, 2)
        pf = None if pose_fixed is None else np.ascontiguousarray(pose_fixed, np.uint8)
        pr = BaProblem()
        pr.n_poses, pr.n_points, pr.n_edges = len(poses), len(points), len(ep)
        pr.pose_T_w_c, pr.points = poses.ctypes.data, points.ctypes.data
        pr.edge_pose, pr.edge_point, pr.edge_uv = ep.ctypes.data, el.ctypes.data, uv.ctypes.data
        pr.focal, pr.cx, pr.cy = focal, cx, cy
        pr.info = (C.c_double * 4)(*np.asarray(info, np.float64).ravel())
        pr.huber_delta = huber_delta
        pr.fix_points = int(bool(fix_points))
        pr.pose_fixed = None if pf is None else pf.ctypes.data
        pr.max_iterations = int(max_iterations)
        st = BaStats()
        self._chk(self.lib.mvo_bundle_adjustment(self.h, C.byref(pr), C.byref(st)))
        return poses.reshape(-1, 4, 4), points, {k: getattr(st, k) for k, _ in BaStats._fields_}

    def ba_solve_batch(self, problems, **kw):
        """mvo_ba_solve_batch: `problems` = list of argument tuples of bundle_adjustment(); the windows are solved in one
        grid (8 per launch).  Returns a list of (poses, points, stats)."""
        prs = (BaProblem * len(problems))()
        keeps = []
        for i, a in enumerate(problems):
            d = dict(info=(1, 0, 0, 1), huber_delta=1.0, fix_points=False, pose_fixed=None, max_iterations=50)
            d.update(kw)
            pr, keep = self._ba_problem(*a, d["info"], d["huber_delta"], d["fix_points"], d["pose_fixed"], d["max_iterations"])
            prs[i] = pr
            keeps.append(keep)
        sts = (BaStats * len(problems))()
        self._chk(self.lib.mvo_ba_solve_batch(self.h, prs, len(problems), sts))
        return [(k["poses"].reshape(-1, 4, 4), k["points"], {f: getattr(sts[i], f) for f, _ in BaStats._fields_})
                for i, k in enumerate(keeps)]

    def ba_set_mode(self, mode):
        """mvo_ba_set_mode: "latency" (default, ~300 observations per workgroup), "throughput" (~670, resident grid under load) or
        "shared" (the throughput cut on the launch path only)."""
        self._chk(self.lib.mvo_ba_set_mode(self.h, {"latency": 0, "throughput": 1, "shared": 2}[mode]))

    def ba_trace_enable(self, on=True):
        self._chk(self.lib.mvo_debug_ba_trace_enable(self.h, int(on)))

    def ba_trace(self, handle=None, raw_rows=0):
        """LM trace of the last solve: rows {lambda, chi2, rho, accepted} per trial (raw_rows > 0: that many raw rows)."""
        out = np.zeros((512, 4))
        n = C.c_int()
        self._chk(self.lib.mvo_debug_get_ba_trace(self.h, handle[0] if handle else None, _p(out),
                                                  -int(raw_rows) if raw_rows else 512, C.byref(n)))
        return out[:n.value].copy()

    def ba_plan(self, handle=None):
        """Summation plan of the last window: dict(wgs, nsplit, groups, wg_pt_start)."""
        g, ns = C.c_int(), C.c_int()
        pt = np.zeros(257, np.int32)
        self._chk(self.lib.mvo_debug_get_ba_plan(self.h, handle[0] if handle else None, C.byref(g), C.byref(ns), _p(pt), 257))
        return dict(wgs=g.value, nsplit=ns.value & 0xffff, groups=max(1, ns.value >> 16), wg_pt_start=pt[:g.value + 1].copy())

    # ---- tracking rows (vo.cpp:16-49, 270-357)
    def map_create(self):
        m = C.c_void_p()
        self._chk(self.lib.mvo_map_create(self.h, C.byref(m)))
        return m

    def map_release(self, m):
        self.lib.mvo_map_release.restype = None
        self.lib.mvo_map_release(self.h, m)

    def map_upload(self, m, pos, desc):
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        assert len(pos) == len(desc)
        self._chk(self.lib.mvo_map_upload(self.h, m, _p(pos), _p(desc), len(pos)))

    def map_update_positions(self, m, pos, first=0):
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        self._chk(self.lib.mvo_map_update_positions(self.h, m, _p(pos), int(first), len(pos)))

    def map_points_in_view(self, m, T_w_c, K, cols, rows, cap):
        """-> (idx [n] int32, px [n,2] float32, device pointer of the gathered n x 32 descriptors)."""
        T = np.ascontiguousarray(T_w_c, np.float64).reshape(4, 4)
        idx = np.zeros(max(cap, 1), np.int32)
        px = np.zeros((max(cap, 1), 2), np.float32)
        n = C.c_int()
        d = C.c_void_p()
        self._chk(self.lib.mvo_map_points_in_view(self.h, m, _p(T), C.c_double(K["fx"]), C.c_double(K["fy"]),
                                                  C.c_double(K["cx"]), C.c_double(K["cy"]), int(cols), int(rows),
                                                  _p(idx), _p(px), int(cap), C.byref(n), C.byref(d)))
        return idx[:n.value].copy(), px[:n.value].copy(), d.value

    def solve_pnp_ransac(self, pts3d, pts2d, K, iterations=100, reprojection_error=2.0, confidence=0.999):
        """cv::solvePnPRansac as vo.cpp:326-329 calls it -> dict(ok, rvec, tvec, inliers)."""
        p3 = np.ascontiguousarray(pts3d, np.float32).reshape(-1, 3)
        p2 = np.ascontiguousarray(pts2d, np.float32).reshape(-1, 2)
        assert len(p3) == len(p2)
        n = len(p3)
        rvec, tvec = np.zeros(3), np.zeros(3)
        inl = np.zeros(max(n, 1), np.int32)
        n_inl, found = C.c_int(), C.c_int()
        self._chk(self.lib.mvo_solve_pnp_ransac(self.h, _p(p3), _p(p2), n, C.c_double(K["fx"]), C.c_double(K["fy"]),
                                                C.c_double(K["cx"]), C.c_double(K["cy"]), int(iterations),
                                                C.c_float(reprojection_error), C.c_double(confidence), _p(rvec),
                                                _p(tvec), _p(inl), len(inl), C.byref(n_inl), C.byref(found)))
        return dict(ok=bool(found.value), rvec=rvec, tvec=tvec, inliers=inl[:n_inl.value].copy())

    def triangulate_points(self, kp_prev, kp_curr, K, R, t):
        """geometry::helperTriangulatePoints -> (points in the previous camera frame, returned points), n x 3 f32."""
        a = np.ascontiguousarray(kp_prev, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(kp_curr, np.float32).reshape(-1, 2)
        assert len(a) == len(b)
        R = np.ascontiguousarray(R, np.float64).reshape(3, 3)
        t = np.ascontiguousarray(t, np.float64).reshape(3)
        n = len(a)
        pp, pc = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        self._chk(self.lib.mvo_triangulate_points(self.h, _p(a), _p(b), n, C.c_double(K["fx"]), C.c_double(K["fy"]),
                                                  C.c_double(K["cx"]), C.c_double(K["cy"]), _p(R), _p(t), _p(pp), _p(pc)))
        return pp, pc

    def find_essential_inliers(self, kp_prev, kp_curr, K, prob=0.999, threshold=1.0):
        """geometry::helperFindInlierMatchesByEpipolarCons -> ascending inlier indices into the matches."""
        a = np.ascontiguousarray(kp_prev, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(kp_curr, np.float32).reshape(-1, 2)
        assert len(a) == len(b)
        n = len(a)
        inl = np.zeros(max(n, 1), np.int32)
        cnt = C.c_int()
        self._chk(self.lib.mvo_find_essential_inliers(self.h, _p(a), _p(b), n, C.c_double(K["fx"]), C.c_double(K["fy"]),
                                                      C.c_double(K["cx"]), C.c_double(K["cy"]), C.c_double(prob),
                                                      C.c_double(threshold), _p(inl), len(inl), C.byref(cnt)))
        return inl[:cnt.value].copy()

    def debug_essential(self):
        counts = np.zeros((1000, 10), np.int32)
        info = np.zeros(5, np.int32)
        it = self.lib.mvo_debug_get_essential(self.h, _p(counts), 1000, _p(info))
        if it < 0:
            self._chk(it)
        return dict(counts=counts[:it].copy(), best_iter=int(info[0]), best_model=int(info[1]), iters_run=int(info[2]),
                    evaluated=int(info[3]))

    def find_homography(self, src, dst, threshold=3.0, confidence=0.995):
        """cv::findHomography(src, dst, RANSAC, threshold) of estiMotionByHomography -> dict(H (3 x 3, or None when
        findHomography returns an empty matrix), inliers (ascending indices of the RANSAC mask))."""
        a = np.ascontiguousarray(src, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(dst, np.float32).reshape(-1, 2)
        assert len(a) == len(b)
        n = len(a)
        H = np.zeros(9)
        inl = np.zeros(max(n, 1), np.int32)
        cnt, found = C.c_int(), C.c_int()
        self._chk(self.lib.mvo_find_homography(self.h, _p(a), _p(b), n, C.c_double(threshold), C.c_double(confidence),
                                               _p(H), _p(inl), len(inl), C.byref(cnt), C.byref(found)))
        return dict(H=H.reshape(3, 3) if found.value else None, inliers=inl[:cnt.value].copy())

    def esti_motion_by_essential(self, kp1, kp2, K, prob=0.999, threshold=1.0):
        """estiMotionByEssential -> dict(found, E (scaled by 1 / E(2,2)), R, t (unit), inliers (ascending indices of
        the RANSAC mask)); E, R, t are None when found is False."""
        a = np.ascontiguousarray(kp1, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(kp2, np.float32).reshape(-1, 2)
        assert len(a) == len(b)
        n = len(a)
        E, R, t = np.zeros(9), np.zeros(9), np.zeros(3)
        inl = np.zeros(max(n, 1), np.int32)
        cnt, found = C.c_int(), C.c_int()
        self._chk(self.lib.mvo_esti_motion_by_essential(
            self.h, _p(a), _p(b), n, C.c_double(K["fx"]), C.c_double(K["fy"]), C.c_double(K["cx"]), C.c_double(K["cy"]),
            C.c_double(prob), C.c_double(threshold), _p(E), _p(R), _p(t), _p(inl), len(inl), C.byref(cnt), C.byref(found)))
        ok = bool(found.value)
        return dict(found=ok, E=E.reshape(3, 3) if ok else None, R=R.reshape(3, 3) if ok else None, t=t if ok else None,
                    inliers=inl[:cnt.value].copy())

    def debug_recover_pose(self, cap=1 << 16):
        """Record of the last esti_motion_by_essential: dict(good (4 counts), chosen (0..3, -1: none), R1, R2, t of the
        decomposition, masks (bit k: the match passes combination k))."""
        good = np.zeros(4, np.int32)
        chosen = C.c_int32()
        d = np.zeros(21)
        masks = np.zeros(cap, np.uint8)
        n = self.lib.mvo_debug_get_recover_pose(self.h, _p(good), C.byref(chosen), _p(d), _p(masks), cap)
        if n < 0:
            self._chk(n)
        return dict(good=good, chosen=int(chosen.value), R1=d[:9].reshape(3, 3), R2=d[9:18].reshape(3, 3), t=d[18:].copy(),
                    masks=masks[:n].copy())

    def check_init_scores(self, kp1, kp2, K, E, inl_e, H, inl_h, sigma=1.0):
        """checkEssentialScore + checkHomographyScore -> dict(score_e, score_h, kept_e, kept_h).  E / H may be None."""
        a = np.ascontiguousarray(kp1, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(kp2, np.float32).reshape(-1, 2)
        assert len(a) == len(b)
        Ed = None if E is None else np.ascontiguousarray(E, np.float64).reshape(9)
        Hd = None if H is None else np.ascontiguousarray(H, np.float64).reshape(9)
        le = np.ascontiguousarray(inl_e if inl_e is not None else [], np.int32).reshape(-1)
        lh = np.ascontiguousarray(inl_h if inl_h is not None else [], np.int32).reshape(-1)
        ke, kh = np.zeros(max(len(le), 1), np.int32), np.zeros(max(len(lh), 1), np.int32)
        se, sh = C.c_double(), C.c_double()
        ne, nh = C.c_int(), C.c_int()
        self._chk(self.lib.mvo_check_init_scores(
            self.h, _p(a), _p(b), len(a), C.c_double(K["fx"]), C.c_double(K["fy"]), C.c_double(K["cx"]),
            C.c_double(K["cy"]), _p(Ed), _p(le), len(le), _p(Hd), _p(lh), len(lh), C.c_double(sigma), C.byref(se),
            C.byref(sh), _p(ke), C.byref(ne), _p(kh), C.byref(nh)))
        return dict(score_e=se.value, score_h=sh.value, kept_e=ke[:ne.value].copy(), kept_h=kh[:nh.value].copy())

    def esti_motion_by_homography(self, kp1, kp2, K, threshold=3.0, confidence=0.995):
        """estiMotionByHomography + removeWrongRtOfHomography -> dict(found, H (scaled by 1 / H(2,2)), inliers
        (ascending indices of the RANSAC mask), Rs, ts (unit), normals: lists of the surviving candidates)."""
        a = np.ascontiguousarray(kp1, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(kp2, np.float32).reshape(-1, 2)
        assert len(a) == len(b)
        n = len(a)
        H, Rs, ts, ns = np.zeros(9), np.zeros(36), np.zeros(12), np.zeros(12)
        inl = np.zeros(max(n, 1), np.int32)
        cnt, k, found = C.c_int(), C.c_int(), C.c_int()
        self._chk(self.lib.mvo_esti_motion_by_homography(
            self.h, _p(a), _p(b), n, C.c_double(K["fx"]), C.c_double(K["fy"]), C.c_double(K["cx"]), C.c_double(K["cy"]),
            C.c_double(threshold), C.c_double(confidence), _p(H), _p(inl), len(inl), C.byref(cnt), _p(Rs), _p(ts),
            _p(ns), C.byref(k), C.byref(found)))
        ok = bool(found.value)
        m = k.value
        return dict(found=ok, H=H.reshape(3, 3) if ok else None, inliers=inl[:cnt.value].copy(),
                    Rs=[Rs[9 * j:9 * j + 9].reshape(3, 3).copy() for j in range(m)], ts=[ts[3 * j:3 * j + 3].copy() for j in range(m)],
                    normals=[ns[3 * j:3 * j + 3].copy() for j in range(m)])

    def debug_homography_decomposition(self):
        """Record of the last homography decomposition: dict(count (0: no H, 1: rotation-only, 4), rotation_only,
        index (of the largest |S_ii|, -1 for rotation-only), Hn, w, Rs (4 x 3 x 3), ts (4 x 3, before t / |t|), normals
        (4 x 3), rejected (H inliers rejecting each candidate))."""
        Hn, w, Rs, ts, ns = np.zeros(9), np.zeros(3), np.zeros(36), np.zeros(12), np.zeros(12)
        br, rej = np.zeros(2, np.int32), np.zeros(4, np.int32)
        cnt = self.lib.mvo_debug_get_homography_decomposition(self.h, _p(Hn), _p(w), _p(br), _p(Rs), _p(ts), _p(ns), _p(rej))
        if cnt < 0:
            self._chk(cnt)
        return dict(count=cnt, rotation_only=bool(br[0]), index=int(br[1]), Hn=Hn.reshape(3, 3), w=w,
                    Rs=Rs.reshape(4, 3, 3), ts=ts.reshape(4, 3), normals=ns.reshape(4, 3), rejected=rej)

    def estimate_possible_relative_poses(self, kp1, kp2, K, prob=0.999, threshold=1.0, h_threshold=3.0,
                                         h_confidence=0.995, sigma=1.0, motion_cam2_to_cam1=True):
        """helperEstimatePossibleRelativePosesByEpipolarGeometry (is_calc_homo = true) -> dict(best (-1: the rule picked
        a slot that does not exist), ratio, score_e, score_h, E, H (None when absent), inliers_e, inliers_h,
        solutions=[dict(kind "E" / "H", R, t, normal (None for E), inliers, pts3d (in camera 1), candidate (H: index in
        the decomposition))]).  solutions[0] is the E slot, None when E has no model; best indexes solutions."""
        a = np.ascontiguousarray(kp1, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(kp2, np.float32).reshape(-1, 2)
        assert len(a) == len(b)
        n = len(a)
        ie, ih = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        pts = np.zeros((max(5 * n, 1), 3), np.float32)
        o = InitPoses()
        o.inliers_e, o.inliers_h, o.cap_inliers = _p(ie), _p(ih), len(ie)
        o.pts3d, o.cap_pts = _p(pts), len(pts)
        self._chk(self.lib.mvo_estimate_possible_relative_poses(
            self.h, _p(a), _p(b), n, C.c_double(K["fx"]), C.c_double(K["fy"]), C.c_double(K["cx"]), C.c_double(K["cy"]),
            C.c_double(prob), C.c_double(threshold), C.c_double(h_threshold), C.c_double(h_confidence),
            C.c_double(sigma), int(bool(motion_cam2_to_cam1)), C.byref(o)))
        return self._poses_dict(o, ie, ih, pts)

    @staticmethod
    def _poses_dict(o, ie, ih, pts):
        ine, inh = ie[:o.n_inliers_e].copy(), ih[:o.n_inliers_h].copy()
        sols = []
        for s in range(o.n_slots):
            if not o.present[s]:
                sols.append(None)
                continue
            off, m = o.pts_offset[s], o.pts_count[s]
            sols.append(dict(kind="E" if s == 0 else "H", R=np.array(o.R[9 * s:9 * s + 9]).reshape(3, 3),
                             t=np.array(o.t[3 * s:3 * s + 3]),
                             normal=None if s == 0 else np.array(o.normal[3 * s:3 * s + 3]), inliers=ine if s == 0 else inh,
                             pts3d=pts[off:off + m].copy(), candidate=-1 if s == 0 else int(o.h_candidate[s])))
        return dict(best=int(o.best), ratio=o.ratio, score_e=o.score_e, score_h=o.score_h,
                    E=np.array(o.E).reshape(3, 3) if o.found_e else None, H=np.array(o.H).reshape(3, 3) if o.found_h else None,
                    inliers_e=ine, inliers_h=inh, solutions=sols)

    def init_two_view(self, kp1, kp2, K, T_w_c_ref=None, prob=0.999, threshold=1.0, h_threshold=3.0, h_confidence=0.995,
                      sigma=1.0, min_triang_angle=1.0, max_ratio_to_median=20.0, assumed_mean_depth=0.8,
                      min_inlier_matches=15, min_pixel_dist=50.0, min_median_triangulation_angle=2.0):
        """VisualOdometry::estimateMotionAnd3DPoints_ + isVoGoodToInit_ (vo.cpp:53-170; defaults of config.yaml:101-113)
        -> dict(poses (what estimate_possible_relative_poses returns), slot, n_slot_inliers, n_kept, scaled,
        matches_for_3d (indices into the matches), pts3d_in_curr, angles, R, t, T_w_c, mean_depth, scale,
        mean_pixel_dist, mean_angle, median_angle, min_angle, max_angle, criteria (3 bools), good).  T_w_c_ref: the
        pose of the first keyframe (identity by default)."""
        a = np.ascontiguousarray(kp1, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(kp2, np.float32).reshape(-1, 2)
        assert len(a) == len(b)
        n = len(a)
        Tr = np.ascontiguousarray(np.eye(4) if T_w_c_ref is None else T_w_c_ref, np.float64).reshape(4, 4)
        ie, ih = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        pts = np.zeros((max(5 * n, 1), 3), np.float32)
        o = InitPoses()
        o.inliers_e, o.inliers_h, o.cap_inliers = _p(ie), _p(ih), len(ie)
        o.pts3d, o.cap_pts = _p(pts), len(pts)
        m3d, p3d, ang = np.zeros(max(n, 1), np.int32), np.zeros((max(n, 1), 3), np.float32), np.zeros(max(n, 1))
        res = InitResult()
        res.matches_for_3d, res.pts3d_in_curr, res.angles, res.cap = _p(m3d), _p(p3d), _p(ang), len(m3d)
        prm = InitParams(min_triang_angle, max_ratio_to_median, assumed_mean_depth, int(min_inlier_matches),
                         min_pixel_dist, min_median_triangulation_angle)
        self._chk(self.lib.mvo_init_two_view(
            self.h, _p(a), _p(b), n, C.c_double(K["fx"]), C.c_double(K["fy"]), C.c_double(K["cx"]), C.c_double(K["cy"]),
            C.c_double(prob), C.c_double(threshold), C.c_double(h_threshold), C.c_double(h_confidence),
            C.c_double(sigma), _p(Tr), C.byref(prm), C.byref(o), C.byref(res)))
        k = res.n_kept
        return dict(poses=self._poses_dict(o, ie, ih, pts), slot=int(res.slot), n_slot_inliers=int(res.n_slot_inliers),
                    n_kept=int(k), scaled=bool(res.scaled), matches_for_3d=m3d[:k].copy(), pts3d_in_curr=p3d[:k].copy(),
                    angles=ang[:k].copy(), R=np.array(res.R).reshape(3, 3), t=np.array(res.t),
                    T_w_c=np.array(res.T_w_c).reshape(4, 4), mean_depth=res.mean_depth, scale=res.scale,
                    mean_pixel_dist=res.mean_pixel_dist, mean_angle=res.mean_angle, median_angle=res.median_angle,
                    min_angle=res.min_angle, max_angle=res.max_angle, criteria=[bool(c) for c in res.criteria],
                    good=bool(res.good))

    def debug_init_finish(self):
        """Record of the last init_two_view: what k_init_finish wrote per entry of the chosen slot's inlier list ->
        dict(p_curr (m x 3 f32, unscaled), cosang, pixdist (m f64))."""
        n = C.c_int()
        self._chk(self.lib.mvo_debug_get_init_finish(self.h, None, None, None, 0, C.byref(n)))
        m = n.value
        pc, cs, pd = np.zeros((max(m, 1), 3), np.float32), np.zeros(max(m, 1)), np.zeros(max(m, 1))
        self._chk(self.lib.mvo_debug_get_init_finish(self.h, _p(pc), _p(cs), _p(pd), len(cs), C.byref(n)))
        return dict(p_curr=pc[:m].copy(), cosang=cs[:m].copy(), pixdist=pd[:m].copy())

    def debug_homography(self):
        counts = np.zeros(2000, np.int32)
        info = np.zeros(6, np.int32)
        it = self.lib.mvo_debug_get_homography(self.h, _p(counts), 2000, _p(info))
        if it < 0:
            self._chk(it)
        return dict(counts=counts[:it].copy(), best_iter=int(info[0]), iters_run=int(info[1]), evaluated=int(info[2]),
                    n_subsets=int(info[3]), lm_iters=int(info[4]), dlt=int(info[5]))

    def debug_pnp(self, cap=4096):
        models = np.zeros((cap, 12))
        counts = np.zeros(cap, np.int32)
        info = np.zeros(6, np.int32)
        h = self.lib.mvo_debug_get_pnp(self.h, _p(models), _p(counts), cap, _p(info))
        if h < 0:
            self._chk(h)
        return dict(models=models[:h].copy(), counts=counts[:h].copy(), best_iter=int(info[0]), iters_run=int(info[1]),
                    dlt=int(info[2]), lm_iters=int(info[3]), lm_evals=int(info[4]), n_hyp=int(info[5]))

    # ---- measurement / debug
    def last_error(self):
        return (self.lib.mvo_last_error(self.h) or b"").decode() if self.h else ""

    def synchronize(self):
        self._chk(self.lib.mvo_synchronize(self.h))

    def profile_enable(self, on=True):
        self._chk(self.lib.mvo_profile_enable(self.h, int(on)))

    def profile_reset(self):
        self._chk(self.lib.mvo_profile_reset(self.h))

    def profile_get(self):
        arr = (KernelTime * 64)()
        n = self.lib.mvo_profile_get(self.h, arr, 64)
        return {arr[i].name.decode(): (arr[i].launches, arr[i].total_ms) for i in range(min(n, 64))}

    def ba_launch_stats(self, reset=False):
        a, b, ms = C.c_longlong(), C.c_longlong(), C.c_double()
        rw, rs = C.c_longlong(), C.c_longlong()
        rc = C.c_double()
        self.lib.mvo_debug_ba_resident_stats(self.device, C.byref(rw), C.byref(rs))   # (before a reset clears them)
        self.lib.mvo_debug_ba_resident_cycles(self.device, C.byref(rc))
        self.lib.mvo_ba_launch_stats(self.device, C.byref(a), C.byref(b), C.byref(ms), int(reset))
        return dict(launches=a.value, windows=b.value, ms=ms.value, resident_windows=rw.value, resident_grid_starts=rs.value,
                    resident_cycles=rc.value)

    def ba_service_times(self):
        """Wall-clock of the BA launch thread's stages since the last stats reset (ms)."""
        t = (C.c_double * 5)()
        self.lib.mvo_debug_ba_service_times(self.device, t)
        return dict(zip(("wait_for_work", "wait_for_batch", "issue", "wait_for_kernel", "publish"), [round(v, 3) for v in t]))

    def debug_ba_phases(self):
        arr = (C.c_longlong * 16)()
        g = C.c_int()
        self._chk(self.lib.mvo_debug_get_ba_phases(self.h, arr, 16, C.byref(g)))
        names = ["lin", "hpp", "pt+xchg", "t1", "schur", "publish+bar", "assemble", "ldlt", "backsub", "chi2",
                 "chi2xchg", "total", "schur.loop", "schur.wait", "schur.acc", "x15"]
        return {"wgs": g.value, **{n: arr[i] for i, n in enumerate(names)}}

    def debug_level(self, level, blurred=False):
        w, h, s = C.c_int(), C.c_int(), C.c_int()
        self._chk(self.lib.mvo_debug_get_level(self.h, level, int(blurred), None, 0, C.byref(w), C.byref(h), C.byref(s)))
        buf = np.zeros((h.value + 64, s.value), np.uint8)
        self._chk(self.lib.mvo_debug_get_level(self.h, level, int(blurred), _p(buf), buf.size, None, None, None))
        return buf[:, :w.value + 64].copy()

    def debug_candidates(self):
        n = C.c_int()
        self._chk(self.lib.mvo_debug_get_candidates(self.h, None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), CANDIDATE_DTYPE)
        self._chk(self.lib.mvo_debug_get_candidates(self.h, _p(out), len(out), C.byref(n)))
        return out[:n.value].copy()


def set_wait_policy(device, policy):
    """How host threads wait for `device`: "spin" | "yield" | "block" | "auto" (mvo_set_wait_policy)."""
    r = load_library().mvo_set_wait_policy(int(device), {"auto": 0, "spin": 1, "yield": 2, "block": 3}[policy])
    if r != MVO_OK:
        raise MvoError(r, "mvo_set_wait_policy")


def debug_set(key, value):
    r = load_library().mvo_debug_set(key.encode(), int(value))
    if r != MVO_OK:
        raise MvoError(r, "unknown debug key")


def rodrigues(rvec):
    """cv::Rodrigues(rvec) -> 3x3 (vo.cpp:334)."""
    r = np.ascontiguousarray(rvec, np.float64).reshape(3)
    R = np.zeros((3, 3))
    if load_library().mvo_rodrigues(_p(r), _p(R)) != MVO_OK:
        raise MvoError(MVO_ERR_INVALID, "mvo_rodrigues")
    return R


def fundamental_from_poses(T_w_c_1, T_w_c_2, K):
    """mvo_fundamental_from_poses: F (3 x 3, x2^T F x1 = 0 in pixels) of two camera-to-world poses; K = 3 x 3 or
    dict(fx, fy, cx, cy).  Host-side, needs no GPU."""
    T1 = np.ascontiguousarray(T_w_c_1, np.float64).reshape(16)
    T2 = np.ascontiguousarray(T_w_c_2, np.float64).reshape(16)
    if isinstance(K, dict):
        fx, fy, cx, cy = K["fx"], K["fy"], K["cx"], K["cy"]
    else:
        K = np.asarray(K, np.float64)
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    F = np.zeros(9)
    r = load_library().mvo_fundamental_from_poses(_p(T1), _p(T2), C.c_double(fx), C.c_double(fy), C.c_double(cx),
                                                  C.c_double(cy), _p(F))
    if r != MVO_OK:
        raise MvoError(r, "mvo_fundamental_from_poses: singular pose or fx / fy 0")
    return F.reshape(3, 3)


def predict_pose(T_w_c_prev2, T_w_c_prev):
    """mvo_predict_pose: T_prev * (inv(T_prev2) * T_prev), the constant-velocity prediction of the next camera-to-world pose
    (4 x 4); T_w_c_prev2 None: T_prev.  Host-side, needs no GPU."""
    T2 = None if T_w_c_prev2 is None else np.ascontiguousarray(T_w_c_prev2, np.float64).reshape(16)
    T1 = np.ascontiguousarray(T_w_c_prev, np.float64).reshape(16)
    out = np.zeros(16)
    r = load_library().mvo_predict_pose(_p(T2), _p(T1), _p(out))
    if r != MVO_OK:
        raise MvoError(r, "mvo_predict_pose: singular T_w_c_prev2")
    return out.reshape(4, 4)


def retain_good_triangulation(pts3d_in_curr, T_w_c_curr, T_w_c_ref, min_triang_angle=1.0, max_ratio_to_median=20.0):
    """VisualOdometry::retainGoodTriangulationResult_ -> (kept indices, all angles in degrees)."""
    p = np.ascontiguousarray(pts3d_in_curr, np.float32).reshape(-1, 3)
    Tc = np.ascontiguousarray(T_w_c_curr, np.float64).reshape(4, 4)
    Tr = np.ascontiguousarray(T_w_c_ref, np.float64).reshape(4, 4)
    n = len(p)
    keep, ang, cnt = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1)), C.c_int()
    r = load_library().mvo_retain_good_triangulation(_p(p), n, _p(Tc), _p(Tr), C.c_double(min_triang_angle),
                                                     C.c_double(max_ratio_to_median), _p(keep), C.byref(cnt), _p(ang))
    if r != MVO_OK:
        raise MvoError(r, "mvo_retain_good_triangulation")
    return keep[:cnt.value].copy(), ang[:n].copy()


def remove_duplicated_matches(matches):
    """geometry::removeDuplicatedMatches (feature_match.cpp:241-260) -- host-side, needs no GPU."""
    m = np.ascontiguousarray(matches, DMATCH_DTYPE).copy()
    n = C.c_int(len(m))
    r = load_library().mvo_remove_duplicated_matches(_p(m), C.byref(n))
    if r != MVO_OK:
        raise MvoError(r, "mvo_remove_duplicated_matches")
    return m[:n.value].copy()


# ------------------------------------------------------------------------------------------------------
# Mirror of the reference's free-function interface (my_slam::geometry / my_slam::optimization) with the
# same latching behaviour as its function-local statics.  `Config` plays basics::Config (config.h:16-50).
class Config:
    """basics::Config stand-in holding config/config.yaml:63-123 values; get_int reproduces the
    cv::FileNode -> int rounding that turns lowe_method_dist_ratio 0.8 into 1 (feature_match.cpp:137-139)."""
    values = {
        "number_of_keypoints_to_extract": 8000, "max_number_of_keypoints": 1500, "scale_factor": 1.2,
        "level_pyramid": 4, "score_threshold": 20,
        "xiang_gao_method_match_ratio": 2, "lowe_method_dist_ratio": 0.8, "method_3_feature_dist_threshold": 50.0,
        "kpts_uniform_selection_grid_size": 16, "kpts_uniform_selection_max_pts_per_grid": 8,
        "num_prev_frames_to_opti_by_ba": 5, "information_matrix": "1.0 0.0 0.0 1.0", "is_ba_fix_map_points": "true",
    }

    @classmethod
    def get(cls, key):
        if key not in cls.values:
            raise RuntimeError("Key " + key + " does not exist")  # config.cpp:34-35
        return cls.values[key]

    @classmethod
    def get_int(cls, key):
        return int(np.rint(float(cls.get(key))))  # cv::FileNode real -> int rounds


_default_ctx = None


def default_context():
    """The process-wide ctx behind the free functions (the reference's function-local statics)."""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(nfeatures=Config.get_int("number_of_keypoints_to_extract"),
                               scale_factor=float(Config.get("scale_factor")),
                               nlevels=Config.get_int("level_pyramid"),
                               fast_threshold=Config.get_int("score_threshold"),
                               max_keypoints=Config.get_int("max_number_of_keypoints"),
                               grid_size=Config.get_int("kpts_uniform_selection_grid_size"),
                               grid_max_per_cell=Config.get_int("kpts_uniform_selection_max_pts_per_grid"))
    return _default_ctx


def reset_default_context():
    global _default_ctx
    if _default_ctx is not None:
        _default_ctx.close()
    _default_ctx = None


def calcKeyPoints(image):
    return default_context().calc_keypoints(image)


def calcDescriptors(image, keypoints):
    return default_context().calc_descriptors(image, keypoints)


def selectUniformKptsByGrid(keypoints, image_rows, image_cols):
    return default_context().select_uniform_kpts_by_grid(keypoints, image_rows, image_cols)


def matchFeatures(descriptors_1, descriptors_2, method_index=1, is_print_res=False, keypoints_1=None,
                  keypoints_2=None, max_matching_pixel_dist=0.0):
    xy1 = xy2 = None
    if keypoints_1 is not None and len(keypoints_1):
        xy1 = np.stack([keypoints_1["x"], keypoints_1["y"]], 1)
        xy2 = np.stack([keypoints_2["x"], keypoints_2["y"]], 1)
    return default_context().match_features(descriptors_1, descriptors_2, method_index,
                                            float(Config.get_int("xiang_gao_method_match_ratio")),
                                            float(Config.get_int("lowe_method_dist_ratio")), xy1, xy2,
                                            max_matching_pixel_dist)


removeDuplicatedMatches = remove_duplicated_matches


def bundleAdjustment(v_pts_2d, v_pts_2d_to_3d_idx, K, pts_3d, v_camera_g2o_poses, information_matrix,
                     is_fix_map_pts=False, is_update_map_pts=True):
    """optimization::bundleAdjustment (g2o_ba.h:23-30) with Python containers standing in for the pointer
    lists: v_pts_2d[i] = float32 [n_i, 2] pixels of frame i, v_pts_2d_to_3d_idx[i] = map-point ids,
    pts_3d = dict id -> float32[3] (mutated in place when is_update_map_pts), v_camera_g2o_poses = list of
    4x4 float64 cam->world matrices (mutated in place)."""
    ids = list(pts_3d.keys())
    slot = {pid: i for i, pid in enumerate(ids)}
    pts = np.array([pts_3d[i] for i in ids], np.float64).reshape(-1, 3)
    ep, el, uv = [], [], []
    for i, (p2, idx) in enumerate(zip(v_pts_2d, v_pts_2d_to_3d_idx)):
        for j in range(len(p2)):
            ep.append(i)
            el.append(slot[idx[j]])
            uv.append(p2[j])
    poses = np.array(v_camera_g2o_poses, np.float64).reshape(-1, 16)
    K = np.asarray(K, np.float64)
    P, X, st = default_context().bundle_adjustment(
        poses, pts, np.array(ep, np.int32), np.array(el, np.int32), np.array(uv, np.float64).reshape(-1, 2),
        K[0, 0], K[0, 2], K[1, 2], np.asarray(information_matrix, np.float64).ravel(), 1.0, is_fix_map_pts)
    for i in range(len(v_camera_g2o_poses)):
        v_camera_g2o_poses[i][...] = P[i]
    if is_update_map_pts:
        for pid, x in zip(ids, X):
            pts_3d[pid][...] = x.astype(np.float32)   # double -> cv::Point3f (g2o_ba.cpp:313-315)
    return st
