"""TEST INFRASTRUCTURE: ctypes front end of tests/init_finish_restatement.cpp (the finish of the monocular
initialisation restated sequentially in the arithmetic csrc/init_wave.h declares) and mvo_init_two_view composed from the
restatements: everything up to the chosen slot from tests/pose_restate.py, the finish from the C++ restatement."""
import ctypes as C
import os
import subprocess

import numpy as np

import init_restate as IR
import pose_restate as PR

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "init_finish_restatement.cpp")
DEPS = [SRC, os.path.join(HERE, "..", "oracle", "linalg_oracle.h")]
OUT = os.path.join(HERE, "sim", "_build", "libfinish_restate.so")

DEFAULTS = dict(min_triang_angle=1.0, max_ratio_to_median=20.0, assumed_mean_depth=0.8, min_inlier_matches=15,
                min_pixel_dist=50.0, min_median_triangulation_angle=2.0)   # config/config.yaml:105-113


class Params(C.Structure):
    _fields_ = [("min_triang_angle", C.c_double), ("max_ratio_to_median", C.c_double), ("assumed_mean_depth", C.c_double),
                ("min_inlier_matches", C.c_int), ("min_pixel_dist", C.c_double),
                ("min_median_triangulation_angle", C.c_double)]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Restatement:
    def __init__(self):
        if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(d) for d in DEPS):
            os.makedirs(os.path.dirname(OUT), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math", "-std=c++17",
                                   "-fPIC", "-shared", "-o", OUT, SRC])
        self.lib = C.CDLL(OUT)
        self.lib.fr_compose.argtypes = [C.c_void_p] * 4
        self.lib.fr_compose.restype = None
        self.lib.fr_finish.argtypes = [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 14
        self.lib.fr_finish.restype = C.c_int
        self.PR = PR.Restatement()

    def compose(self, T_ref, R, t):
        T_ref = np.ascontiguousarray(T_ref, np.float64).reshape(16)
        R = np.ascontiguousarray(R, np.float64).reshape(9)
        t = np.ascontiguousarray(t, np.float64).reshape(3)
        T = np.zeros(16)
        self.lib.fr_compose(_p(T_ref), _p(R), _p(t), _p(T))
        return T.reshape(4, 4)

    def finish(self, p1, px1, px2, R, t, T_ref=None, **params):
        """The finish on one solution: p1 (m x 3 f32, camera 1), px1 / px2 (m x 2 f32), in list order -> dict with the
        per-entry arrays (p_curr, cosang, pixdist, angle), kept (positions in the list) and the fields of
        mvo_init_result.  Asserts that no angle is NaN."""
        p1 = np.ascontiguousarray(p1, np.float32).reshape(-1, 3)
        a = np.ascontiguousarray(px1, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(px2, np.float32).reshape(-1, 2)
        m = len(p1)
        assert len(a) == m and len(b) == m
        R = np.ascontiguousarray(R, np.float64).reshape(9).copy()
        t = np.ascontiguousarray(t, np.float64).reshape(3).copy()
        Tr = np.ascontiguousarray(np.eye(4) if T_ref is None else T_ref, np.float64).reshape(16)
        prm = dict(DEFAULTS)
        prm.update(params)
        cp = Params(prm["min_triang_angle"], prm["max_ratio_to_median"], prm["assumed_mean_depth"],
                    int(prm["min_inlier_matches"]), prm["min_pixel_dist"], prm["min_median_triangulation_angle"])
        k = max(m, 1)
        pc, cs, pd, ang = np.zeros((k, 3), np.float32), np.zeros(k), np.zeros(k), np.zeros(k)
        kept, kpts, kang = np.zeros(k, np.int32), np.zeros((k, 3), np.float32), np.zeros(k)
        T, scal, flags = np.zeros(16), np.zeros(7), np.zeros(6, np.int32)
        n_nan = self.lib.fr_finish(_p(p1), _p(a), _p(b), m, _p(R), _p(t), _p(Tr), C.byref(cp), _p(pc), _p(cs), _p(pd),
                                   _p(ang), _p(kept), _p(kpts), _p(kang), _p(T), _p(scal), _p(flags))
        assert n_nan == 0, "%d NaN triangulation angles in a test input" % n_nan
        nk = int(flags[0])
        return dict(p_curr=pc[:m], cosang=cs[:m], pixdist=pd[:m], angle=ang[:m], kept=kept[:nk].copy(),
                    n_slot_inliers=m, n_kept=nk, scaled=bool(flags[1]), pts3d_in_curr=kpts[:nk].copy(),
                    angles=kang[:nk].copy(), R=R.reshape(3, 3), t=t, T_w_c=T.reshape(4, 4), mean_depth=scal[0],
                    scale=scal[1], mean_pixel_dist=scal[2], mean_angle=scal[3], median_angle=scal[4], min_angle=scal[5],
                    max_angle=scal[6], criteria=[bool(c) for c in flags[2:5]], good=bool(flags[5]))

    def init_two_view(self, O, kp1, kp2, K, T_w_c_ref=None, **params):
        """The same dict as mvo.Context.init_two_view (plus the per-entry arrays under "finish"), from the restatements."""
        a = np.ascontiguousarray(kp1, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(kp2, np.float32).reshape(-1, 2)
        Tr = np.ascontiguousarray(np.eye(4) if T_w_c_ref is None else T_w_c_ref, np.float64).reshape(4, 4)
        poses = self.PR.estimate_possible_relative_poses(O, a, b, K)
        best = poses["best"]
        if best < 0:   # DESIGN.md section 2, deviation 12
            e0, ef = np.zeros(0), np.zeros((0, 3), np.float32)
            return dict(poses=poses, slot=-1, n_slot_inliers=0, n_kept=0, scaled=False, matches_for_3d=np.zeros(0, np.int32),
                        pts3d_in_curr=ef, angles=e0, R=np.zeros((3, 3)), t=np.zeros(3), T_w_c=Tr.copy(), mean_depth=0.0,
                        scale=0.0, mean_pixel_dist=0.0, mean_angle=0.0, median_angle=0.0, min_angle=0.0, max_angle=0.0,
                        criteria=[False] * 3, good=False, finish=dict(p_curr=ef, cosang=e0, pixdist=e0))
        s = poses["solutions"][best]
        inl = np.asarray(s["inliers"], np.int64)
        f = self.finish(s["pts3d"], a[inl], b[inl], s["R"], s["t"], Tr, **params)
        out = {k: f[k] for k in ("n_slot_inliers", "n_kept", "scaled", "pts3d_in_curr", "angles", "R", "t", "T_w_c",
                                 "mean_depth", "scale", "mean_pixel_dist", "mean_angle", "median_angle", "min_angle",
                                 "max_angle", "criteria", "good")}
        out.update(poses=poses, slot=best, matches_for_3d=inl[f["kept"]].astype(np.int32), finish=f)
        return out


kdict = IR.kdict
