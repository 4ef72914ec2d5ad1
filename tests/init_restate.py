"""TEST INFRASTRUCTURE: ctypes front end of tests/init_motion_restatement.cpp (estiMotionByEssential after its RANSAC
and the ORB-SLAM E / H scores, restated in the arithmetic csrc/em_wave.h declares).  The RANSAC stage and its selected
E come from the CPU oracle (orc_find_essential_inliers)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "init_motion_restatement.cpp")
DEPS = [SRC, os.path.join(HERE, "..", "oracle", "linalg_oracle.h")]
OUT = os.path.join(HERE, "sim", "_build", "libinit_restate.so")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def kdict(K):
    K = np.asarray(K, float)
    return dict(fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2])


def scale_by_22(M):
    """M * (1 / M(2,2)): the rule the reference's `M /= M(2,2)` follows (cv::Mat::convertTo)."""
    M = np.asarray(M, np.float64)
    return M * (1.0 / M[2, 2])


class Restatement:
    def __init__(self):
        if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(d) for d in DEPS):
            os.makedirs(os.path.dirname(OUT), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math", "-std=c++17",
                                   "-fPIC", "-shared", "-o", OUT, SRC])
        self.lib = C.CDLL(OUT)
        self.lib.ir_recover_pose.argtypes = [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 10
        self.lib.ir_recover_pose.restype = None
        self.lib.ir_check_init_scores.argtypes = ([C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double]
                                                  + [C.c_void_p] * 6)
        self.lib.ir_check_init_scores.restype = None
        self.lib.ir_invert3.argtypes = [C.c_void_p, C.c_void_p]
        self.lib.ir_invert3.restype = None

    def recover_pose(self, kp1, kp2, K, E_raw, mask=None):
        a = np.ascontiguousarray(kp1, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(kp2, np.float32).reshape(-1, 2)
        n = len(a)
        k = kdict(K)
        k4 = np.array([k["fx"], k["fy"], k["cx"], k["cy"]])
        Er = np.ascontiguousarray(E_raw, np.float64).reshape(9)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        E, R, t, D = np.zeros(9), np.zeros(9), np.zeros(3), np.zeros(21)
        good = np.zeros(4, np.int32)
        chosen = np.zeros(1, np.int32)
        masks = np.zeros(max(n, 1), np.uint8)
        self.lib.ir_recover_pose(_p(a), _p(b), n, _p(k4), _p(Er), _p(m), _p(E), _p(R), _p(t), _p(good), _p(chosen), _p(D),
                                 _p(masks))
        return dict(E=E.reshape(3, 3), R=R.reshape(3, 3), t=t, good=good, chosen=int(chosen[0]), R1=D[:9].reshape(3, 3),
                    R2=D[9:18].reshape(3, 3), tdec=D[18:].copy(), masks=masks[:n].copy())

    def esti_motion_by_essential(self, O, kp1, kp2, K, prob=0.999, threshold=1.0):
        """The oracle's findEssentialMat, then the restated remainder.  found = False where the device reports no model
        (n < 5, no RANSAC model, n == 5 with several five-point candidates)."""
        a = np.ascontiguousarray(kp1, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(kp2, np.float32).reshape(-1, 2)
        n = len(a)
        none = dict(found=False, E=None, R=None, t=None, inliers=np.zeros(0, np.int32), rp=None)
        if n < 5:
            return none
        em = O.find_essential_inliers(a, b, kdict(K), prob, threshold)
        if em["best_iter"] < 0 or (n == 5 and em["n_models"] != 1):
            return none
        inl = em["inliers"]
        mask = None
        if n > 5:
            mask = np.zeros(n, np.uint8)
            mask[inl] = 1
        rp = self.recover_pose(a, b, K, em["E"], mask)
        return dict(found=True, E=rp["E"], R=rp["R"], t=rp["t"], inliers=inl, rp=rp, E_raw=em["E"])

    def check_init_scores(self, kp1, kp2, K, E, inl_e, H, inl_h, sigma=1.0):
        a = np.ascontiguousarray(kp1, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(kp2, np.float32).reshape(-1, 2)
        k = kdict(K)
        k4 = np.array([k["fx"], k["fy"], k["cx"], k["cy"]])
        Ed = None if E is None else np.ascontiguousarray(E, np.float64).reshape(9)
        Hd = None if H is None else np.ascontiguousarray(H, np.float64).reshape(9)
        le = np.ascontiguousarray(inl_e if inl_e is not None else [], np.int32).reshape(-1)
        lh = np.ascontiguousarray(inl_h if inl_h is not None else [], np.int32).reshape(-1)
        ke, kh = np.zeros(max(len(le), 1), np.int32), np.zeros(max(len(lh), 1), np.int32)
        se, sh = np.zeros(1), np.zeros(1)
        ne, nh = np.zeros(1, np.int32), np.zeros(1, np.int32)
        self.lib.ir_check_init_scores(_p(a), _p(b), _p(k4), _p(Ed), _p(le), len(le), _p(Hd), _p(lh), len(lh), sigma, _p(se),
                                      _p(sh), _p(ke), _p(ne), _p(kh), _p(nh))
        return dict(score_e=float(se[0]), score_h=float(sh[0]), kept_e=ke[:ne[0]].copy(), kept_h=kh[:nh[0]].copy())

    def invert3(self, M):
        M = np.ascontiguousarray(M, np.float64).reshape(9)
        out = np.zeros(9)
        self.lib.ir_invert3(_p(M), _p(out))
        return out.reshape(3, 3)
