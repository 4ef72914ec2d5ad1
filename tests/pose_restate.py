"""TEST INFRASTRUCTURE: ctypes front end of tests/init_pose_restatement.cpp (the homography decomposition, the
visibility filter, the choice and invRt of the monocular initialisation, restated in the arithmetic csrc/hd_wave.h
declares) and the whole of helperEstimatePossibleRelativePosesByEpipolarGeometry composed from the restatements: the
E branch from tests/init_restate.py (on the CPU oracle's RANSAC), findHomography from tests/h_restate.py, the points
from the oracle's triangulate_points and the scores from tests/init_restate.py."""
import ctypes as C
import os
import subprocess

import numpy as np

import h_restate as HR
import init_restate as IR

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "init_pose_restatement.cpp")
DEPS = [SRC, os.path.join(HERE, "..", "oracle", "linalg_oracle.h")]
OUT = os.path.join(HERE, "sim", "_build", "libpose_restate.so")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def k4(K):
    k = IR.kdict(K)
    return np.array([k["fx"], k["fy"], k["cx"], k["cy"]])


class Restatement:
    def __init__(self):
        if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(d) for d in DEPS):
            os.makedirs(os.path.dirname(OUT), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math", "-std=c++17",
                                   "-fPIC", "-shared", "-o", OUT, SRC])
        self.lib = C.CDLL(OUT)
        self.lib.pr_decompose.argtypes = [C.c_void_p] * 8
        self.lib.pr_decompose.restype = C.c_int
        self.lib.pr_normalise_t.argtypes = [C.c_void_p] * 2
        self.lib.pr_normalise_t.restype = None
        self.lib.pr_filter.argtypes = [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p]
        self.lib.pr_filter.restype = None
        self.lib.pr_choose.argtypes = [C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        self.lib.pr_choose.restype = C.c_int
        self.lib.pr_inv_rt.argtypes = [C.c_void_p] * 2
        self.lib.pr_inv_rt.restype = None
        self.HR = HR.Restatement()
        self.IR = IR.Restatement()

    def decompose(self, Hs, K):
        """decomposeHomographyMat of the scaled H -> dict(count, rotation_only, index, Hn, w, Rs, ts, normals)."""
        H = np.ascontiguousarray(Hs, np.float64).reshape(9)
        Hn, w, Rs, ts, ns = np.zeros(9), np.zeros(3), np.zeros(36), np.zeros(12), np.zeros(12)
        br = np.zeros(2, np.int32)
        cnt = self.lib.pr_decompose(_p(H), _p(k4(K)), _p(Hn), _p(w), _p(br), _p(Rs), _p(ts), _p(ns))
        return dict(count=cnt, rotation_only=bool(br[0]), index=int(br[1]), Hn=Hn.reshape(3, 3), w=w,
                    Rs=Rs.reshape(4, 3, 3), ts=ts.reshape(4, 3), normals=ns.reshape(4, 3))

    def normalise_t(self, t):
        t = np.ascontiguousarray(t, np.float64).reshape(3)
        out = np.zeros(3)
        self.lib.pr_normalise_t(_p(t), _p(out))
        return out

    def filter(self, kp1, kp2, inliers, K, dec):
        a = np.ascontiguousarray(kp1, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(kp2, np.float32).reshape(-1, 2)
        lst = np.ascontiguousarray(inliers, np.int32).reshape(-1)
        Rs = np.ascontiguousarray(dec["Rs"], np.float64)
        ns = np.ascontiguousarray(dec["normals"], np.float64)
        rej = np.zeros(4, np.int32)
        self.lib.pr_filter(_p(a), _p(b), _p(lst), len(lst), _p(k4(K)), _p(Rs), _p(ns), dec["count"], _p(rej))
        return rej

    def choose(self, score_e, score_h, has_e, nz):
        """nz: |n_z| of the H slots 1..k in slot order."""
        arr = np.ascontiguousarray([0.0] + list(nz), np.float64)
        ratio = np.zeros(1)
        best = self.lib.pr_choose(score_e, score_h, int(bool(has_e)), _p(arr), len(nz), _p(ratio))
        return best, float(ratio[0])

    def inv_rt(self, R, t):
        R = np.ascontiguousarray(R, np.float64).reshape(9).copy()
        t = np.ascontiguousarray(t, np.float64).reshape(3).copy()
        self.lib.pr_inv_rt(_p(R), _p(t))
        return R.reshape(3, 3), t

    def esti_motion_by_homography(self, kp1, kp2, K, threshold=3.0, confidence=0.995):
        """findHomography (the restatement), H / H(2,2), the decomposition, t / |t| and the filter -> dict(found, H,
        inliers, dec, rejected, survivors, Rs, ts, normals)."""
        h = self.HR.find_homography(kp1, kp2, threshold, confidence)
        if h["H"] is None:
            return dict(found=False, H=None, inliers=h["inliers"], dec=None, rejected=np.zeros(4, np.int32),
                        survivors=[], Rs=[], ts=[], normals=[])
        H = IR.scale_by_22(h["H"])
        dec = self.decompose(H, K)
        rej = self.filter(kp1, kp2, h["inliers"], K, dec)
        surv = [c for c in range(dec["count"]) if rej[c] == 0]
        return dict(found=True, H=H, inliers=h["inliers"], dec=dec, rejected=rej, survivors=surv,
                    Rs=[dec["Rs"][c] for c in surv], ts=[self.normalise_t(dec["ts"][c]) for c in surv],
                    normals=[dec["normals"][c] for c in surv])

    def estimate_possible_relative_poses(self, O, kp1, kp2, K, prob=0.999, threshold=1.0, h_threshold=3.0,
                                         h_confidence=0.995, sigma=1.0, motion_cam2_to_cam1=True):
        """The same dict as mvo.Context.estimate_possible_relative_poses, from the restatements."""
        a = np.ascontiguousarray(kp1, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(kp2, np.float32).reshape(-1, 2)
        kd = IR.kdict(K)
        e = self.IR.esti_motion_by_essential(O, a, b, K, prob, threshold)
        hb = self.esti_motion_by_homography(a, b, K, h_threshold, h_confidence)
        sols = []

        def points(inl, R, t):
            if len(inl) == 0:
                return np.zeros((0, 3), np.float32)
            return O.triangulate_points(a[inl], b[inl], kd, R, t)[0]

        if e["found"]:
            sols.append(dict(kind="E", R=e["R"], t=e["t"], normal=None, inliers=e["inliers"],
                             pts3d=points(e["inliers"], e["R"], e["t"]), candidate=-1))
        else:
            sols.append(None)
        for c, R, t, nrm in zip(hb["survivors"], hb["Rs"], hb["ts"], hb["normals"]):
            sols.append(dict(kind="H", R=R, t=t, normal=nrm, inliers=hb["inliers"], pts3d=points(hb["inliers"], R, t),
                             candidate=c))
        sc = self.IR.check_init_scores(a, b, K, e["E"] if e["found"] else None, e["inliers"], hb["H"], hb["inliers"], sigma)
        best, ratio = self.choose(sc["score_e"], sc["score_h"], e["found"], [abs(s["normal"][2]) for s in sols[1:]])
        if not motion_cam2_to_cam1:
            for s in sols:
                if s is not None:
                    s["R"], s["t"] = self.inv_rt(s["R"], s["t"])
        return dict(best=best, ratio=ratio, score_e=sc["score_e"], score_h=sc["score_h"], E=e["E"] if e["found"] else None,
                    H=hb["H"], inliers_e=e["inliers"], inliers_h=hb["inliers"], solutions=sols, h=hb)
