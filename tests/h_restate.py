"""TEST INFRASTRUCTURE: ctypes front end of tests/homography_restatement.cpp (findHomography restated in the canonical
arithmetic csrc/h_wave.h declares) and the synthetic two-view problems the initialisation tests share."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "homography_restatement.cpp")
DEPS = [SRC, os.path.join(HERE, "..", "oracle", "linalg_oracle.h")]
OUT = os.path.join(HERE, "sim", "_build", "libh_restate.so")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Restatement:
    def __init__(self):
        if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(d) for d in DEPS):
            os.makedirs(os.path.dirname(OUT), exist_ok=True)
            subprocess.check_call(["g++", "-O2", "-march=x86-64-v3", "-ffp-contract=off", "-fno-fast-math", "-std=c++17",
                                   "-fPIC", "-shared", "-o", OUT, SRC])
        self.lib = C.CDLL(OUT)
        self.lib.hr_find_homography.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p]

    def find_homography(self, src, dst, threshold=3.0, confidence=0.995):
        a = np.ascontiguousarray(src, np.float32).reshape(-1, 2)
        b = np.ascontiguousarray(dst, np.float32).reshape(-1, 2)
        n = len(a)
        H = np.zeros(9)
        mask = np.zeros(max(n, 1), np.uint8)
        counts = np.zeros(2000, np.int32)
        info = np.zeros(6, np.int32)
        found = self.lib.hr_find_homography(_p(a), _p(b), n, threshold, confidence, _p(H), _p(mask), _p(counts), _p(info))
        return dict(H=H.reshape(3, 3) if found else None, inliers=np.nonzero(mask[:n])[0].astype(np.int32) if found
                    else np.zeros(0, np.int32), counts=counts[:info[1]].copy(), best_iter=int(info[0]),
                    iters_run=int(info[1]), n_subsets=int(info[3]), lm_iters=int(info[4]), dlt=int(info[5]))

    def check_subset(self, src, dst, idx):
        a = np.ascontiguousarray(src, np.float32)
        b = np.ascontiguousarray(dst, np.float32)
        i = np.ascontiguousarray(idx, np.int32)
        return bool(self.lib.hr_check_subset(_p(a), _p(b), _p(i)))

    def subsets(self, src, dst, iters=2000):
        a = np.ascontiguousarray(src, np.float32)
        b = np.ascontiguousarray(dst, np.float32)
        out = np.zeros((iters, 4), np.int32)
        k = self.lib.hr_subsets(_p(a), _p(b), len(a), iters, _p(out))
        return out[:k]

    def run_kernel4(self, src, dst, idx):
        a = np.ascontiguousarray(src, np.float32)
        b = np.ascontiguousarray(dst, np.float32)
        i = np.ascontiguousarray(idx, np.int32)
        H = np.zeros(9)
        ok = self.lib.hr_run_kernel4(_p(a), _p(b), _p(i), _p(H))
        return H.reshape(3, 3) if ok else None


K_DEFAULT = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1]])


def rot(axis, deg):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    a = np.deg2rad(deg)
    X = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * X + (1 - np.cos(a)) * X @ X


def two_view(n, seed, planar=True, outlier_frac=0.0, noise=0.5, rotation_only=False, K=K_DEFAULT):
    """n matches between camera 1 = [I|0] and camera 2 = [R|t] (x2 = R x1 + t) of a plane n^T X = d (planar) or of a
    thick scene.  Outliers are moved at least 25 px away from their true match.  Returns pixels (float32), the
    ground-truth inlier flags and the plane homography K (R + t n^T / d) K^-1 scaled to H(2,2) = 1."""
    rng = np.random.RandomState(seed)
    R = rot([0.2, 1.0, 0.1], 6.0)
    t = np.zeros(3) if rotation_only else np.array([0.3, 0.05, 0.02])
    nrm = np.array([0.1, -0.2, 1.0])
    nrm /= np.linalg.norm(nrm)
    d = 4.0
    uv = rng.uniform([40, 40], [600, 440], (n, 2))
    rays = np.linalg.solve(K, np.c_[uv, np.ones(n)].T).T
    if planar:
        depth = d / (rays @ nrm)
    else:
        depth = rng.uniform(2.5, 8.0, n)
    X1 = rays * depth[:, None]
    X2 = X1 @ R.T + t
    p2 = X2 @ K.T
    uv2 = p2[:, :2] / p2[:, 2:]
    uv2 = uv2 + rng.normal(0, noise, uv2.shape) if noise else uv2
    gt = np.ones(n, bool)
    n_out = int(round(outlier_frac * n))
    if n_out:
        idx = rng.choice(n, n_out, replace=False)
        for i in idx:
            while True:
                q = rng.uniform([0, 0], [640, 480])
                if np.linalg.norm(q - uv2[i]) > 25:
                    break
            uv2[i] = q
        gt[idx] = False
    Ht = K @ (R + np.outer(t, nrm) / d) @ np.linalg.inv(K)
    return dict(src=uv.astype(np.float32), dst=uv2.astype(np.float32), inlier_gt=gt, H_true=Ht / Ht[2, 2], R=R, t=t,
                n=nrm, d=d, K=K)
