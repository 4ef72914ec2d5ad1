"""Numpy transcription of the robust motion-only pose optimisation (include/mvo_hip.h: mvo_optimize_pose),
written from the declared arithmetic and sharing no code with the product: ORB-SLAM's PoseOptimization -- a Levenberg-Marquardt
over the six pose unknowns from a predicted pose, all matches, inliers and outliers classified round by round.  f64 throughout;
per observation the operations are numpy elementwise operations (each rounded on its own, which is the declared order); the 28
sums follow the declared order: slot k mod 256 adds its observations in ascending k from 0.0, then eight times
S <- S[even] + S[odd]; the 6 x 6 Cholesky, the Rodrigues formula (math.sin / math.cos of the C library) and the pose product are
Python floats in the written order.  Known answers: tests/test_pose_optimize_numpy.py."""
import math

import numpy as np

from projection_numpy import invert_pose

MAX_OBS, SLOTS = 4096, 256
DEFAULTS = dict(rounds=4, iterations=10, min_inliers=10, chi2_threshold=5.991, huber_delta=float(np.sqrt(np.float64(5.991))),
                rel_tolerance=1e-6)
OPTIMISED, FEW_INLIERS, FEW_IN_FRONT, NO_STEP = 0, 1, 2, 3
FR1_K = dict(fx=517.3, fy=516.5, cx=318.6, cy=255.3)
UPPER = [(r, c) for r in range(6) for c in range(r, 6)]      # the 21 entries of H, row by row


def tree_sum(terms, take):
    """The declared sum of one term per observation: an observation outside `take` contributes 0.0."""
    n = len(terms)
    padded = np.zeros(-(-max(n, 1) // SLOTS) * SLOTS)
    padded[:n] = np.where(take, terms, 0.0)
    S = np.zeros(SLOTS)
    for row in padded.reshape(-1, SLOTS):                     # ascending k inside every slot
        S = S + row
    while len(S) > 1:                                         # eight times
        S = S[0::2] + S[1::2]
    return float(S[0])


def project(R, t, p3, p2, s, K):
    """Every observation at (R, t): q (3 arrays), ax, ay, ex, ey, c."""
    fx, fy, cx, cy = (np.float64(K[k]) for k in ("fx", "fy", "cx", "cy"))
    P = p3.astype(np.float64)
    with np.errstate(all="ignore"):
        q = [((np.float64(R[r][0]) * P[:, 0] + np.float64(R[r][1]) * P[:, 1]) + np.float64(R[r][2]) * P[:, 2]) + np.float64(t[r])
             for r in range(3)]
        ax, ay = fx * q[0], fy * q[1]
        ex = (ax / q[2] + cx) - p2[:, 0].astype(np.float64)
        ey = (ay / q[2] + cy) - p2[:, 1].astype(np.float64)
        c = (ex * ex + ey * ey) * s
    return q, ax, ay, ex, ey, c


def evaluate(R, t, p3, p2, s, K, take, delta, robust):
    """-> (the 28 sums: H 21 upper entries row by row, b 6, chi2; whether every observation of `take` has q_z > 0)."""
    fx, fy = np.float64(K["fx"]), np.float64(K["fy"])
    d = np.float64(delta)
    q, ax, ay, ex, ey, c = project(R, t, p3, p2, s, K)
    with np.errstate(all="ignore"):
        d2 = d * d
        sq = np.sqrt(c)
        quad = (c <= d2) if robust else np.ones(len(c), bool)
        rho = np.where(quad, c, (np.float64(2.0) * d) * sq - d2)
        w = np.where(quad, np.float64(1.0), d / sq)
        ws = w * s
        zz = q[2] * q[2]
        a0, a2 = fx / q[2], -(ax / zz)
        b1, b2 = fy / q[2], -(ay / zz)
        zero = np.zeros(len(c))
        J0 = [a2 * q[1], a0 * q[2] - a2 * q[0], -(a0 * q[1]), a0, zero, a2]
        J1 = [b2 * q[1] - b1 * q[2], -(b2 * q[0]), b1 * q[0], zero, b1, b2]
        sums = [tree_sum(ws * (J0[r] * J0[k] + J1[r] * J1[k]), take) for r, k in UPPER]
        sums += [tree_sum(ws * (J0[r] * ex + J1[r] * ey), take) for r in range(6)]
        sums.append(tree_sum(rho, take))
    return sums, not (take & ~(q[2] > 0)).any()


def solve6(sums, lam):
    """(H + lam I) x = -b by Cholesky in the declared order; None when a pivot is not positive and finite."""
    A = [[0.0] * 6 for _ in range(6)]
    for i, (r, c) in enumerate(UPPER):
        A[c][r] = float(sums[i])
    b = [float(v) for v in sums[21:27]]
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        d = A[j][j] + lam
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        if not (d > 0.0 and d < math.inf):
            return None
        L[j][j] = math.sqrt(d)
        for r in range(j + 1, 6):
            v = A[r][j]
            for k in range(j):
                v = v - L[r][k] * L[j][k]
            L[r][j] = v / L[j][j]
    y, x = [0.0] * 6, [0.0] * 6
    for r in range(6):
        v = -b[r]
        for k in range(r):
            v = v - L[r][k] * y[k]
        y[r] = v / L[r][r]
    for r in range(5, -1, -1):
        v = y[r]
        for k in range(r + 1, 6):
            v = v - L[k][r] * x[k]
        x[r] = v / L[r][r]
    return x


def rodrigues(r):
    """The rotation matrix of the rotation vector r: rodrigues_fwd of csrc/pnp_wave.h, which tests/test_wave_linalg.py holds to
    mpmath.  3 x 3 Python floats."""
    theta = math.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    I = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    if theta < np.finfo(np.float64).eps:
        return [I[0:3], I[3:6], I[6:9]]
    c, s = math.cos(theta), math.sin(theta)
    c1, it = 1.0 - c, 1.0 / theta
    rx, ry, rz = r[0] * it, r[1] * it, r[2] * it
    rrt = [rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz]
    r_x = [0.0, -rz, ry, rz, 0.0, -rx, -ry, rx, 0.0]
    W = [c * I[k] + c1 * rrt[k] + s * r_x[k] for k in range(9)]
    return [W[0:3], W[3:6], W[6:9]]


def moved(R, t, x):
    """The left update: R' = W R, t' = W t + upsilon."""
    W = rodrigues(x[:3])
    Rn = [[(W[r][0] * R[0][c] + W[r][1] * R[1][c]) + W[r][2] * R[2][c] for c in range(3)] for r in range(3)]
    tn = [((W[r][0] * t[0] + W[r][1] * t[1]) + W[r][2] * t[2]) + x[3 + r] for r in range(3)]
    return Rn, tn


def pose_rows(R, t):
    return np.array([R[0] + [t[0]], R[1] + [t[1]], R[2] + [t[2]], [0.0, 0.0, 0.0, 1.0]], np.float64)


def optimize_pose(pts3d, pts2d, inv_sigma2, T_w_c_init, K, params=None, traces=None):
    """-> (T_w_c 4 x 4, T_c_w 4 x 4, outlier n uint8, chi2 2, info 6 int32, rows rounds x 6) as mvo_optimize_pose and
    mvo_debug_get_pose_optimize deliver them.  traces (a list) receives one list of bools per round: each trial accepted or not."""
    P = dict(DEFAULTS, **(params or {}))
    p3 = np.ascontiguousarray(pts3d, np.float32).reshape(-1, 3)
    p2 = np.ascontiguousarray(pts2d, np.float32).reshape(-1, 2)
    n = len(p3)
    assert n <= MAX_OBS and len(p2) == n
    s = np.ones(n) if inv_sigma2 is None else np.asarray(inv_sigma2, np.float32).astype(np.float64)
    T_init = np.array(T_w_c_init, np.float64).reshape(4, 4)
    T0 = np.array(invert_pose(T_init), np.float64).reshape(4, 4)
    T0[3] = (0.0, 0.0, 0.0, 1.0)
    R0, t0 = [[float(T0[r, c]) for c in range(3)] for r in range(3)], [float(T0[r, 3]) for r in range(3)]
    rows = np.zeros((0, 6))
    if n == 0:
        return T_init, T0, np.zeros(0, np.uint8), np.zeros(2), np.array([FEW_IN_FRONT, 0, 0, 0, 0, 0], np.int32), rows
    front0 = project(R0, t0, p3, p2, s, K)[0][2] > 0
    n_front = int(front0.sum())
    if n_front < P["min_inliers"]:
        return T_init, T0, np.ones(n, np.uint8), np.zeros(2), np.array([FEW_IN_FRONT, 0, 0, 0, 0, n_front], np.int32), rows
    take, inliers, status = front0, n_front, OPTIMISED
    trials_all = steps_all = 0
    rows, chi2 = [], [0.0, 0.0]
    for rnd in range(P["rounds"]):
        robust = P["rounds"] == 1 or rnd + 1 < P["rounds"]
        R, t = R0, t0
        S, _ = evaluate(R, t, p3, p2, s, K, take, P["huber_delta"], robust)
        chi2_start = S[27]
        mx = S[0]
        for i in (6, 11, 15, 18, 20):
            if S[i] > mx:
                mx = S[i]
        lam = 1e-3 * mx
        trials = steps = 0
        trace = []
        while trials < P["iterations"]:
            trials += 1
            accepted = False
            x = solve6(S, lam)
            if x is not None:
                Rn, tn = moved(R, t, x)
                N, front = evaluate(Rn, tn, p3, p2, s, K, take, P["huber_delta"], robust)
                accepted = front and N[27] < S[27]
            trace.append(accepted)
            if accepted:
                dec, tol = S[27] - N[27], P["rel_tolerance"] * S[27]
                R, t, S = Rn, tn, N
                steps += 1
                lam = lam * 0.1
                if dec <= tol:
                    break
            else:
                lam = lam * 10.0
        q, _, _, _, _, c = project(R, t, p3, p2, s, K)
        with np.errstate(all="ignore"):
            outlier = ~front0 | ~(q[2] > 0) | (c > np.float64(P["chi2_threshold"]))
        rows.append([float(inliers), chi2_start, S[27], float(trials), float(steps), float((~outlier).sum())])
        inliers, take = int((~outlier).sum()), ~outlier
        if rnd == 0:
            chi2[0] = chi2_start
        chi2[1] = S[27]
        trials_all, steps_all = trials_all + trials, steps_all + steps
        if traces is not None:
            traces.append(trace)
        if inliers < P["min_inliers"]:
            status = FEW_INLIERS
            break
    if status == OPTIMISED and steps_all == 0:
        status = NO_STEP
    T_c_w = pose_rows(R, t)
    T_w_c = T_init if status == NO_STEP else np.array(invert_pose(T_c_w), np.float64).reshape(4, 4)
    info = np.array([status, len(rows), trials_all, steps_all, inliers, n_front], np.int32)
    return T_w_c, T_c_w, outlier.astype(np.uint8), np.array(chi2), info, np.array(rows, np.float64).reshape(-1, 6)


def failed_then_accepted(trace):
    return any(not a and b for a, b in zip(trace, trace[1:]))


def rotation(axis, angle):
    """Rotation matrix about a unit axis (scene construction only)."""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def scene(rng, n, noise=0.0, moved_every=0, n_behind=0, K=FR1_K, depth=(2.0, 6.0)):
    """n world points in front of a camera with a general pose, their pixels (f32 roundings of the exact projections plus
    `noise` px of Gaussian noise; every `moved_every`-th observation moved by (40, -30) px), the last n_behind points behind the
    camera.  -> (pts3d n x 3 f32, pts2d n x 2 f32, T_w_c true 4 x 4, indices of the moved observations, indices behind)."""
    Rwc = rotation([0.3, -0.8, 0.5], 0.4)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rwc, (0.7, -0.2, 1.1)
    z = rng.uniform(depth[0], depth[1], n)
    u, v = rng.uniform(20, 620, n), rng.uniform(20, 460, n)
    behind = np.arange(n - n_behind, n)
    z[behind] = -z[behind]
    pc = np.stack([(u - K["cx"]) / K["fx"] * z, (v - K["cy"]) / K["fy"] * z, z], 1)
    p3 = (pc @ Rwc.T + T[:3, 3]).astype(np.float32)
    Tcw = np.linalg.inv(T)
    q = p3.astype(np.float64) @ Tcw[:3, :3].T + Tcw[:3, 3]
    uv = np.stack([K["fx"] * q[:, 0] / q[:, 2] + K["cx"], K["fy"] * q[:, 1] / q[:, 2] + K["cy"]], 1)
    if noise:
        uv = uv + rng.normal(0.0, noise, uv.shape)
    idx_moved = np.arange(0, n - n_behind, moved_every) if moved_every else np.zeros(0, int)
    uv[idx_moved] += (40.0, -30.0)
    return p3, uv.astype(np.float32), T, idx_moved, behind


def stationary_scene():
    """Status 3 by construction: identity pose, fx = fy = 512, cx = 320, cy = 256, points with x / z and y / z multiples of 1/8
    and z a power of two: every projection is an integer-valued f32, every e is 0.0 in f64, so chi2 = 0 and b = 0, delta = 0,
    W = I: the trial state is the state and 0 < 0 never holds."""
    rng = np.random.RandomState(5)
    z = 2.0 ** rng.randint(0, 3, 40)
    p3 = np.stack([rng.randint(-4, 5, 40) / 8.0 * z, rng.randint(-3, 4, 40) / 8.0 * z, z], 1).astype(np.float32)
    Kd = dict(fx=512.0, fy=512.0, cx=320.0, cy=256.0)
    p2 = np.stack([512.0 * p3[:, 0] / p3[:, 2] + 320.0, 512.0 * p3[:, 1] / p3[:, 2] + 256.0], 1).astype(np.float32)
    return p3, p2, np.eye(4), Kd


def perturbed(T_w_c, angle_deg, shift):
    """T_w_c turned by angle_deg about a fixed axis and moved by `shift` (a 3-vector) in the world."""
    T = np.array(T_w_c, np.float64)
    T[:3, :3] = rotation([0.6, 0.5, -0.62], np.deg2rad(angle_deg)) @ T[:3, :3]
    T[:3, 3] += shift
    return T
