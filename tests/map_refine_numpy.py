"""Numpy transcription of the map-point position refinement (include/mvo_hip.h: mvo_map_refine_positions),
written from the declared arithmetic and sharing no code with the product: every map point's position re-estimated from all
its observations with the poses fixed -- a 3-unknown Huber-weighted Levenberg-Marquardt per point.  f64 throughout; per
observation the operations are numpy elementwise operations (each rounded on its own, which is the declared order), every sum
over the observations runs from 0.0 in observation order (np.add.accumulate is sequential), the 3 x 3 algebra is numpy scalars
in the written order.  Known answers: tests/test_map_refine_numpy.py."""
import numpy as np

from projection_numpy import invert_pose

MAX_OBS, MAX_FRAMES = 64, 64
DEFAULTS = dict(max_trials=20, min_observations=2, huber_delta=float(np.sqrt(np.float64(5.991))), rel_tolerance=1e-6)
REFINED, TOO_FEW, BEHIND, NO_STEP = 0, 1, 2, 3


def ordered_sum(terms):
    """0.0 + t_0 + t_1 + ... in this order."""
    return np.add.accumulate(np.concatenate([np.zeros(1), np.asarray(terms, np.float64)]))[-1]


def evaluate(p, Tcw, uv, K, delta):
    """The m observations of one point at the f64 position p.  Tcw: m x 3 x 4 (rows 0..2 of T_c_w of each observation's
    frame), uv: m x 2 f32.  -> (H six entries 00 01 02 11 12 22, b, chi2, e2 per observation, in_front per observation)."""
    fx, fy, cx, cy = (np.float64(K[k]) for k in ("fx", "fy", "cx", "cy"))
    d = np.float64(delta)
    R, t = Tcw[:, :, :3], Tcw[:, :, 3]
    with np.errstate(all="ignore"):
        q = [((R[:, r, 0] * p[0] + R[:, r, 1] * p[1]) + R[:, r, 2] * p[2]) + t[:, r] for r in range(3)]
        ax, ay = fx * q[0], fy * q[1]
        ex = (ax / q[2] + cx) - uv[:, 0].astype(np.float64)
        ey = (ay / q[2] + cy) - uv[:, 1].astype(np.float64)
        e2 = ex * ex + ey * ey
        d2 = d * d
        s = np.sqrt(e2)
        inl = e2 <= d2
        rho = np.where(inl, e2, (np.float64(2.0) * d) * s - d2)
        w = np.where(inl, np.float64(1.0), d / s)
        zz = q[2] * q[2]
        a0, a2 = fx / q[2], -(ax / zz)
        b1, b2 = fy / q[2], -(ay / zz)
        J0 = [a0 * R[:, 0, c] + a2 * R[:, 2, c] for c in range(3)]
        J1 = [b1 * R[:, 1, c] + b2 * R[:, 2, c] for c in range(3)]
        H = [ordered_sum(w * (J0[c] * J0[e] + J1[c] * J1[e])) for c, e in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
        b = [ordered_sum(w * (J0[c] * ex + J1[c] * ey)) for c in range(3)]
        chi2 = ordered_sum(rho)
    return H, b, chi2, e2, q[2] > 0


def solve(H, b, lam):
    """(H + lam I) d = -b by 3 x 3 Cholesky; None when a pivot is not positive."""
    h00, h01, h02, h11, h12, h22 = H
    with np.errstate(all="ignore"):
        a00 = h00 + lam
        if not a00 > 0:
            return None
        l00 = np.sqrt(a00)
        l10 = h01 / l00
        l20 = h02 / l00
        p1 = (h11 + lam) - l10 * l10
        if not p1 > 0:
            return None
        l11 = np.sqrt(p1)
        l21 = (h12 - l20 * l10) / l11
        p2 = ((h22 + lam) - l20 * l20) - l21 * l21
        if not p2 > 0:
            return None
        l22 = np.sqrt(p2)
        y0 = (-b[0]) / l00
        y1 = ((-b[1]) - l10 * y0) / l11
        y2 = (((-b[2]) - l20 * y0) - l21 * y1) / l22
        d2 = y2 / l22
        d1 = (y1 - l21 * d2) / l11
        d0 = ((y0 - l10 * d1) - l20 * d2) / l00
    return [d0, d1, d2]


def refine_point(pos_f32, Tcw, uv, K, params=None, trace=None):
    """One point with m >= min_observations observations -> (status, p f64 x 3, chi2 before, chi2 after, accepted steps,
    trials, outlier flags m).  trace (a list) receives one bool per trial: accepted or not."""
    P = dict(DEFAULTS, **(params or {}))
    m = len(uv)
    p = [np.float64(np.float32(v)) for v in pos_f32]
    none = np.zeros(m, np.uint8)
    H, b, chi2, e2, front = evaluate(p, Tcw, uv, K, P["huber_delta"])
    if not front.all():
        return BEHIND, p, np.float64(0.0), np.float64(0.0), 0, 0, none
    chi2_0 = chi2
    d2 = np.float64(P["huber_delta"]) * np.float64(P["huber_delta"])
    mx = H[0]
    if H[3] > mx:
        mx = H[3]
    if H[5] > mx:
        mx = H[5]
    lam = np.float64(1e-3) * mx
    steps = trials = 0
    if lam > 0 and lam < np.inf:
        while trials < P["max_trials"]:
            trials += 1
            d = solve(H, b, lam)
            accepted = False
            if d is not None:
                p_new = [p[r] + d[r] for r in range(3)]
                H_n, b_n, chi2_n, e2_n, front_n = evaluate(p_new, Tcw, uv, K, P["huber_delta"])
                accepted = bool(front_n.all() and chi2_n < chi2)
            if trace is not None:
                trace.append(accepted)
            if accepted:
                dec = chi2 - chi2_n
                tol = np.float64(P["rel_tolerance"]) * chi2
                p, H, b, chi2, e2 = p_new, H_n, b_n, chi2_n, e2_n
                steps += 1
                lam = lam * np.float64(0.1)
                if dec <= tol:
                    break
            else:
                lam = lam * np.float64(10.0)
    return (REFINED if steps else NO_STEP), p, chi2_0, chi2, steps, trials, (e2 > d2).astype(np.uint8)


def refine(pos, T_w_c, K, obs_frame, obs_uv, obs_start, params=None, traces=None):
    """-> (pos n x 3 f32 after the call, chi2 n x 2 f64, info n x 3 int32: status, accepted steps, trials; outlier n_obs u8).
    Only status 0 rewrites a position.  traces (a dict) receives the accept / reject sequence of every point that ran trials."""
    P = dict(DEFAULTS, **(params or {}))
    out_pos = np.array(pos, np.float32).reshape(-1, 3)
    T_w_c = np.asarray(T_w_c, np.float64).reshape(-1, 4, 4)
    obs_frame = np.asarray(obs_frame, np.int32).reshape(-1)
    obs_uv = np.asarray(obs_uv, np.float32).reshape(-1, 2)
    n = len(out_pos)
    assert len(T_w_c) <= MAX_FRAMES and len(obs_start) == n + 1 and obs_start[0] == 0 and obs_start[n] == len(obs_uv) == len(obs_frame)
    Tcw = np.array([invert_pose(T)[:3] for T in T_w_c], np.float64).reshape(-1, 3, 4)
    chi2, info, outlier = np.zeros((n, 2), np.float64), np.zeros((n, 3), np.int32), np.zeros(len(obs_uv), np.uint8)
    for i in range(n):
        a, e = int(obs_start[i]), int(obs_start[i + 1])
        assert 0 <= e - a <= MAX_OBS
        if e - a < P["min_observations"]:
            info[i, 0] = TOO_FEW
            continue
        trace = []
        status, p, c0, c1, steps, trials, flags = refine_point(out_pos[i], Tcw[obs_frame[a:e]], obs_uv[a:e], K, P, trace)
        if traces is not None:
            traces[i] = trace
        info[i] = (status, steps, trials)
        chi2[i] = (c0, c1)
        outlier[a:e] = flags
        if status == REFINED:
            out_pos[i] = np.array(p, np.float64).astype(np.float32)
    return out_pos, chi2, info, outlier


# ---- the scene of the CPU check of the rule and of the device tests

FR1_K = dict(fx=517.3, fy=516.5, cx=325.1, cy=249.7)


def camera(j, step=0.03, yaw=0.01):
    """T_w_c of camera j: j * step along x, j * yaw about y."""
    c, s = np.cos(j * yaw), np.sin(j * yaw)
    T = np.eye(4)
    T[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    T[0, 3] = j * step
    return T


def project_f64(p, T_w_c, K):
    q = np.linalg.inv(T_w_c) @ np.r_[p, 1.0]
    return np.array([K["fx"] * q[0] / q[2] + K["cx"], K["fy"] * q[1] / q[2] + K["cy"]]), q[2]


def scene(rng, counts, n_frames=20, noise=0.0, moved_every=0, off=0.03, K=FR1_K, step=0.03, yaw=0.01):
    """n points at depths 0.5 .. 1.5 in front of `n_frames` cameras, `step` apart and each with `yaw` more yaw; point i is seen by counts[i] observations in frames
    drawn in ascending order (with repetition when counts[i] > n_frames); pixels are the f32 rounding of the projection plus
    `noise` px of Gaussian noise; every `moved_every`-th point (with 3 observations or more) has one observation moved by
    (40, -30) px; the start positions are `off` (relative) away from the truth.
    -> truth n x 3 f64, pos n x 3 f32, T_w_c, obs_frame, obs_uv f32, obs_start, moved (index of the moved observation or -1)."""
    n = len(counts)
    T = np.stack([camera(j, step, yaw) for j in range(n_frames)])
    z = rng.uniform(0.5, 1.5, n)
    mid = step * (n_frames - 1) / 2
    truth = np.stack([mid + rng.uniform(-0.3, 0.3, n) * z, rng.uniform(-0.25, 0.25, n) * z, z], 1)
    frames, uv, start, moved = [], [], [0], np.full(n, -1, np.int64)
    for i, m in enumerate(counts):
        fr = np.sort(rng.choice(n_frames, m, replace=m > n_frames)) if m else np.zeros(0, np.int64)
        for f in fr:
            px, depth = project_f64(truth[i], T[f], K)
            assert depth > 0.2
            uv.append(px + noise * rng.normal(size=2))
        if moved_every and i % moved_every == moved_every - 1 and m >= 3:
            k = int(rng.randint(m))
            uv[start[-1] + k] = uv[start[-1] + k] + np.array([40.0, -30.0])
            moved[i] = start[-1] + k
        frames += list(fr)
        start.append(start[-1] + m)
    direction = rng.normal(size=(n, 3))
    direction /= np.linalg.norm(direction, axis=1)[:, None]
    pos = (truth + off * z[:, None] * direction).astype(np.float32)
    return (truth, pos, T, np.array(frames, np.int32), np.array(uv, np.float64).reshape(-1, 2).astype(np.float32),
            np.array(start, np.int32), moved)


def failed_then_accepted(trace):
    return any((not a) and b for a, b in zip(trace, trace[1:]))
