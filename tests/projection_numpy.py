"""TEST AID: tracking by projection transcribed to numpy from its declared arithmetic -- the LU pose
inverse, the projection of every map point with its in-view test, the inclusive disc gate, the two nearest gated frame
keypoints with the tie rule, the filter, and the constant-velocity pose prediction.  Vectorised f64 (numpy rounds every
elementwise product and sum on its own, which is the declared order), Python floats for the 4 x 4 algebra, integers for the
rest; it shares no code with the product (csrc/projection_kernels.hip, csrc/projection_host.cpp) and is what the MI355X and
the emulated build are compared with, bit for bit.  Its own known answers are in tests/test_projection_numpy.py.
tracking_scene() builds the scene those tests, the GPU tests and the host program share."""
import numpy as np

from epipolar_numpy import DMATCH, FR1_K, INT32_MAX, filter_matches, hamming, project, rodrigues  # noqa: F401


def invert_pose(T):
    """inv of a 4 x 4 by the partial-pivoting LU the library declares for poses (mvo_invert_pose); None if singular."""
    A = [[float(x) for x in row] for row in np.asarray(T, np.float64).reshape(4, 4)]
    B = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for i in range(4):
        piv = i
        for j in range(i + 1, 4):
            if abs(A[j][i]) > abs(A[piv][i]):
                piv = j
        if abs(A[piv][i]) < np.finfo(np.float64).eps * 100:
            return None
        if piv != i:
            A[i], A[piv] = A[piv], A[i]
            B[i], B[piv] = B[piv], B[i]
        d = -1 / A[i][i]
        for j in range(i + 1, 4):
            alpha = A[j][i] * d
            for c in range(i + 1, 4):
                A[j][c] += alpha * A[i][c]
            for c in range(4):
                B[j][c] += alpha * B[i][c]
    for i in range(3, -1, -1):
        for j in range(4):
            s = B[i][j]
            for c in range(i + 1, 4):
                s -= A[i][c] * B[c][j]
            B[i][j] = s / A[i][i]
    return np.array(B, np.float64)


def mul4(A, B):
    """4 x 4 product, each entry summed k = 0..3 in order from 0.0."""
    out = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            s = 0.0
            for k in range(4):
                s += float(A[i][k]) * float(B[k][j])
            out[i, j] = s
    return out


def predict_pose(T_prev2, T_prev):
    """T_prev * (inv(T_prev2) * T_prev); without a T_prev2 the prediction is T_prev."""
    T_prev = np.asarray(T_prev, np.float64).reshape(4, 4)
    if T_prev2 is None:
        return T_prev.copy()
    return mul4(T_prev, mul4(invert_pose(T_prev2), T_prev))


def project_map(pos, T_w_c, K, cols, rows):
    """-> u, v (f32) and in_view per map point: p_cam = (float)(T_c_w p) summed in double from 0.0 over k = 0..3,
    u = (float)(fx (double)pcx / (double)pcz + cx), in_view = !(pcz < 0) && 0 < u < cols && 0 < v < rows."""
    Ti = invert_pose(T_w_c)
    p = np.asarray(pos, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(all="ignore"):
        pc = []
        for r in range(3):
            acc = 0.0 + Ti[r, 0] * p[:, 0]
            acc = acc + Ti[r, 1] * p[:, 1]
            acc = acc + Ti[r, 2] * p[:, 2]
            acc = acc + Ti[r, 3] * 1.0
            pc.append(acc.astype(np.float32))
        pcx, pcy, pcz = pc
        u = (np.float64(K["fx"]) * pcx.astype(np.float64) / pcz.astype(np.float64) + np.float64(K["cx"])).astype(np.float32)
        v = (np.float64(K["fy"]) * pcy.astype(np.float64) / pcz.astype(np.float64) + np.float64(K["cy"])).astype(np.float32)
        in_view = ~(pcz < 0) & (u > 0) & (v > 0) & (u < np.float32(cols)) & (v < np.float32(rows))
    return u, v, in_view


def radii2(nt, max_px, t_scale=None):
    """r2[j] = rj rj with rj = max_px * (double)t_scale[j] (1 without scales)."""
    s = np.ones(nt) if t_scale is None else np.asarray(t_scale, np.float32).reshape(nt).astype(np.float64)
    r = np.float64(max_px) * s
    return r * r


def gate(u, v, in_view, txy, r2):
    """n_map x nt bool: keypoint j within its radius of point i's projection.  Inclusive; a NaN passes nothing."""
    t = np.asarray(txy, np.float32).reshape(-1, 2).astype(np.float64)
    with np.errstate(all="ignore"):
        du = t[:, 0][None, :] - u.astype(np.float64)[:, None]
        dv = t[:, 1][None, :] - v.astype(np.float64)[:, None]
        d2 = du * du + dv * dv
        return in_view[:, None] & (d2 <= np.asarray(r2, np.float64)[None, :])


def knn2(pos, desc, T_w_c, K, cols, rows, t, txy, max_px, t_scale=None, use_gate=True):
    """-> px n_map x 2 f32, idx n_map x 2, dist n_map x 2, n_candidates n_map.  In view: the two smallest distances among
    the passing keypoints, equal distances keep the lower train index first, a missing neighbour is (-1, INT32_MAX).  Not
    in view: px (0, 0), idx -1, dist INT32_MAX, n_candidates -1."""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    t = np.asarray(t, np.uint8).reshape(-1, 32)
    n, nt = len(desc), len(t)
    u, v, in_view = project_map(pos, T_w_c, K, cols, rows)
    px = np.where(in_view[:, None], np.stack([u, v], 1), np.float32(0)).astype(np.float32)
    idx = np.full((n, 2), -1, np.int32)
    dist = np.full((n, 2), INT32_MAX, np.int32)
    cnt = np.where(in_view, 0, -1).astype(np.int32)
    if n == 0 or nt == 0:
        return px, idx, dist, cnt
    ok = gate(u, v, in_view, txy, radii2(nt, max_px, t_scale)) if use_gate else np.repeat(in_view[:, None], nt, 1)
    d = np.where(ok, hamming(desc, t).astype(np.int64), 1 << 40)
    order = np.argsort(d, axis=1, kind="stable")[:, :2]      # stable: the lower index first among equal distances
    passing = ok.sum(1).astype(np.int32)
    cnt[in_view] = passing[in_view]
    for k in range(min(2, nt)):
        have = passing > k
        idx[have, k] = order[have, k]
        dist[have, k] = d[np.nonzero(have)[0], order[have, k]]
    return px, idx, dist, cnt


def match_features(pos, desc, T_w_c, K, cols, rows, t, txy, max_px, lowe_ratio, max_hamming, t_scale=None, use_gate=True):
    """The raw call and the filter of section 14 -> DMATCH sorted by trainIdx, queryIdx = map index."""
    _, idx, dist, _ = knn2(pos, desc, T_w_c, K, cols, rows, t, txy, max_px, t_scale, use_gate)
    return filter_matches(idx, dist, lowe_ratio, max_hamming)


def pose(rvec, t):
    T = np.eye(4)
    T[:3, :3] = rodrigues(rvec)
    T[:3, 3] = t
    return T


_scene = {}


def tracking_scene(seed=11, n_points=400, cols=640, rows=480, K=FR1_K, noise=0.3, partner_flips=20, twin_flips=8, twin_offset=40.0):
    """What the feature is for: a map seen by a frame that moved 0.3 m and 4 degrees from its keyframe (pose I).  Every
    seen point has in the frame its partner (partner_flips bits from the map descriptor, at the noisy true projection)
    and a TWIN, closer in descriptor space (twin_flips bits) but twin_offset px away.  A global search takes the twin
    every time; a disc around the keyframe-pose projection misses the partner or holds the twin as well; a small disc
    around the projection under a prediction of the pose holds the partner alone.
    -> dict(K, cols, rows, pos, desc (the map), T_key, T_true, T_pred, t, txy (the frame: partners and twins shuffled), seen
    (map indices), partner / twin (train index per seen point)).  Built once per argument set; callers must not write."""
    key = (seed, n_points, cols, rows, noise, partner_flips, twin_flips, twin_offset)
    if key in _scene:
        return _scene[key]
    rng = np.random.RandomState(seed)
    pos = rng.uniform([-2.4, -1.8, 2.1], [2.6, 1.8, 8.0], (n_points, 3)).astype(np.float32)
    jitter = rng.normal(0, noise, (n_points, 2))
    angle = rng.uniform(0, 2 * np.pi, n_points)
    bits = rng.randint(0, 2, (n_points, 256)).astype(np.uint8)

    def flipped(k):
        out = bits.copy()
        for i in range(n_points):
            out[i, rng.permutation(256)[:k]] ^= 1
        return np.packbits(out, axis=1)

    dp, dt = flipped(partner_flips), flipped(twin_flips)
    rv, tv = np.array([0.03, -0.06, 0.02]), np.array([0.30, 0.04, 0.08])
    T_true = pose(rv, tv)
    T_pred = pose(rv + [0.002, -0.0015, 0.001], tv + [0.010, -0.005, 0.008])
    p, z = project(T_true, K, pos.astype(np.float64))
    seen = np.nonzero((z > 0) & (p[:, 0] >= 8) & (p[:, 0] < cols - 8) & (p[:, 1] >= 8) & (p[:, 1] < rows - 8))[0]
    n = len(seen)
    xyp = (p[seen] + jitter[seen]).astype(np.float32)
    xyt = (xyp.astype(np.float64) + twin_offset * np.stack([np.cos(angle[seen]), np.sin(angle[seen])], 1)).astype(np.float32)
    perm = rng.permutation(2 * n)
    inv = np.argsort(perm)
    s = dict(K=K, cols=cols, rows=rows, pos=pos, desc=np.packbits(bits, axis=1), T_key=np.eye(4), T_true=T_true, T_pred=T_pred,
             t=np.concatenate([dp[seen], dt[seen]])[perm], txy=np.concatenate([xyp, xyt])[perm], seen=seen.astype(np.int32),
             partner=inv[:n].astype(np.int32), twin=inv[n:].astype(np.int32))
    for a in s.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _scene[key] = s
    return s


def scene_score(s, matches):
    """(number of matches, how many of them join a seen point with its true partner, how many with its twin)."""
    partner = np.full(len(s["pos"]), -2, np.int64)
    twin = np.full(len(s["pos"]), -2, np.int64)
    partner[s["seen"]], twin[s["seen"]] = s["partner"], s["twin"]
    q, t = matches["queryIdx"], matches["trainIdx"]
    return len(matches), int((partner[q] == t).sum()), int((twin[q] == t).sum())
