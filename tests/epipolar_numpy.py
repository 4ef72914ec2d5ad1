"""TEST AID: the pose-guided matcher transcribed to numpy from its declared arithmetic -- the epipolar
line of every query, the inclusive gate, 256-bit Hamming distances via unpackbits, the two nearest gated trains with the
tie rule, the ceiling / ratio filter, one query per train, and F from two poses.  Vectorised f64 (numpy rounds every
elementwise product and sum on its own, which is the declared order) and integers; it shares no code with the product
(csrc/epipolar_kernels.hip, csrc/epipolar_host.cpp) and is what the MI355X and the emulated build are compared with, bit
for bit.  Its own known answers are in tests/test_epipolar_numpy.py.  two_view_scene() builds the scene those tests, the
GPU tests and the host program share."""
import numpy as np

FR1_K = dict(fx=517.3, fy=516.5, cx=325.1, cy=249.7)                  # TUM fr1
INT32_MAX = np.iinfo(np.int32).max
DMATCH = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])


def lines(F, qxy):
    """a, b, c, nrm per query: a = (F0 x + F1 y) + F2 ... nrm = a a + b b, every operation rounded to f64."""
    F = np.asarray(F, np.float64).reshape(9)
    p = np.asarray(qxy, np.float32).reshape(-1, 2).astype(np.float64)
    x, y = p[:, 0], p[:, 1]
    a = (F[0] * x + F[1] * y) + F[2]
    b = (F[3] * x + F[4] * y) + F[5]
    c = (F[6] * x + F[7] * y) + F[8]
    return a, b, c, a * a + b * b


def tolerances(nt, max_line_px, t_scale=None):
    """tol2[j] = tl tl with tl = max_line_px * (double)t_scale[j] (1 without scales)."""
    s = np.ones(nt) if t_scale is None else np.asarray(t_scale, np.float32).reshape(nt).astype(np.float64)
    tl = np.float64(max_line_px) * s
    return tl * tl


def gate(F, qxy, txy, tol2):
    """nq x nt bool: train j within its tolerance of query i's line.  Inclusive; NaN and nrm == 0 pass nothing."""
    a, b, c, nrm = lines(F, qxy)
    t = np.asarray(txy, np.float32).reshape(-1, 2).astype(np.float64)
    u, v = t[:, 0][None, :], t[:, 1][None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        num = (a[:, None] * u + b[:, None] * v) + c[:, None]
        return (nrm[:, None] > 0) & (num * num <= np.asarray(tol2, np.float64)[None, :] * nrm[:, None])


def hamming(q, t):
    """nq x nt int32 Hamming distances of 32-byte descriptors."""
    qb = np.unpackbits(np.asarray(q, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    tb = np.unpackbits(np.asarray(t, np.uint8).reshape(-1, 32), axis=1).astype(np.float32)
    # differing bits = q (1 - t) + (1 - q) t; sums of at most 256 ones are exact in f32
    return (qb @ (1 - tb).T + (1 - qb) @ tb.T).astype(np.int32)


def knn2(q, qxy, t, txy, F, max_line_px, t_scale=None, use_gate=True):
    """-> idx nq x 2, dist nq x 2, n_candidates nq: the two smallest distances among the passing trains, equal distances
    keep the lower train index first; a missing neighbour is (-1, INT32_MAX)."""
    q = np.asarray(q, np.uint8).reshape(-1, 32)
    t = np.asarray(t, np.uint8).reshape(-1, 32)
    nq, nt = len(q), len(t)
    idx = np.full((nq, 2), -1, np.int32)
    dist = np.full((nq, 2), INT32_MAX, np.int32)
    cnt = np.zeros(nq, np.int32)
    if nq == 0 or nt == 0:
        return idx, dist, cnt
    ok = gate(F, qxy, txy, tolerances(nt, max_line_px, t_scale)) if use_gate else np.ones((nq, nt), bool)
    d = np.where(ok, hamming(q, t).astype(np.int64), 1 << 40)
    order = np.argsort(d, axis=1, kind="stable")[:, :2]     # stable: the lower index first among equal distances
    cnt[:] = ok.sum(1)
    for k in range(min(2, nt)):
        have = cnt > k
        idx[have, k] = order[have, k]
        dist[have, k] = d[np.nonzero(have)[0], order[have, k]]
    return idx, dist, cnt


def filter_matches(idx, dist, lowe_ratio, max_hamming):
    """Ceiling and ratio, then one query per train (smallest distance, then lower queryIdx), sorted by trainIdx."""
    best = {}
    for i in range(len(idx)):
        j, d0 = int(idx[i, 0]), int(dist[i, 0])
        if j < 0 or d0 > max_hamming:
            continue
        if idx[i, 1] >= 0 and not (float(d0) < float(lowe_ratio) * float(dist[i, 1])):
            continue
        if j not in best or (d0, i) < best[j]:
            best[j] = (d0, i)
    out = np.zeros(len(best), DMATCH)
    for k, j in enumerate(sorted(best)):
        out[k] = (best[j][1], j, 0, np.float32(best[j][0]))
    return out


def match_features(d1, xy1, d2, xy2, F, max_line_px, lowe_ratio, max_hamming, scale2=None, use_gate=True):
    idx, dist, _ = knn2(d1, xy1, d2, xy2, F, max_line_px, scale2, use_gate)
    return filter_matches(idx, dist, lowe_ratio, max_hamming)


def rodrigues(rvec):
    r = np.asarray(rvec, np.float64)
    th = np.linalg.norm(r)
    if th == 0:
        return np.eye(3)
    k = r / th
    S = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * S + (1 - np.cos(th)) * S @ S


def fundamental_from_poses(T_w_c_1, T_w_c_2, K):
    """F with x2^T F x1 = 0: T_2_1 = inv(T_w_c_2) T_w_c_1, E = [t]x R, F = K^-T E K^-1."""
    T = np.linalg.inv(np.asarray(T_w_c_2, np.float64).reshape(4, 4)) @ np.asarray(T_w_c_1, np.float64).reshape(4, 4)
    R, t = T[:3, :3], T[:3, 3]
    S = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(np.array([[K["fx"], 0, K["cx"]], [0, K["fy"], K["cy"]], [0, 0, 1.0]]))
    return Ki.T @ (S @ R) @ Ki


def project(T_w_c, K, X):
    """Pixels and depths of world points X (n x 3) in the camera with pose T_w_c."""
    T = np.linalg.inv(np.asarray(T_w_c, np.float64).reshape(4, 4))
    Xc = X @ T[:3, :3].T + T[:3, 3]
    return np.stack([K["fx"] * Xc[:, 0] / Xc[:, 2] + K["cx"], K["fy"] * Xc[:, 1] / Xc[:, 2] + K["cy"]], 1), Xc[:, 2]


def line_distance(F, xy1, xy2):
    """Distance in px of xy2[i] from the epipolar line of xy1[i] (a diagnostic, not the gate)."""
    a, b, c, nrm = lines(F, xy1)
    p = np.asarray(xy2, np.float64)
    return np.abs(a * p[:, 0] + b * p[:, 1] + c) / np.sqrt(nrm)


_scene = {}


def two_view_scene(seed=11, n_points=300, width=640, height=480, K=FR1_K, noise=0.3, partner_flips=20, twin_flips=8,
                   twin_offset=40.0):
    """What the feature is for: points seen by two cameras with known poses; in view 2 every point has its partner
    (partner_flips bits away) and a TWIN, closer in descriptor space (twin_flips bits) but twin_offset px off the point's
    epipolar line.  A global nearest-neighbour search takes the twin every time; the gated one cannot see it.
    -> dict(T1, T2, F, K, d1, xy1 (queries), d2, xy2 (trains: partners and twins shuffled), partner (train index of the
    true partner per query), twin).  Built once per argument set; callers must not write to it."""
    key = (seed, n_points, width, height, noise, partner_flips, twin_flips, twin_offset)
    if key in _scene:
        return _scene[key]
    rng = np.random.RandomState(seed)
    X = rng.uniform([-2.0, -1.5, 2.1], [2.0, 1.5, 8.0], (n_points, 3))  # 280 of the 300 land in both views
    T1 = np.eye(4)
    T2 = np.eye(4)
    T2[:3, :3] = rodrigues([0.02, -0.05, 0.03])
    T2[:3, 3] = [0.25, 0.03, 0.05]
    p1, z1 = project(T1, K, X)
    p2, z2 = project(T2, K, X)
    inside = (z1 > 0) & (z2 > 0)
    for p in (p1, p2):
        inside &= (p[:, 0] >= 0) & (p[:, 0] < width) & (p[:, 1] >= 0) & (p[:, 1] < height)
    p1, p2 = p1[inside], p2[inside]
    n = len(p1)
    xy1 = (p1 + rng.normal(0, noise, p1.shape)).astype(np.float32)
    xyp = (p2 + rng.normal(0, noise, p2.shape)).astype(np.float32)
    F = fundamental_from_poses(T1, T2, K)
    a, b, _, nrm = lines(F, xy1)
    normal = np.stack([a, b], 1) / np.sqrt(nrm)[:, None]
    xyt = (xyp.astype(np.float64) + twin_offset * normal).astype(np.float32)
    bits = rng.randint(0, 2, (n, 256)).astype(np.uint8)

    def flipped(k):
        out = bits.copy()
        for i in range(n):
            out[i, rng.permutation(256)[:k]] ^= 1
        return np.packbits(out, axis=1)

    d1 = np.packbits(bits, axis=1)
    dp, dt = flipped(partner_flips), flipped(twin_flips)
    perm = rng.permutation(2 * n)
    inv = np.argsort(perm)
    s = dict(T1=T1, T2=T2, F=F, K=K, d1=d1, xy1=xy1, d2=np.concatenate([dp, dt])[perm], xy2=np.concatenate([xyp, xyt])[perm],
             partner=inv[:n].astype(np.int32), twin=inv[n:].astype(np.int32))
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _scene[key] = s
    return s
