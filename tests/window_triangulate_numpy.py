"""TEST AID: the triangulation of new map points against every buffered frame transcribed to numpy and plain
Python from its declared rule -- the relative pose and the fundamental matrix of every frame, the baseline test, the search of
every free keypoint of the new keyframe along its epipolar line among the free keypoints of every frame (the line and the
inclusive gate of section 14), the filter with one query per train, the verification of every pair (depths, parallax, the two
reprojection errors, the scale consistency), the choice.  Vectorised f64 (numpy rounds every elementwise product and sum on its
own, which is the declared order), Python floats for the 4 x 4 and 3 x 3 algebra, integers for the rest.  The triangulation itself
(the DLT of helperTriangulatePoints) is the CPU oracle's, which mvo_triangulate_points is held to bit for bit elsewhere
(tests/test_gpu_keyframe.py).  It shares no code with the product (csrc/window_triangulate_kernels.hip,
csrc/window_triangulate_host.cpp) and is what the MI355X and the emulated build are compared with, bit for bit.  Its own known
answers are in tests/test_window_triangulate_numpy.py.  scene() builds the synthetic scene those tests, the GPU tests and the host
program share.

A frame (and the new keyframe, curr) is a dict: desc (n x 32 uint8), xy (n x 2 f32), scale (n f32 or None), conn (n int32: -1
free, anything else not free), T (4 x 4, camera to world)."""
import numpy as np

import epipolar_numpy as E
from epipolar_numpy import FR1_K, INT32_MAX  # noqa: F401
from projection_numpy import invert_pose, mul4

DEFAULTS = dict(max_line_px=2.0, lowe_ratio=0.8, max_hamming=64, max_cos_parallax=0.9998, max_reproj_chi2=5.991, ratio_factor=1.8,
                min_baseline=0.0)
PAIR = np.dtype([("frame", np.int32), ("keypoint", np.int32), ("train", np.int32), ("hamming", np.int32), ("status", np.int32),
                 ("p_curr", np.float32, 3), ("p_frame", np.float32, 3), ("cos2", np.float64)])
POINT = np.dtype([("keypoint", np.int32), ("frame", np.int32), ("train", np.int32), ("hamming", np.int32), ("p_curr", np.float32, 3),
                  ("cos2", np.float64)])
NOT_FINITE, DEPTH, PARALLAX, REPROJ_FRAME, REPROJ_CURR, SCALE = 1, 2, 4, 8, 16, 32

_oracle = []


def oracle():
    """The CPU oracle (oracle/oracle_py.py), built on first use."""
    if not _oracle:
        import __graft_entry__ as graft
        o = graft.load_oracle()
        o.build()
        _oracle.append(o)
    return _oracle[0]


def _mul3(A, B):
    """3 x 3 product of nested lists, each entry summed k = 0..2 in order from 0.0."""
    out = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            s = 0.0
            for k in range(3):
                s += A[i][k] * B[k][j]
            out[i][j] = s
    return out


def fundamental(T_w_c_1, T_w_c_2, K):
    """mvo_fundamental_from_poses as declared in section 14, operation by operation: T = inv(T2) T1 (LU inverse, product summed
    k = 0..3), E = [t]x R, M = E K^-1, F = K^-T M with K^-1 = [[1/fx, 0, -cx/fx], [0, 1/fy, -cy/fy], [0, 0, 1]].  None if a pose
    is singular or F is not finite."""
    T1 = np.asarray(T_w_c_1, np.float64).reshape(4, 4)
    if invert_pose(T1) is None:
        return None
    Ti2 = invert_pose(T_w_c_2)
    if Ti2 is None:
        return None
    T = mul4(Ti2, T1)
    tx, ty, tz = float(T[0, 3]), float(T[1, 3]), float(T[2, 3])
    S = [[0.0, -tz, ty], [tz, 0.0, -tx], [-ty, tx, 0.0]]
    fx, fy, cx, cy = (float(K[k]) for k in ("fx", "fy", "cx", "cy"))
    Ki = [[1 / fx, 0.0, -cx / fx], [0.0, 1 / fy, -cy / fy], [0.0, 0.0, 1.0]]
    Em = _mul3(S, [[float(T[i, j]) for j in range(3)] for i in range(3)])
    M = _mul3(Em, Ki)
    F = np.array(_mul3([[Ki[k][i] for k in range(3)] for i in range(3)], M), np.float64)
    return F if np.isfinite(F).all() else None


def relative(curr, frame, min_baseline):
    """-> R (3 x 3), t (3), active: M = inv(T_w_c_curr) T_w_c_f; b2 = (tx tx + ty ty) + tz tz; active = b2 > 0 and
    b2 >= min_baseline min_baseline."""
    M = mul4(invert_pose(curr["T"]), np.asarray(frame["T"], np.float64).reshape(4, 4))
    t = M[:3, 3].copy()
    b2 = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]
    return M[:3, :3].copy(), t, bool(b2 > 0 and b2 >= np.float64(min_baseline) * np.float64(min_baseline))


def _free(fr):
    return np.asarray(fr["conn"], np.int32).reshape(-1) == -1


def search(curr, frames, K, max_line_px=2.0, min_baseline=0.0):
    """-> idx F x n x 2, dist F x n x 2, n_candidates F x n: per frame the rows of section 14's raw call with F_f, with
    active = free and frame active and nrm > 0 in the place of nrm > 0, and tol2 = -1.0 for a keypoint of the frame that is not
    free.  Not active: idx -1, dist INT32_MAX, n_candidates -1."""
    q = np.asarray(curr["desc"], np.uint8).reshape(-1, 32)
    n, F = len(q), len(frames)
    idx = np.full((F, n, 2), -1, np.int32)
    dist = np.full((F, n, 2), INT32_MAX, np.int32)
    cnt = np.full((F, n), -1, np.int32)
    if n == 0:
        return idx, dist, cnt
    free_c = _free(curr)
    for f, fr in enumerate(frames):
        t = np.asarray(fr["desc"], np.uint8).reshape(-1, 32)
        nt = len(t)
        Ff = fundamental(curr["T"], fr["T"], K)
        _, _, frame_active = relative(curr, fr, min_baseline)
        with np.errstate(all="ignore"):
            nrm = E.lines(Ff, curr["xy"])[3]
            active = free_c & frame_active & (nrm > 0)
        cnt[f] = np.where(active, 0, -1)
        if nt == 0:
            continue
        tol2 = np.where(_free(fr), E.tolerances(nt, max_line_px, fr.get("scale")), -1.0)
        ok = E.gate(Ff, curr["xy"], fr["xy"], tol2) & active[:, None]
        d = np.where(ok, E.hamming(q, t).astype(np.int64), 1 << 40)
        order = np.argsort(d, axis=1, kind="stable")[:, :2]      # stable: the lower keypoint first among equal distances
        passing = ok.sum(1).astype(np.int32)
        cnt[f][active] = passing[active]
        for k in range(min(2, nt)):
            have = passing > k
            idx[f][have, k] = order[have, k]
            dist[f][have, k] = d[np.nonzero(have)[0], order[have, k]]
    return idx, dist, cnt


def filter_pairs(idx, dist, lowe_ratio, max_hamming):
    """Per frame section 14's filter (ceiling, ratio, one query per train: smallest distance, then the lower keypoint) ->
    rows (f, i, j, d) ordered by (f, j)."""
    out = []
    for f in range(len(idx)):
        for m in E.filter_matches(idx[f], dist[f], lowe_ratio, max_hamming):
            out.append((f, int(m["queryIdx"]), int(m["trainIdx"]), int(m["distance"])))
    return np.array(out, np.int32).reshape(-1, 4)


def _sum3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _reproj2(K, p, uv):
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    eu = ((np.float64(K["fx"]) * x) / z + np.float64(K["cx"])) - uv[:, 0].astype(np.float64)
    ev = ((np.float64(K["fy"]) * y) / z + np.float64(K["cy"])) - uv[:, 1].astype(np.float64)
    return eu * eu + ev * ev


def _scales(fr, rows):
    s = fr.get("scale")
    return np.ones(len(rows)) if s is None else np.asarray(s, np.float32).reshape(-1)[rows].astype(np.float64)


def verify(curr, frames, K, rows, max_cos_parallax=0.9998, max_reproj_chi2=5.991, ratio_factor=1.8, min_baseline=0.0,
           triangulate=None):
    """rows: (f, i, j, d) -> PAIR records in the same order.  triangulate(kp1, kp2, K, R, t) -> (points in camera 1, points in
    camera 2): the oracle's by default."""
    triangulate = triangulate or oracle().triangulate_points
    out = np.zeros(len(rows), PAIR)
    out["frame"], out["keypoint"], out["train"], out["hamming"] = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
    c2max = np.float64(max_cos_parallax) * np.float64(max_cos_parallax)
    rf2 = np.float64(ratio_factor) * np.float64(ratio_factor)
    chi2 = np.float64(max_reproj_chi2)
    xy_c = np.asarray(curr["xy"], np.float32).reshape(-1, 2)
    for f in sorted(set(rows[:, 0].tolist())):
        sel = np.nonzero(rows[:, 0] == f)[0]
        i, j = rows[sel, 1], rows[sel, 2]
        fr = frames[f]
        xy_f = np.asarray(fr["xy"], np.float32).reshape(-1, 2)
        R, t, _ = relative(curr, fr, min_baseline)
        p_f, p_c = triangulate(xy_f[j], xy_c[i], K, R, t)
        with np.errstate(all="ignore"):
            status = np.zeros(len(sel), np.int32)
            status |= np.where(np.isfinite(p_f).all(1) & np.isfinite(p_c).all(1), 0, NOT_FINITE).astype(np.int32)
            status |= np.where((p_f[:, 2] > 0) & (p_c[:, 2] > 0), 0, DEPTH).astype(np.int32)
            v1 = p_c.astype(np.float64)
            v2 = v1 - t[None, :]
            dot, n1, n2 = _sum3(v1, v2), _sum3(v1, v1), _sum3(v2, v2)
            cos2 = (dot * dot) / (n1 * n2)
            status |= np.where((dot > 0) & (cos2 < c2max), 0, PARALLAX).astype(np.int32)
            s_f, s_c = _scales(fr, j), _scales(curr, i)
            sf2, sc2 = s_f * s_f, s_c * s_c
            status |= np.where(_reproj2(K, p_f, xy_f[j]) <= chi2 * sf2, 0, REPROJ_FRAME).astype(np.int32)
            status |= np.where(_reproj2(K, p_c, xy_c[i]) <= chi2 * sc2, 0, REPROJ_CURR).astype(np.int32)
            pf64 = p_f.astype(np.float64)
            a, b = _sum3(pf64, pf64) * sf2, n1 * sc2
            status |= np.where((a * rf2 >= b) & (a <= b * rf2), 0, SCALE).astype(np.int32)
        out["status"][sel], out["cos2"][sel], out["p_curr"][sel], out["p_frame"][sel] = status, cos2, p_c, p_f
    return out


def choose(pairs):
    """Per keypoint among the pairs with status 0 the smallest cos2, then the lower frame -> POINT records sorted by keypoint."""
    best = {}
    for k in range(len(pairs)):
        p = pairs[k]
        if p["status"] != 0:
            continue
        i = int(p["keypoint"])
        if i not in best or (float(p["cos2"]), int(p["frame"])) < (float(pairs[best[i]]["cos2"]), int(pairs[best[i]]["frame"])):
            best[i] = k
    out = np.zeros(len(best), POINT)
    for r, i in enumerate(sorted(best)):
        p = pairs[best[i]]
        out[r] = (i, p["frame"], p["train"], p["hamming"], p["p_curr"], p["cos2"])
    return out


def window_triangulate(curr, frames, K, triangulate=None, **params):
    """-> points (POINT), pairs (PAIR), counts (12 int32: free keypoints of curr, active frames, rows with idx0 >= 0, pairs after
    the filter, pairs failing bit 1, 2, 4, 8, 16, 32, accepted pairs, new points), raw (idx, dist, n_candidates)."""
    P = dict(DEFAULTS, **params)
    raw = search(curr, frames, K, P["max_line_px"], P["min_baseline"])
    rows = filter_pairs(raw[0], raw[1], P["lowe_ratio"], P["max_hamming"])
    pairs = verify(curr, frames, K, rows, P["max_cos_parallax"], P["max_reproj_chi2"], P["ratio_factor"], P["min_baseline"], triangulate)
    points = choose(pairs)
    counts = np.array([int(_free(curr).sum()), sum(relative(curr, fr, P["min_baseline"])[2] for fr in frames), int((raw[0][:, :, 0] >= 0).sum()),
                       len(pairs)] + [int(((pairs["status"] >> b) & 1).sum()) for b in range(6)]
                      + [int((pairs["status"] == 0).sum()), len(points)], np.int32)
    return points, pairs, counts, raw


def camera(x, yaw=0.0):
    """A camera at (x, 0, 0) looking down +z, turned by yaw about y (camera to world)."""
    T = np.eye(4)
    T[:3, :3] = E.rodrigues([0.0, yaw, 0.0])
    T[0, 3] = x
    return T


def scene(rng, n_curr, kp_counts, K=FR1_K, cols=640, rows=480, step=0.083, yaw=0.004, noise=0.5, flips=15, scales=False,
          still=(), depth=(2.0, 6.0), twins=True, mirror=True, busy=True, block=0):
    """The new keyframe curr (n_curr keypoints) and len(kp_counts) older frames, oldest first: cameras in a row, `step` apart and
    turned by `yaw` each, curr the last; the frames listed in `still` stand where curr stands (zero baseline).  Three quarters of
    the keypoints of curr are noisy projections (noise px a coordinate) of points at depth depth[0] .. depth[1], the rest
    distractors at random pixels with random descriptors; with twins, every eighth real keypoint is a copy of its neighbour's pixel
    with the same point's descriptor (two keypoints that claim the same partners).  A frame holds, for the points of curr it sees,
    their noisy projections (descriptor: the point's with `flips` bits flipped, as in curr), every ninth of them MIRRORED through
    the centre of curr (the pixel on the far side of the epipole: a pair that triangulates behind both cameras), and distractors,
    a quarter of its keypoints at least.  With busy, a fifth of the keypoints of curr and a seventh of every frame's are not free; the first `block` keypoints of curr are
    not free either.  (With yaw 0 the relative translation of a still frame is exactly zero.)
    -> dict(curr, frames, point_c (the point of each keypoint of curr, -1 a distractor), point_f (per frame; mirrored: -2 - point),
    X)."""
    F = len(kp_counts)
    T_c = camera(step * F, yaw * F)
    n_real = n_curr - n_curr // 4
    X_cam = np.stack([rng.uniform(-1, 1, 4 * n_curr + 8), rng.uniform(-1, 1, 4 * n_curr + 8), rng.uniform(depth[0], depth[1], 4 * n_curr + 8)], 1)
    X_cam[:, 0] *= 0.55 * X_cam[:, 2]
    X_cam[:, 1] *= 0.42 * X_cam[:, 2]
    X = X_cam @ T_c[:3, :3].T + T_c[:3, 3]
    p, z = E.project(T_c, K, X)
    ok = (z > 0) & (p[:, 0] > 8) & (p[:, 0] < cols - 8) & (p[:, 1] > 8) & (p[:, 1] < rows - 8)
    X = X[ok][:n_real]
    n_real = len(X)
    bits = rng.randint(0, 2, (n_real, 256)).astype(np.uint8)

    def observe(pts):
        b = bits[pts].copy()
        for r in range(len(b)):
            b[r, rng.permutation(256)[:flips]] ^= 1
        return np.packbits(b, axis=1).reshape(-1, 32)

    def keypoints(T, nk, pts, px, mirrored=None):
        xy = rng.uniform([8, 8], [cols - 8, rows - 8], (nk, 2)).astype(np.float32)
        d = np.packbits(rng.randint(0, 2, (nk, 256)).astype(np.uint8), axis=1).reshape(nk, 32)
        point = np.full(nk, -1, np.int32)
        slot = rng.permutation(nk)[:len(pts)]
        if len(pts):
            xy[slot] = (px + rng.normal(0, noise, (len(pts), 2))).astype(np.float32)
            d[slot] = observe(pts)
            point[slot] = pts if mirrored is None else np.where(mirrored, -2 - pts, pts)
        scale = (np.float32(1.2) ** rng.randint(0, 4, nk)).astype(np.float32) if scales else None
        return dict(desc=d, xy=xy, scale=scale, conn=np.full(nk, -1, np.int32), T=T), point

    pts_c = rng.permutation(n_real)
    curr, point_c = keypoints(T_c, n_curr, pts_c, E.project(T_c, K, X[pts_c])[0])
    if twins:
        real = np.nonzero(point_c >= 0)[0]
        for a, b in zip(real[0::8], real[1::8]):             # b becomes a second keypoint on a's point
            curr["xy"][b] = curr["xy"][a]
            curr["desc"][b] = observe(point_c[a:a + 1])[0]
            point_c[b] = point_c[a]
    if busy:
        curr["conn"][rng.permutation(n_curr)[:n_curr // 5]] = rng.choice([0, 3, -2, 17], n_curr // 5)
    curr["conn"][:block] = 5
    seen_c = np.unique(point_c[point_c >= 0])
    frames, point_f = [], []
    C_c = T_c[:3, 3]
    for f in range(F):
        T = T_c.copy() if f in still else camera(step * f, yaw * f)
        nk = int(kp_counts[f])
        cand = rng.permutation(seen_c)
        mirrored = ((np.arange(len(cand)) % 9) == 4) & mirror
        Xf = np.where(mirrored[:, None], 2 * C_c - X[cand], X[cand])
        px, zf = E.project(T, K, Xf)
        vis = (px[:, 0] > 8) & (px[:, 0] < cols - 8) & (px[:, 1] > 8) & (px[:, 1] < rows - 8) & ((zf > 0) != mirrored)
        keep = np.nonzero(vis)[0][:nk - nk // 4]
        fr, pt = keypoints(T, nk, cand[keep], px[keep], mirrored[keep])
        if busy:
            fr["conn"][rng.permutation(nk)[:nk // 7]] = rng.choice([1, 2, -2], nk // 7)
        frames.append(fr)
        point_f.append(pt)
    for fr in [curr] + frames:
        for a in fr.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return dict(curr=curr, frames=frames, point_c=point_c, point_f=point_f, X=X)


def prototype_scene(seed=7, n_points=400, n_cameras=6, step=0.083, K=FR1_K, cols=640, rows=480, noise=0.5, flips=15):
    """The scene of the CPU prototype of section 20: n_cameras cameras in a row, `step` apart, all looking down +z, the last one
    curr; n_points points at depth 2 to 6; every camera sees the points inside its image as noisy projections with `flips`
    flipped descriptor bits, and a quarter of its keypoints are distractors.  Every keypoint is free, no scales.
    -> dict(curr, frames (oldest first), point_c, point_f (the point of each keypoint, -1 a distractor))."""
    rng = np.random.RandomState(seed)
    z = rng.uniform(2.0, 6.0, n_points)
    X = np.stack([rng.uniform(-0.62, 0.62, n_points) * z + 0.5 * step * (n_cameras - 1), rng.uniform(-0.46, 0.46, n_points) * z, z], 1)
    bits = rng.randint(0, 2, (n_points, 256)).astype(np.uint8)
    views, points = [], []
    for c in range(n_cameras):
        T = camera(step * c)
        px, zc = E.project(T, K, X)
        vis = np.nonzero((zc > 0) & (px[:, 0] > 0) & (px[:, 0] < cols) & (px[:, 1] > 0) & (px[:, 1] < rows))[0]
        nk = len(vis) + len(vis) // 3
        xy = rng.uniform([0, 0], [cols, rows], (nk, 2)).astype(np.float32)
        d = np.packbits(rng.randint(0, 2, (nk, 256)).astype(np.uint8), axis=1).reshape(nk, 32)
        point = np.full(nk, -1, np.int32)
        slot = rng.permutation(nk)[:len(vis)]
        xy[slot] = (px[vis] + rng.normal(0, noise, (len(vis), 2))).astype(np.float32)
        b = bits[vis].copy()
        for r in range(len(b)):
            b[r, rng.permutation(256)[:flips]] ^= 1
        d[slot] = np.packbits(b, axis=1)
        point[slot] = vis
        views.append(dict(desc=d, xy=xy, scale=None, conn=np.full(nk, -1, np.int32), T=T))
        points.append(point)
    return dict(curr=views[-1], frames=views[:-1], point_c=points[-1], point_f=points[:-1])
