"""TEST AID: tracking the local map transcribed to numpy from its declared arithmetic -- the projection
with its in-view test (projection_numpy.project_map), the distance to the camera centre, the range, the viewing cosine, the
predicted level as a count, the radius, the inclusive disc with the level window, the two nearest passing keypoints with the
tie rule, ORB-SLAM's acceptance rule and the one-point-per-keypoint rule.  Vectorised f64 (numpy rounds every elementwise
product, sum, quotient and square root on its own, which is the declared order); it shares no code with the product
(csrc/local_map_kernels.hip, csrc/local_map_host.cpp) and is what the MI355X and the emulated build are compared with, bit for
bit.  Its own known answers are in tests/test_local_map_numpy.py.  scene() builds the inputs the emulated and the GPU tests
share; trace() says which clause decided which pair."""
import functools

import numpy as np

from epipolar_numpy import DMATCH, FR1_K, INT32_MAX, hamming
from projection_numpy import pose, project_map

DEFAULTS = dict(min_view_cos=0.5, radius_near=2.5, radius_far=4.0, near_cos=0.998, radius_scale=1.0, lowe_ratio=0.8, max_hamming=100)


def level_scales(scale_factor, L):
    """level_scale[l] = scale_factor multiplied l times, in f64."""
    out, s = [], np.float64(1.0)
    for _ in range(L):
        out.append(s)
        s = s * np.float64(scale_factor)
    return np.array(out, np.float64)


def view(pos, normal, max_dist, T_w_c, K, cols, rows, level_scale, skip=None, params=None):
    """Per map point -> dict(u, v, in_view, dist, in_range, vc, facing, lv, r2, skip, active)."""
    P = dict(DEFAULTS, **(params or {}))
    ls = np.asarray(level_scale, np.float64).reshape(-1)
    L = len(ls)
    T = np.asarray(T_w_c, np.float64).reshape(4, 4)
    p = np.asarray(pos, np.float32).reshape(-1, 3).astype(np.float64)
    n = len(p)
    nrm = np.asarray(normal, np.float32).reshape(-1, 3).astype(np.float64)
    md = np.asarray(max_dist, np.float32).reshape(-1).astype(np.float64)
    skip = np.zeros(n, bool) if skip is None else np.asarray(skip).reshape(-1) != 0
    u, v, in_view = project_map(pos, T, K, cols, rows)
    with np.errstate(all="ignore"):
        dx, dy, dz = p[:, 0] - T[0, 3], p[:, 1] - T[1, 3], p[:, 2] - T[2, 3]
        s = dx * dx
        s = s + dy * dy
        s = s + dz * dz
        dist = np.sqrt(s)
        lo = np.float64(0.8) * (md / ls[L - 1])
        hi = np.float64(1.2) * md
        in_range = (md > 0) & (dist >= lo) & (dist <= hi)
        dot = (dx * nrm[:, 0] + dy * nrm[:, 1]) + dz * nrm[:, 2]
        vc = dot / dist
        facing = vc >= np.float64(P["min_view_cos"])
        lv = np.zeros(n, np.int32)
        for l in range(L - 1):
            lv += (dist * ls[l] < md).astype(np.int32)
        r = (np.where(vc > np.float64(P["near_cos"]), np.float64(P["radius_near"]), np.float64(P["radius_far"]))
             * np.float64(P["radius_scale"])) * ls[lv]
        r2 = r * r
    active = in_view & in_range & facing & ~skip
    return dict(u=u, v=v, in_view=in_view, dist=dist, in_range=in_range, vc=vc, facing=facing, lv=lv, r2=r2, skip=skip, active=active)


def pair_clauses(w, txy, levels):
    """n_map x nt bool each: the disc (inclusive; a NaN passes nothing) and the level window for the given keypoint levels."""
    t = np.asarray(txy, np.float32).reshape(-1, 2).astype(np.float64)
    lev = np.asarray(levels, np.int32).reshape(-1)
    with np.errstate(all="ignore"):
        du = t[:, 0][None, :] - w["u"].astype(np.float64)[:, None]
        dv = t[:, 1][None, :] - w["v"].astype(np.float64)[:, None]
        d2 = du * du + dv * dv
        disc = d2 <= w["r2"][:, None]
    window = (lev[None, :] == w["lv"][:, None]) | (lev[None, :] == w["lv"][:, None] - 1)
    return disc, window


def knn2(pos, desc, normal, max_dist, T_w_c, K, cols, rows, t, txy, t_level, level_scale, skip=None, params=None):
    """-> px n_map x 2 f32, idx n_map x 2, dist n_map x 2, n_candidates, level (int32), view_cos (f64).  Active: the two smallest
    distances among the passing keypoints, equal distances keep the lower train index first, a missing neighbour is
    (-1, INT32_MAX).  Not active: px (0, 0), idx -1, dist INT32_MAX, n_candidates -1, level -1, view_cos 0.0."""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    t = np.asarray(t, np.uint8).reshape(-1, 32)
    n, nt = len(desc), len(t)
    w = view(pos, normal, max_dist, T_w_c, K, cols, rows, level_scale, skip, params)
    act = w["active"]
    px = np.where(act[:, None], np.stack([w["u"], w["v"]], 1), np.float32(0)).astype(np.float32)
    idx = np.full((n, 2), -1, np.int32)
    dist = np.full((n, 2), INT32_MAX, np.int32)
    cnt = np.where(act, 0, -1).astype(np.int32)
    lv = np.where(act, w["lv"], -1).astype(np.int32)
    vc = np.where(act, w["vc"], 0.0).astype(np.float64)
    if n == 0 or nt == 0:
        return px, idx, dist, cnt, lv, vc
    disc, window = pair_clauses(w, txy, t_level)          # (a taken keypoint, level -2, is in nobody's window: lv - 1 >= -1)
    ok = act[:, None] & disc & window
    d = np.where(ok, hamming(desc, t).astype(np.int64), 1 << 40)
    order = np.argsort(d, axis=1, kind="stable")[:, :2]      # stable: the lower index first among equal distances
    passing = ok.sum(1).astype(np.int32)
    cnt[act] = passing[act]
    for k in range(min(2, nt)):
        have = passing > k
        idx[have, k] = order[have, k]
        dist[have, k] = d[np.nonzero(have)[0], order[have, k]]
    return px, idx, dist, cnt, lv, vc


def filter_local(idx, dist, t_level, lowe_ratio=0.8, max_hamming=100):
    """ORB-SLAM's rule: kept if idx0 >= 0, d0 <= max_hamming and (idx1 < 0 or the two neighbours sit on different levels or
    (double)d0 <= lowe_ratio (double)d1); one point per keypoint (smallest distance, then the lower map index); sorted by
    trainIdx."""
    lev = np.asarray(t_level, np.int32).reshape(-1)
    best = {}
    for i in range(len(idx)):
        j0, j1, d0, d1 = int(idx[i][0]), int(idx[i][1]), int(dist[i][0]), int(dist[i][1])
        if j0 < 0 or d0 > max_hamming:
            continue
        if not (j1 < 0 or lev[j0] != lev[j1] or np.float64(d0) <= np.float64(lowe_ratio) * np.float64(d1)):
            continue
        if j0 not in best or d0 < best[j0][0]:
            best[j0] = (d0, i)
    out = np.zeros(len(best), DMATCH)
    for k, j in enumerate(sorted(best)):
        out[k] = (best[j][1], j, 0, np.float32(best[j][0]))
    return out


def match_features(pos, desc, normal, max_dist, T_w_c, K, cols, rows, t, txy, t_level, level_scale, skip=None, params=None):
    P = dict(DEFAULTS, **(params or {}))
    _, idx, dist, _, _, _ = knn2(pos, desc, normal, max_dist, T_w_c, K, cols, rows, t, txy, t_level, level_scale, skip, params)
    return filter_local(idx, dist, t_level, P["lowe_ratio"], P["max_hamming"])


CLAUSES = ("range", "facing", "level window", "disc", "taken", "skip", "ceiling", "ratio", "level exemption")


def trace(pos, desc, normal, max_dist, T_w_c, K, cols, rows, t, txy, octave, taken, level_scale, skip=None, params=None):
    """How many pairs (for the last three: points) each clause decides ALONE: every other clause lets the pair through and this
    one stops it.  octave: the keypoints' levels before the taken ones were marked; taken: nt bool.  ceiling: a nearest
    neighbour over the ceiling that the ratio rule would have kept; ratio: one under the ceiling that the ratio stops;
    level exemption: one under the ceiling, kept although the ratio fails, because its neighbours sit on different levels."""
    P = dict(DEFAULTS, **(params or {}))
    taken = np.asarray(taken, bool).reshape(-1)
    t_level = np.where(taken, -2, np.asarray(octave, np.int32)).astype(np.int32)
    w = view(pos, normal, max_dist, T_w_c, K, cols, rows, level_scale, skip, params)
    disc, window = pair_clauses(w, txy, octave)
    n, nt = disc.shape
    full = lambda a: np.repeat(a[:, None], nt, 1)
    c = {"in view": full(w["in_view"]), "range": full(w["in_range"]), "facing": full(w["facing"]), "skip": full(~w["skip"]),
         "level window": window, "disc": disc, "taken": np.repeat(~taken[None, :], n, 0)}
    out = {}
    for name in CLAUSES[:6]:
        others = np.ones((n, nt), bool)
        for k, m in c.items():
            if k != name:
                others &= m
        out[name] = int((others & ~c[name]).sum())
    _, idx, dist, _, _, _ = knn2(pos, desc, normal, max_dist, T_w_c, K, cols, rows, t, txy, t_level, level_scale, skip, params)
    has0, has1 = idx[:, 0] >= 0, idx[:, 1] >= 0
    under = has0 & (dist[:, 0] <= P["max_hamming"])
    same = has1 & (t_level[np.maximum(idx[:, 0], 0)] == t_level[np.maximum(idx[:, 1], 0)])
    ratio_ok = dist[:, 0].astype(np.float64) <= np.float64(P["lowe_ratio"]) * dist[:, 1].astype(np.float64)
    out["ceiling"] = int((has0 & ~under & (~has1 | ~same | ratio_ok)).sum())
    out["ratio"] = int((under & same & ~ratio_ok).sum())
    out["level exemption"] = int((under & has1 & ~same & ~ratio_ok).sum())
    return out


COLS, ROWS = 640, 480
SCALE_FACTOR = 1.2


def _scene(n_map, nt, L, seed):
    rng = np.random.RandomState(seed)
    K = FR1_K
    ls = level_scales(SCALE_FACTOR, L)
    T = pose(rng.uniform(-0.08, 0.08, 3), rng.uniform(-0.4, 0.4, 3))
    # the map: pixels of the frame back-projected to random depths; every seventh point behind the camera or outside the frame
    pix = rng.uniform([20, 20], [COLS - 20, ROWS - 20], (n_map, 2))
    z = rng.uniform(1.0, 8.0, n_map)
    out = np.arange(n_map) % 7 == 6
    how = rng.randint(0, 3, n_map)
    pix[out & (how == 1), 0] += COLS
    pix[out & (how == 2), 1] -= ROWS
    z[out & (how == 0)] *= -1
    Xc = np.stack([(pix[:, 0] - K["cx"]) / K["fx"] * z, (pix[:, 1] - K["cy"]) / K["fy"] * z, z], 1)
    pos = (Xc @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    desc = rng.randint(0, 256, (n_map, 32)).astype(np.uint8)
    # normals: the viewing direction turned by up to 75 degrees (a third within 3 degrees: the near radius); a few NaN
    d = pos.astype(np.float64) - T[:3, 3]
    dist = np.linalg.norm(d, axis=1)
    d /= dist[:, None]
    ang = np.where(rng.rand(n_map) < 0.33, rng.uniform(0, 3, n_map), rng.uniform(3, 75, n_map)) * np.pi / 180
    side = np.cross(d, rng.normal(size=(n_map, 3)))
    side /= np.linalg.norm(side, axis=1)[:, None]
    normal = (np.cos(ang)[:, None] * d + np.sin(ang)[:, None] * side).astype(np.float32)
    normal[rng.rand(n_map) < 0.02, 1] = np.nan
    # max_dist: the point sits on level k; some pushed out of range on either side, a few not positive
    k = rng.randint(0, L, n_map)
    md = dist * ls[k] * rng.uniform(0.86, 0.99, n_map)
    kind = rng.rand(n_map)
    md[kind < 0.10] *= 0.7
    md[(kind >= 0.10) & (kind < 0.16)] *= ls[L - 1] * 1.5
    md[(kind >= 0.16) & (kind < 0.18)] = 0.0
    md[(kind >= 0.18) & (kind < 0.19)] = -1.0
    max_dist = md.astype(np.float32)
    skip = (rng.rand(n_map) < 0.10).astype(np.uint8)
    # the frame: every keypoint near the projection of a point (every other one of any point, the rest of the first few active ones,
    # which so have several candidates), on a level around the predicted one, its descriptor a number of bits from the point's
    w = view(pos, normal, max_dist, T, K, COLS, ROWS, ls)
    j = np.arange(nt)
    live = np.nonzero(w["active"] & (skip == 0))[0]
    live = live if len(live) else np.arange(n_map)
    target = np.where(j % 2 == 0, rng.randint(0, n_map, nt), live[rng.randint(0, np.minimum(len(live), 1 + j // 16))])
    centre = np.stack([w["u"], w["v"]], 1).astype(np.float64)[target]
    lost = ~np.isfinite(centre).all(1) | ~w["in_view"][target]
    centre[lost] = rng.uniform([0, 0], [COLS, ROWS], (int(lost.sum()), 2))
    rad = np.sqrt(np.where(np.isfinite(w["r2"][target]), w["r2"][target], 16.0))
    txy = (centre + rng.uniform(-1, 1, (nt, 2)) * (1.3 * rad)[:, None]).astype(np.float32)
    octave = np.clip(w["lv"][target] + rng.choice([-2, -1, -1, -1, 0, 0, 0, 1], nt), 0, L - 1).astype(np.int32)
    taken = rng.rand(nt) < 0.10
    bits = np.unpackbits(desc[target], axis=1)
    for j in range(nt):
        bits[j, rng.permutation(256)[:rng.choice([3, 20, 25, 30, 30, 35, 40, 60, 110, 128])]] ^= 1
    t = np.packbits(bits, axis=1)
    return dict(K=K, cols=COLS, rows=ROWS, T=T, level_scale=ls, pos=pos, desc=desc, normal=normal, max_dist=max_dist, skip=skip,
                t=t, txy=txy, octave=octave, taken=taken, t_level=np.where(taken, -2, octave).astype(np.int32))


NT_MAX = 1100


@functools.lru_cache(maxsize=None)
def scene(n_map, L, seed=None):
    """The scene of one (map size, number of levels): NT_MAX keypoints, of which a test takes the first nt.  Built once; callers
    must not write."""
    s = _scene(n_map, NT_MAX, L, 100 * n_map + L if seed is None else seed)
    for a in s.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return s


def scene_args(s, nt):
    """The arguments of knn2 / match_features behind (pos, desc, normal, max_dist) for the first nt keypoints."""
    return (s["T"], s["K"], s["cols"], s["rows"], s["t"][:nt], s["txy"][:nt], s["t_level"][:nt], s["level_scale"])


@functools.lru_cache(maxsize=None)
def scene_answer(n_map, L, nt, params=None):
    s = scene(n_map, L)
    P = dict(params) if params else None
    m = (s["pos"], s["desc"], s["normal"], s["max_dist"])
    raw = knn2(*m, *scene_args(s, nt), s["skip"], P)
    feat = match_features(*m, *scene_args(s, nt), s["skip"], P)
    for a in raw + (feat,):
        a.setflags(write=False)
    return raw, feat


def scene_trace(n_map, L, nt, params=None):
    s = scene(n_map, L)
    return trace(s["pos"], s["desc"], s["normal"], s["max_dist"], s["T"], s["K"], s["cols"], s["rows"], s["t"][:nt], s["txy"][:nt],
                 s["octave"][:nt], s["taken"][:nt], s["level_scale"], s["skip"], dict(params) if params else None)
