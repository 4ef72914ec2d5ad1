"""TEST AID: the fusion of duplicate map points transcribed to numpy and plain Python from its declared
rule -- the seen masks, the search of every map point in every buffered frame (the projection, in-view test and inclusive disc
gate of section 15 with a point already seen in the frame set aside and a keypoint of a departed point parked out of reach), the
candidates, one claimant per keypoint, the merges in ascending (d, f, i) over components kept as plain sets, the additions, the
survivors.  Python integers for the masks; it shares no code with the product (csrc/map_fuse_kernels.hip,
csrc/map_fuse_host.cpp) and is what the MI355X and the emulated build are compared with, bit for bit.  Its own known answers
are in tests/test_map_fuse_numpy.py.  scene() builds the synthetic scene those tests, the GPU tests and the host program share.

A frame is a dict: desc (n x 32 uint8), xy (n x 2 f32), scale (n f32 or None), conn (n int32: >= 0 map row, -1 free, -2 a point
that left the map), T (4 x 4, camera to world)."""
import numpy as np

import projection_numpy as P
from projection_numpy import FR1_K, INT32_MAX  # noqa: F401

DEFAULT_MAX_PX, DEFAULT_MAX_HAMMING = 3.0, 50


def seen_masks(n_map, frames):
    """seen[i]: bit f set when some conn[f][j] == i (Python integers)."""
    seen = [0] * n_map
    for f, fr in enumerate(frames):
        for c in np.asarray(fr["conn"]).reshape(-1):
            if c >= 0:
                seen[int(c)] |= 1 << f
    return seen


def search(pos, desc, frames, K, cols, rows, max_px):
    """-> idx F x n x 2, dist F x n x 2, n_candidates F x n, px F x n x 2 f32: per frame the rows of section 15's raw call,
    with active = in_view and not seen in the frame in the place of in_view, and r2 = -1.0 for a conn == -2 keypoint."""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    n, F = len(desc), len(frames)
    seen = seen_masks(n, frames)
    idx = np.full((F, n, 2), -1, np.int32)
    dist = np.full((F, n, 2), INT32_MAX, np.int32)
    cnt = np.full((F, n), -1, np.int32)
    px = np.zeros((F, n, 2), np.float32)
    if n == 0:
        return idx, dist, cnt, px
    for f, fr in enumerate(frames):
        t = np.asarray(fr["desc"], np.uint8).reshape(-1, 32)
        nt = len(t)
        u, v, in_view = P.project_map(pos, fr["T"], K, cols, rows)
        active = in_view & ~np.array([(s >> f) & 1 for s in seen], bool)
        px[f] = np.where(active[:, None], np.stack([u, v], 1), np.float32(0))
        cnt[f] = np.where(active, 0, -1)
        if nt == 0:
            continue
        r2 = P.radii2(nt, max_px, fr.get("scale"))
        r2 = np.where(np.asarray(fr["conn"]).reshape(-1) == -2, -1.0, r2)
        ok = P.gate(u, v, active, fr["xy"], r2)
        d = np.where(ok, P.hamming(desc, t).astype(np.int64), 1 << 40)
        order = np.argsort(d, axis=1, kind="stable")[:, :2]      # stable: the lower keypoint first among equal distances
        passing = ok.sum(1).astype(np.int32)
        cnt[f][active] = passing[active]
        for k in range(min(2, nt)):
            have = passing > k
            idx[f][have, k] = order[have, k]
            dist[f][have, k] = d[np.nonzero(have)[0], order[have, k]]
    return idx, dist, cnt, px


def resolve(n_map, frames, idx, dist, max_hamming, order_key=None, trace=None):
    """The rule after the search -> replaced_by (n_map int32), added (k x 3 int32: frame, keypoint, point), counts (6 int32:
    candidates, merges accepted, merges refused, observations added, observations refused, points replaced).  order_key, for the
    tests only, replaces the declared order (d, f, i) of the winners; trace, a dict, receives what the tests ask about."""
    seen = seen_masks(n_map, frames)
    key = order_key or (lambda w: (w[0], w[1], w[2]))
    candidates = 0
    winners = {}                                   # (f, j) -> (d, f, i, j), the smallest (d, i)
    contested = 0
    for f in range(len(frames)):
        for i in range(n_map):
            j, d = int(idx[f][i, 0]), int(dist[f][i, 0])
            if j < 0 or d > max_hamming:
                continue
            candidates += 1
            old = winners.get((f, j))
            contested += old is not None
            if old is None or (d, i) < (old[0], old[2]):
                winners[(f, j)] = (d, f, i, j)
    members = {i: {i} for i in range(n_map)}       # component name -> its rows
    name = list(range(n_map))                      # row -> component name
    mask = {i: seen[i] for i in range(n_map)}
    accepted = refused = 0
    for d, f, i, j in sorted((w for w in winners.values() if frames[w[1]]["conn"][w[3]] >= 0), key=key):
        a, b = name[i], name[int(frames[f]["conn"][j])]
        if a == b:
            continue
        if mask[a] & mask[b]:
            refused += 1
            continue
        for r in members[b]:
            name[r] = a
        members[a] |= members.pop(b)
        mask[a] |= mask.pop(b)
        accepted += 1
    survivor = {}
    for a, rows_ in members.items():
        survivor[a] = min(rows_, key=lambda r: (-bin(seen[r]).count("1"), r))
    replaced_by = np.array([survivor[name[i]] for i in range(n_map)], np.int32).reshape(n_map)
    added, add_refused = [], 0
    for d, f, i, j in sorted((w for w in winners.values() if frames[w[1]]["conn"][w[3]] == -1), key=key):
        a = name[i]
        if (mask[a] >> f) & 1:
            add_refused += 1
            continue
        mask[a] |= 1 << f
        added.append((f, j, survivor[a]))
    counts = np.array([candidates, accepted, refused, len(added), add_refused, int((replaced_by != np.arange(n_map)).sum())], np.int32)
    if trace is not None:
        trace.update(contested=contested, sizes=sorted(len(m) for m in members.values()), members=list(members.values()),
                     final_mask=[mask[name[i]] for i in range(n_map)], seen=seen)
    return replaced_by, np.array(added, np.int32).reshape(-1, 3), counts


def fuse(pos, desc, frames, K, cols, rows, max_px=DEFAULT_MAX_PX, max_hamming=DEFAULT_MAX_HAMMING, trace=None):
    idx, dist, _, _ = search(pos, desc, frames, K, cols, rows, max_px)
    return resolve(len(np.asarray(desc, np.uint8).reshape(-1, 32)), frames, idx, dist, max_hamming, trace=trace)


def flip_bits(rng, desc, k):
    """Every 256-bit row of desc with k (a number, or one per row) of its bits flipped."""
    bits = np.unpackbits(np.asarray(desc, np.uint8).reshape(-1, 32), axis=1)
    k = np.broadcast_to(k, len(bits))
    for i in range(len(bits)):
        bits[i, rng.permutation(256)[:k[i]]] ^= 1
    return np.packbits(bits, axis=1)


def scene(rng, n_map, kp_counts, K=FR1_K, cols=640, rows=480, n_clean=None, n_overlap=None, noise=1.0, obs_flips=(2, 46),
          dup_flips=4, scales=False):
    """A map of n_map points in all.  Cameras in a row looking down +z at a cloud of n_points = n_map - n_clean - n_overlap
    points; frame f has kp_counts[f] keypoints: noisy projections of the
    points it sees (noise px a coordinate; descriptor: the point's with obs_flips[0] .. obs_flips[1] bits flipped, so that neither the
    default radius nor the default ceiling admits all of them), the rest distractors at random pixels with random
    descriptors.  Per frame a random half of the projections is connected to its point, the rest is free.  Then duplicates are
    appended to the map: n_clean points copied (dup_flips bits flipped, same position), the connections of the original in
    every second of its frames handed to the copy (disjoint observation sets: a clean duplicate; n_map // 32 originals with three
    connections or more are split three ways, between two clean copies); n_overlap further copies which
    take over some connections and ALSO get a connection of their own, to a free distractor, in a frame where the original keeps
    its (overlapping sets: two points in one frame are two points; with no free distractor the copy stays a clean one).  Every second clean pair has a twin: a free
    distractor moved onto the original's keypoint in a frame of the copy, with the original's descriptor.  Originals
    need two connections; when too few have them the map is filled up with points behind the cameras.  Every tenth free
    keypoint is then connected to a point that left the map (-2).
    -> dict(pos, desc, frames, clean (k x 2: original, copy), overlap (k x 2))."""
    F = len(kp_counts)
    n_clean = n_map // 8 if n_clean is None else n_clean
    n_overlap = n_map // 10 if n_overlap is None else n_overlap
    n_triple = n_map // 32                                   # originals split three ways: two clean copies each
    n_points = n_map - n_clean - n_overlap - 2 * n_triple
    pos = rng.uniform([-1.6, -1.2, 2.5], [1.6 + 0.05 * F, 1.2, 6.0], (n_points, 3)).astype(np.float32)
    desc = np.packbits(rng.randint(0, 2, (n_points, 256)).astype(np.uint8), axis=1)
    frames, where, spare = [], [], []                        # spare: the distractors no duplicate has taken yet
    for f in range(F):
        T = np.eye(4)
        T[0, 3] = 0.05 * f
        nk = int(kp_counts[f])
        u, v, in_view = P.project_map(pos, T, K, cols, rows)
        vis = np.nonzero(in_view & (u > 8) & (u < cols - 8) & (v > 8) & (v < rows - 8))[0]
        vis = rng.permutation(vis)[:nk - nk // 4]             # a quarter of the keypoints at least are distractors
        xy = rng.uniform([8, 8], [cols - 8, rows - 8], (nk, 2)).astype(np.float32)
        d = np.packbits(rng.randint(0, 2, (nk, 256)).astype(np.uint8), axis=1).reshape(nk, 32)
        conn = np.full(nk, -1, np.int32)
        slot = rng.permutation(nk)[:len(vis)]
        if len(vis):
            xy[slot] = (np.stack([u[vis], v[vis]], 1).astype(np.float64) + rng.normal(0, noise, (len(vis), 2))).astype(np.float32)
            d[slot] = flip_bits(rng, desc[vis], rng.randint(obs_flips[0], obs_flips[1] + 1, len(vis)))
            linked = rng.rand(len(vis)) < 0.5
            conn[slot[linked]] = vis[linked]
        scale = (np.float32(1.2) ** rng.randint(0, 4, nk)).astype(np.float32) if scales else None
        frames.append(dict(desc=d, xy=xy, scale=scale, conn=conn, T=T))
        where.append({int(p): int(s) for p, s in zip(vis, slot)})
        spare.append(sorted(set(range(nk)) - set(int(x) for x in slot)))
    # duplicates: originals observed (connected) in at least two frames
    linked_in = [[f for f in range(F) if i in where[f] and frames[f]["conn"][where[f][i]] == i] for i in range(n_points)]
    pool = [i for i in rng.permutation(n_points) if len(linked_in[i]) >= 2]
    clean, overlap = [], []
    new_pos, new_desc = [pos], [desc]
    nxt = n_points
    triple = [i for i in pool if len(linked_in[i]) >= 3][:n_triple]
    for i in triple:
        for c in (1, 2):                                     # connections 1, 4, 7 ... and 2, 5, 8 ... go to the two copies
            for f in linked_in[i][c::3]:
                frames[f]["conn"][where[f][i]] = nxt
            clean.append((i, nxt))
            new_pos.append(pos[i:i + 1])
            new_desc.append(flip_bits(rng, desc[i:i + 1], dup_flips))
            nxt += 1
    pool = [i for i in pool if i not in triple]
    for k, i in enumerate(pool[:n_clean + n_overlap]):
        fs = linked_in[i]
        for f in fs[1::2]:                                   # every second connection goes to the copy
            frames[f]["conn"][where[f][i]] = nxt
        if k < n_clean or not spare[fs[0]]:
            clean.append((i, nxt))
            if k % 2 == 0 and spare[fs[1]]:                  # a TWIN: a free keypoint on the original's pixel in a frame of the
                j, f = spare[fs[1]].pop(0), fs[1]            # copy, with the original's very descriptor: the original claims it
                xy_f, d_f = frames[f]["xy"], frames[f]["desc"]   # there, and once the two are one point the frame is taken
                xy_f[j], d_f[j] = xy_f[where[f][i]], desc[i]
        else:                                                # ... and the copy claims a free distractor in a frame the original keeps
            frames[fs[0]]["conn"][spare[fs[0]].pop(0)] = nxt
            overlap.append((i, nxt))
        new_pos.append(pos[i:i + 1])
        new_desc.append(flip_bits(rng, desc[i:i + 1], dup_flips))
        nxt += 1
    if nxt < n_map:                                          # filler: behind every camera
        new_pos.append(rng.uniform([-1, -1, -6], [1, 1, -2], (n_map - nxt, 3)).astype(np.float32))
        new_desc.append(np.packbits(rng.randint(0, 2, (n_map - nxt, 256)).astype(np.uint8), axis=1))
    for f in range(F):
        c = frames[f]["conn"]
        gone = np.nonzero(c == -1)[0][9::10]
        c[gone] = -2
    out = dict(pos=np.concatenate(new_pos).astype(np.float32), desc=np.concatenate(new_desc), frames=frames,
               clean=np.array(clean, np.int32).reshape(-1, 2), overlap=np.array(overlap, np.int32).reshape(-1, 2))
    for a in (out["pos"], out["desc"], out["clean"], out["overlap"]):
        a.setflags(write=False)
    for fr in frames:
        for a in fr.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out
