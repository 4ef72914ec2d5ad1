"""Known answers, worked by hand, for the numpy transcription of the fusion of duplicate map points (tests/map_fuse_numpy.py,
DESIGN.md section 19) -- the transcription is what the MI355X and the emulated build are compared with, so it has to stand on
its own: the inclusive gate with exact arithmetic, the rows of pairs that are not active, the tie rules, and every branch of the
rule after the search; then the invariants on a synthetic scene with planted duplicates."""
import numpy as np
import pytest

import map_fuse_numpy as M

INT32_MAX = M.INT32_MAX
# fx = fy = 64, identity pose: the point (0.5, 0.25, 2) lands on u = 64 * 0.5 / 2 + 320 = 336, v = 64 * 0.25 / 2 + 240 = 248, exactly
K = dict(fx=64.0, fy=64.0, cx=320.0, cy=240.0)
COLS, ROWS = 640, 480
ZERO = np.zeros((1, 32), np.uint8)


def bits(k):
    """A descriptor with its first k bits set: Hamming distance k from ZERO."""
    b = np.zeros(256, np.uint8)
    b[:k] = 1
    return np.packbits(b)


def frame(xy, desc, conn, scale=None, T=None):
    return dict(xy=np.array(xy, np.float32).reshape(-1, 2), desc=np.array(desc, np.uint8).reshape(-1, 32),
                conn=np.array(conn, np.int32).reshape(-1), scale=scale, T=np.eye(4) if T is None else T)


def test_the_gate_is_inclusive_at_d2_equal_r2():
    pos = np.array([[0.5, 0.25, 2.0]], np.float32)
    # (339, 252): du = 3, dv = 4, d2 = 25 = 5^2 exactly; (339, 252.5): d2 = 9 + 20.25 = 29.25
    fr = frame([[339, 252], [339, 252.5]], [bits(3), bits(1)], [-1, -1])
    idx, dist, cnt, px = M.search(pos, ZERO, [fr], K, COLS, ROWS, 5.0)
    assert px[0, 0].tolist() == [336.0, 248.0]
    assert idx[0, 0].tolist() == [0, -1] and dist[0, 0].tolist() == [3, INT32_MAX] and cnt[0, 0] == 1
    idx, dist, cnt, _ = M.search(pos, ZERO, [fr], K, COLS, ROWS, np.nextafter(5.0, 0.0))
    assert idx[0, 0].tolist() == [-1, -1] and cnt[0, 0] == 0
    # the scale multiplies the radius keypoint by keypoint: 2.5 * 2 = 5 for keypoint 0 only
    fr = dict(fr, scale=np.array([2.0, 1.0], np.float32))
    idx, dist, cnt, _ = M.search(pos, ZERO, [fr], K, COLS, ROWS, 2.5)
    assert idx[0, 0].tolist() == [0, -1] and cnt[0, 0] == 1


def test_a_pair_already_seen_in_the_frame_and_a_point_not_in_view():
    pos = np.array([[0.5, 0.25, 2.0], [0.5, 0.25, -2.0], [0.5, 0.25, 2.0]], np.float32)
    desc = np.repeat(ZERO, 3, 0)
    f0 = frame([[336, 248], [100, 100]], [bits(2), bits(0)], [-1, 2])      # point 2 is connected in frame 0 (elsewhere)
    f1 = frame([[336, 248]], [bits(4)], [-1])
    idx, dist, cnt, px = M.search(pos, desc, [f0, f1], K, COLS, ROWS, 3.0)
    assert M.seen_masks(3, [f0, f1]) == [0, 0, 1]
    assert idx[0].tolist() == [[0, -1], [-1, -1], [-1, -1]] and cnt[0].tolist() == [1, -1, -1]
    assert px[0].tolist() == [[336, 248], [0, 0], [0, 0]]                  # behind the camera; already seen in frame 0
    assert dist[0].tolist() == [[2, INT32_MAX], [INT32_MAX, INT32_MAX], [INT32_MAX, INT32_MAX]]
    assert idx[1].tolist() == [[0, -1], [-1, -1], [0, -1]] and cnt[1].tolist() == [1, -1, 1]      # ... but not in frame 1
    assert px[1, 2].tolist() == [336, 248]


def test_equal_distances_keep_the_lower_keypoint_and_a_departed_points_keypoint_never_passes():
    pos = np.array([[0.5, 0.25, 2.0]], np.float32)
    fr = frame([[336, 248]] * 4, [bits(1), bits(5), bits(5), bits(5)], [-2, -1, -1, -1])
    idx, dist, cnt, _ = M.search(pos, ZERO, [fr], K, COLS, ROWS, 3.0)
    assert idx[0, 0].tolist() == [1, 2] and dist[0, 0].tolist() == [5, 5] and cnt[0, 0] == 3
    # max_px 0: d2 = 0 <= 0 passes, the parked r2 = -1 still does not
    idx, dist, cnt, _ = M.search(pos, ZERO, [fr], K, COLS, ROWS, 0.0)
    assert idx[0, 0].tolist() == [1, 2] and cnt[0, 0] == 3


def raw(F, n, entries):
    """idx / dist of a search with the first neighbours given as {(f, i): (j, d)}."""
    idx, dist = np.full((F, n, 2), -1, np.int32), np.full((F, n, 2), INT32_MAX, np.int32)
    for (f, i), (j, d) in entries.items():
        idx[f, i, 0], dist[f, i, 0] = j, d
    return idx, dist


def conns(*per_frame):
    return [dict(conn=np.array(c, np.int32)) for c in per_frame]


def test_two_points_claim_one_keypoint():
    frames = conns([-1])
    rep, added, counts = M.resolve(2, frames, *raw(1, 2, {(0, 0): (0, 10), (0, 1): (0, 5)}), 50)
    assert added.tolist() == [[0, 0, 1]] and counts.tolist() == [2, 0, 0, 1, 0, 0] and rep.tolist() == [0, 1]
    rep, added, counts = M.resolve(2, frames, *raw(1, 2, {(0, 0): (0, 5), (0, 1): (0, 5)}), 50)      # equal: the lower point
    assert added.tolist() == [[0, 0, 0]] and counts.tolist() == [2, 0, 0, 1, 0, 0]
    rep, added, counts = M.resolve(2, frames, *raw(1, 2, {(0, 0): (0, 51), (0, 1): (0, 50)}), 50)    # the ceiling is inclusive
    assert added.tolist() == [[0, 0, 1]] and counts.tolist() == [1, 0, 0, 1, 0, 0]


def test_a_merge_a_survivor_tie_and_a_survivor_by_observations():
    # point 1 is seen in frame 0, point 0 in frame 1; in frame 0 point 0 claims the keypoint of point 1
    frames = conns([1], [0])
    rep, added, counts = M.resolve(2, frames, *raw(2, 2, {(0, 0): (0, 7)}), 50)
    assert rep.tolist() == [0, 0] and counts.tolist() == [1, 1, 0, 0, 0, 1] and len(added) == 0      # one observation each: the lower row
    frames = conns([1], [0], [1])                                                                   # point 1 seen twice
    rep, added, counts = M.resolve(2, frames, *raw(3, 2, {(0, 0): (0, 7)}), 50)
    assert rep.tolist() == [1, 1] and counts.tolist() == [1, 1, 0, 0, 0, 1]


def test_a_merge_refused_by_the_mask():
    # point 0 seen in frame 1, point 1 in frames 0 and 1: two points observed in frame 1 are two points
    frames = conns([1], [0, 1])
    rep, added, counts = M.resolve(2, frames, *raw(2, 2, {(0, 0): (0, 7)}), 50)
    assert rep.tolist() == [0, 1] and counts.tolist() == [1, 0, 1, 0, 0, 0]


def test_a_chain_ends_as_one_component():
    # points 0, 1, 2 seen in frames 0, 1, 2; 0 claims 1's keypoint in frame 1, 1 claims 2's in frame 2, then 2 claims 0's in
    # frame 0: the same component already, nothing happens and nothing is counted
    frames = conns([0], [1], [2])
    trace = {}
    idx, dist = raw(3, 3, {(1, 0): (0, 3), (2, 1): (0, 4), (0, 2): (0, 9)})
    rep, added, counts = M.resolve(3, frames, idx, dist, 50, trace=trace)
    assert rep.tolist() == [0, 0, 0] and counts.tolist() == [3, 2, 0, 0, 0, 2] and trace["sizes"] == [3]
    assert trace["final_mask"] == [7, 7, 7]


def test_an_addition_and_additions_refused_after_a_merge_set_the_bit():
    # point 0 seen in frame 0, point 1 in frame 1.  Frame 1: point 0 claims point 1's keypoint (d 2): united, mask {0, 1}.
    # Frame 0: point 1 claims the free keypoint 1 (d 3): bit 0 came with point 0 -> refused.  Frame 2: point 0 claims the free
    # keypoint 0 (d 4): added for the survivor; point 1 claims the free keypoint 1 (d 6): the bit is set by now -> refused.
    frames = conns([0, -1], [1], [-1, -1])
    idx, dist = raw(3, 2, {(1, 0): (0, 2), (0, 1): (1, 3), (2, 0): (0, 4), (2, 1): (1, 6)})
    trace = {}
    rep, added, counts = M.resolve(2, frames, idx, dist, 50, trace=trace)
    assert rep.tolist() == [0, 0] and added.tolist() == [[2, 0, 0]] and counts.tolist() == [4, 1, 0, 1, 2, 1]
    assert trace["final_mask"] == [7, 7]
    # without the merge (ceiling 1) both points take their keypoints
    rep, added, counts = M.resolve(2, frames, idx, dist, 1)
    assert counts.tolist() == [0, 0, 0, 0, 0, 0]
    idx2, dist2 = raw(3, 2, {(0, 1): (1, 3), (2, 0): (0, 4), (2, 1): (1, 6)})
    rep, added, counts = M.resolve(2, frames, idx2, dist2, 50)
    assert rep.tolist() == [0, 1] and added.tolist() == [[0, 1, 1], [2, 0, 0], [2, 1, 1]] and counts.tolist() == [3, 0, 0, 3, 0, 0]


def test_a_winner_on_a_departed_points_keypoint_does_nothing():
    rep, added, counts = M.resolve(1, conns([-2]), *raw(1, 1, {(0, 0): (0, 1)}), 50)
    assert rep.tolist() == [0] and len(added) == 0 and counts.tolist() == [1, 0, 0, 0, 0, 0]


def test_the_order_of_the_merges_is_part_of_the_rule():
    # A = 0 seen in frame 0, B = 1 in frame 1, C = 2 in frames 1 and 2.  A claims B's keypoint in frame 1 (d 5) and C's in
    # frame 2 (d 8).  Ascending d: A and B unite, then {A, B} meets C in frame 1 -> refused.  Descending d: A and C unite
    # (C, observed twice, survives), then B meets them in frame 1 -> refused.
    frames = conns([0], [1, 2], [2])
    idx, dist = raw(3, 3, {(1, 0): (0, 5), (2, 0): (0, 8)})
    rep, _, counts = M.resolve(3, frames, idx, dist, 50)
    assert rep.tolist() == [0, 0, 2] and counts.tolist() == [2, 1, 1, 0, 0, 1]
    rep, _, counts = M.resolve(3, frames, idx, dist, 50, order_key=lambda w: (-w[0], w[1], w[2]))
    assert rep.tolist() == [2, 1, 2] and counts.tolist() == [2, 1, 1, 0, 0, 1]
    # equal distances: the frame decides (frame 1 first), as the declared order says
    idx, dist = raw(3, 3, {(1, 0): (0, 5), (2, 0): (0, 5)})
    assert M.resolve(3, frames, idx, dist, 50)[0].tolist() == [0, 0, 2]


def popcount(x):
    return bin(x).count("1")


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_every_planted_clean_duplicate_is_merged(seed):
    """A scene whose observations are close to their points (0.3 px, 8 .. 12 flipped bits): the rule finds every clean duplicate,
    pair or triple, and refuses every duplicate whose observation set overlaps its original's."""
    s = M.scene(np.random.RandomState(seed), 120, [150] * 12, noise=0.3, obs_flips=(8, 12))
    trace = {}
    rep, added, counts = M.fuse(s["pos"], s["desc"], s["frames"], M.FR1_K, 640, 480, trace=trace)
    assert len(s["clean"]) >= 15 and len(s["overlap"]) >= 5 and trace["sizes"][-1] == 3
    for a, b in s["clean"]:
        assert rep[a] == rep[b], (a, b)
    for a, b in s["overlap"]:
        assert rep[a] != rep[b]
    assert counts[1] == len(s["clean"]) == counts[5] and counts[2] >= len(s["overlap"]) and counts[4] > 0      # (the twins)
    check_invariants(s, rep, added, counts, trace)


@pytest.mark.parametrize("seed", [4, 5, 6])
def test_the_invariants_on_a_noisy_scene(seed):
    s = M.scene(np.random.RandomState(seed), 150, [int(x) for x in np.random.RandomState(seed).randint(60, 200, 16)], scales=seed == 5)
    trace = {}
    rep, added, counts = M.fuse(s["pos"], s["desc"], s["frames"], M.FR1_K, 640, 480, trace=trace)
    assert counts[1] > 0 and counts[2] > 0 and counts[3] > 0
    check_invariants(s, rep, added, counts, trace)


def check_invariants(s, rep, added, counts, trace):
    seen, n = trace["seen"], len(s["pos"])
    for comp in trace["members"]:
        union = 0
        for i in comp:
            assert not union & seen[i], "two points with a common frame were merged: %r" % sorted(comp)
            union |= seen[i]
        best = min(comp, key=lambda r: (-popcount(seen[r]), r))
        assert all(rep[i] == best for i in comp)
    gained = {}
    for f, j, p in added.tolist():
        assert rep[p] == p and s["frames"][f]["conn"][j] == -1
        union = 0
        for i in np.nonzero(rep == p)[0]:
            union |= seen[i]
        assert not (union >> f) & 1, "an observation was added in a frame the component is seen in"
        assert (f, p) not in gained, "a component's mask gained bit %d twice" % f
        gained[(f, p)] = j
    assert len({(f, j) for f, j, _ in added.tolist()}) == len(added)
    assert counts[3] == len(added) and counts[5] == (rep != np.arange(n)).sum() == n - len(trace["members"])
    assert counts[1] == counts[5]          # every accepted merge removes one point
