"""Known answers for tests/orb_distribute_numpy.py, the transcription of the ORB-SLAM style detector:
cell tables, the two thresholds, the suppression at cell borders and the quadtree, each worked by hand in the comments, and the
property the detector exists for on the low-contrast frame.  No GPU and no device code."""
import numpy as np

import orb_distribute_numpy as D
import orb_numpy as N
from test_gpu_orb_distribute import texture_frame


# ------------------------------------------------------------------------------------------------ step 1
def test_cell_table_of_exactly_one_cell_and_of_none():
    # 62 x 62, E = 19: min = 16, max = 46, width = height = 30 -> 1 x 1 cells of 30; ini = 16, maxc = min(16 + 36, 46) = 46:
    # scored [19, 43) both ways
    cells, geom = D.cell_table(62, 62)
    assert geom == (16, 16, 30, 30) and cells == [(0, 0, 19, 43, 19, 43)]
    # one column less: width 29 < 30 -> no column of cells, no key points, no error
    assert D.cell_table(61, 62)[0] == [] and D.cell_table(62, 61)[0] == []
    assert D.cell_table(20, 20)[0] == []            # (width negative)
    # E = 31: 86 - 62 + 6 = 30
    assert D.cell_table(86, 86, edge_threshold=31)[0] == [(0, 0, 31, 55, 31, 55)]
    assert D.cell_table(85, 86, edge_threshold=31)[0] == []


def test_cell_table_with_a_clamped_last_cell():
    # 93 x 70: width 61 -> 2 columns of ceil(61 / 2) = 31; height 38 -> 1 row of 38.  Column 0: ini 16, maxc 16 + 37 = 53 ->
    # [19, 50); column 1: ini 47 < maxX - 6 = 71, maxc = min(84, 77) = 77 (clamped) -> [50, 74).  Row: [19, min(60, 54) - 3 = 51)
    cells, geom = D.cell_table(93, 70)
    assert geom == (16, 16, 61, 38)
    assert cells == [(0, 0, 19, 50, 19, 51), (0, 1, 50, 74, 19, 51)]


def test_cell_table_with_a_cell_skipped_by_the_border_rules():
    # the last column is skipped when (nCols - 1) wCell >= width - 6.  With wCell = ceil(width / nCols) that needs many narrow
    # columns: cell_size 8, w = 65: width 33 -> 4 columns of 9, the last starts at 16 + 27 = 43 = maxX - 6 -> skipped; the third
    # is clamped: maxc = min(34 + 15, 49) = 49
    cells, _ = D.cell_table(65, 62, cell_size=8)
    assert sorted({c[1] for c in cells}) == [0, 1, 2]
    assert [c[2:4] for c in cells if c[0] == 0] == [(19, 28), (28, 37), (37, 46)]
    # at the default cell size the first such width is 813: width 781 -> 26 columns of 31, 25 * 31 = 775 = 781 - 6
    cells, _ = D.cell_table(813, 62)
    assert len(cells) == 25 and cells[-1][1] == 24 and cells[-1][3] == 813 - 19
    assert len(D.cell_table(812, 62)[0]) == 26
    # rows: skipped when (nRows - 1) hCell >= height - 3.  cell_size 8, w = 62: 3 columns of 10, the last scores [39, 43).
    # h = 89: height 57 -> 7 rows of 9, the last starts at 16 + 54 = 70 = maxY - 3 -> skipped; row 5 starts at 61 and is clamped
    # at 73: it scores [64, 70)
    cells, _ = D.cell_table(62, 89, cell_size=8)
    assert sorted({c[0] for c in cells}) == [0, 1, 2, 3, 4, 5] and cells[-1] == (5, 2, 39, 43, 64, 70)
    # h = 67: height 35 -> 4 rows of 9, the last starts at 43 < 51 - 3 and scores the two rows [46, 48)
    assert D.cell_table(62, 67, cell_size=8)[0][-1] == (3, 2, 39, 43, 46, 48)
    # h = 65: height 33 -> 4 rows of 9, the last starts at 43 < 49 - 3: it stays in the table with no scored row, [46, 46)
    assert D.cell_table(62, 65, cell_size=8)[0][-1] == (3, 2, 39, 43, 46, 46)


def test_cell_table_of_a_640_x_480_level():
    # width 608 -> 20 columns of 31, height 448 -> 14 rows of 32; the cells of a row tile [19, 621) without gap or overlap
    cells, geom = D.cell_table(640, 480)
    assert geom == (16, 16, 608, 448) and len(cells) == 280
    row0 = [c for c in cells if c[0] == 0]
    assert row0[0][2] == 19 and row0[-1][2:4] == (608, 621)
    assert all(a[3] == b[2] for a, b in zip(row0, row0[1:]))
    col0 = [c for c in cells if c[1] == 0]
    assert col0[0][4] == 19 and col0[-1][4:6] == (435, 461) and all(a[5] == b[4] for a, b in zip(col0, col0[1:]))
    # every cell fits the device's tile: fewer than 2 * cell_size scored pixels each way
    assert max(c[3] - c[2] for c in cells) == 31 and max(c[5] - c[4] for c in cells) == 32


# ------------------------------------------------------------------------------------------------ steps 2-5
def dots(w, h, spec, base=100):
    """A flat image with single bright pixels: a pixel brighter than its whole FAST circle by c has score c - 1, and no other
    pixel becomes a corner (one circle pixel differs)."""
    img = np.full((h, w), base, np.uint8)
    for x, y, c in spec:
        img[y, x] = base + c
    return N.with_frame(img)


def cand(framed, **kw):
    return [tuple(int(v) for v in r) for r in D.level_candidates(framed, 0, **kw)]


def test_a_cell_with_a_strong_corner_keeps_only_its_strong_corners():
    # 93 x 70: cell 0 scores x in [19, 50), cell 1 x in [50, 74).  Cell 0 holds scores 39 and 9 -> the 9 is dropped; cell 1 holds
    # 9 and 7 only -> both kept (7 = min_threshold exactly), a score of 6 is never a candidate
    f = dots(93, 70, [(30, 25, 40), (40, 40, 10), (60, 30, 10), (65, 45, 8), (70, 22, 7)])
    assert cand(f) == [(30, 25, 0, 39), (60, 30, 0, 9), (65, 45, 0, 7)]
    # score 20 = ini_threshold exactly counts as strong; 19 does not
    assert cand(dots(93, 70, [(30, 25, 21), (40, 40, 20)])) == [(30, 25, 0, 20)]
    assert cand(dots(93, 70, [(30, 25, 20), (40, 40, 19)])) == [(30, 25, 0, 19), (40, 40, 0, 18)]
    # candidate order: cell column before y before x
    f = dots(93, 70, [(60, 20, 30), (25, 40, 30), (45, 21, 30), (21, 21, 30)])
    assert cand(f) == [(21, 21, 0, 29), (45, 21, 0, 29), (25, 40, 0, 29), (60, 20, 0, 29)]
    # pixels outside the scored range are never candidates: x = 18 and x = 74 lie in the edge strip
    assert cand(dots(93, 70, [(18, 30, 50), (74, 30, 50), (30, 18, 50), (30, 51, 50)])) == []


def test_touching_maxima_survive_across_a_cell_border_only():
    # inside cell 0 the weaker of two touching corners is suppressed, and two equal ones suppress each other (strict >)
    assert cand(dots(93, 70, [(30, 30, 30), (31, 30, 31)])) == [(31, 30, 0, 30)]
    assert cand(dots(93, 70, [(30, 30, 30), (31, 31, 30)])) == []
    # x = 49 is the last scored column of cell 0, x = 50 the first of cell 1: a neighbour outside the cell counts as 0
    assert cand(dots(93, 70, [(49, 30, 30), (50, 30, 31)])) == [(49, 30, 0, 29), (50, 30, 0, 30)]
    assert cand(dots(93, 70, [(49, 30, 30), (50, 31, 30)])) == [(49, 30, 0, 29), (50, 31, 0, 29)]


# ------------------------------------------------------------------------------------------------ step 6
def spread(c, width, height, n):
    c = np.array(c).reshape(-1, 3)
    return D.distribute(c[:, 0], c[:, 1], c[:, 2], width, height, n)


def test_quadtree_initial_nodes_of_a_two_to_one_level():
    # nIni = (2 * 200 + 100) / (2 * 100) = 2: strips [0, 100) and [100, 200), kept in strip order whatever the candidate order
    assert spread([(150, 20, 7), (10, 10, 5)], 200, 100, 5) == [1, 0]
    assert spread([(99, 20, 7), (100, 10, 5)], 200, 100, 5) == [0, 1]
    # 199 x 100: (398 + 100) / 200 = 2 still; 149 x 100: (298 + 100) / 200 = 1
    assert spread([(120, 20, 7), (10, 10, 9)], 149, 100, 1) == [1]


def test_quadtree_tie_on_score_and_a_quota_already_met():
    # N = 1: the list has 1 >= N nodes before any split; the leaf gives its best score, the first in candidate order on a tie
    assert spread([(10, 10, 5), (80, 80, 5)], 100, 100, 1) == [0]
    assert spread([(10, 10, 5), (80, 80, 9)], 100, 100, 1) == [1]
    assert spread([(10, 10, 5), (80, 80, 9), (50, 50, 9)], 100, 100, 0) == [1]
    assert spread([], 100, 100, 10) == []


def test_quadtree_candidates_that_stay_together_through_several_splits():
    # 64 x 64, (0, 0) and (1, 1): the halves 32, 16, 8, 4, 2 keep both in the first child, the split of [0, 2) x [0, 2) parts them
    assert spread([(0, 0, 1), (1, 1, 2)], 64, 64, 2) == [0, 1]
    # a third candidate leaves in the first split (fourth child); the leaf order follows the list, not the scores
    assert spread([(40, 40, 9), (0, 0, 1), (1, 1, 2)], 64, 64, 3) == [1, 2, 0]
    # odd extents: 63 -> hx = 32: x = 31 goes left, x = 32 goes right
    assert spread([(32, 0, 1), (31, 0, 2)], 63, 63, 2) == [1, 0]


QUADS = [(5, 5, 10), (60, 10, 3), (30, 5, 11), (10, 60, 9), (90, 40, 8), (5, 30, 12), (70, 70, 1), (40, 90, 2)]


def test_quadtree_quota_reached_in_the_middle_of_a_sorted_round():
    # 100 x 100.  Round 1: 1 + 3 <= N -> split all: A = [0, 50)^2 {0, 2, 5}, B = [50, 100) x [0, 50) {1, 4}, C = [0, 50) x
    # [50, 100) {3, 7}, D {6}.  Round 2: 4 + 3 * 3 > N -> sorted A (3), B (2, position 1), C (2, position 2).  A splits at 25 into
    # {0}, {2}, {5}: 6 leaves.
    # N = 6: reached after A; B and C stay whole and give their best scores (4: 8 > 3, 3: 9 > 2)
    assert spread(QUADS, 100, 100, 6) == [0, 2, 5, 4, 3, 6]
    # N = 7: B splits too ({1} in [50, 75) x [0, 25), {4} in [75, 100) x [25, 50)): 7 leaves, C stays whole
    assert spread(QUADS, 100, 100, 7) == [0, 2, 5, 1, 4, 3, 6]
    # N = 8: C splits too ({3}, {7}): every candidate its own leaf
    assert spread(QUADS, 100, 100, 8) == [0, 2, 5, 1, 4, 3, 7, 6]
    # N = 5: round 2 starts at 4 < 5, A's split overshoots to 6 = N + 1
    assert spread(QUADS, 100, 100, 5) == [0, 2, 5, 4, 3, 6]
    # N = 4: 1 + 3 <= 4 -> split all, then 4 >= N stops: the four quadrants' best (A: 12 at index 5)
    assert spread(QUADS, 100, 100, 4) == [5, 4, 3, 6]
    # equal counts are split in list order: with A reduced to two candidates, A (position 0) still goes before B and C
    assert spread(QUADS[:5] + QUADS[6:], 100, 100, 5) == [0, 2, 4, 3, 5]


def test_quadtree_can_leave_two_more_leaves_than_the_quota():
    # 200 x 100, N = 3: strips {0, 1, 2, 3} and {4}; 2 + 3 > 3 -> sorted: the first strip splits into four: 5 = N + 2 leaves
    c = [(10, 10, 1), (60, 10, 2), (10, 60, 3), (60, 60, 4), (150, 50, 5)]
    assert spread(c, 200, 100, 3) == [0, 1, 2, 3, 4]


# ------------------------------------------------------------------------------------------------ step 8
def test_grid_select_is_a_cap():
    k = np.zeros(5, N.KEYPOINT_DTYPE)
    k["x"], k["y"] = [1, 2, 3, 40, 4], [1, 2, 3, 40, 4]
    assert D.grid_select(k, 64, 64, 16, 2, 100)["x"].tolist() == [1, 2, 40]
    assert D.grid_select(k, 64, 64, 16, 8, 2)["x"].tolist() == [1, 2, 3]       # one past max_keypoints, as the reference
    assert D.grid_select(k, 64, 64, 16, 8, 100).tobytes() == k.tobytes()


# ------------------------------------------------------------------------------------------------ what the detector is for
def test_low_contrast_frame_gets_more_and_better_spread_keypoints(mvo):
    img = texture_frame(mvo, True)
    p = dict(nfeatures=2000, scale_factor=1.2, nlevels=4)
    old = N.Orb(fast_threshold=20, **p).detect(img)
    det = D.OrbDistribute(**p)
    pyr = det.pyramid(img)
    c = det.candidates(img, pyr)
    new = det.detect(img, pyr, c, grid=False)
    print("low-contrast 640 x 480 frame: %d key points (existing detector at threshold 20), %d candidates, %d key points "
          "(cell-wise FAST 20 / 7 + quadtree)" % (len(old), len(c), len(new)))
    assert len(new) > len(old)
    # the image cut into 4 x 4 blocks of 160 x 120: every block with a candidate has a key point
    s = np.array([float(v) for v in pyr.scales])
    bc = set(zip((c[:, 0] * s[c[:, 2]] // 160).astype(int), (c[:, 1] * s[c[:, 2]] // 120).astype(int)))
    bk = set(zip((new["x"] // 160).astype(int), (new["y"] // 120).astype(int)))
    assert bc == bk and len(bc) == 16
    # cv::ORB::compute's 31-px filter then takes the key points of the outer strip (deviation 5)
    kept, _ = N.Orb(**p).compute(img, new)
    print("after the 31-px filter of the descriptor stage: %d of %d" % (len(kept), len(new)))
    assert len(old) < len(kept) < len(new)
