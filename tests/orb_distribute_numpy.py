"""TEST AID: the ORB-SLAM style detector of DESIGN.md section 16 (cell-wise FAST with two thresholds, a quadtree spread per
level, the intensity-centroid angle for the kept points), transcribed from the declared arithmetic -- plain numpy and Python
lists, no code shared with csrc/.  The pyramid, the FAST score, the disc moments, fastAtan2 and the per-level quota are the
ones of tests/orb_numpy.py.  Everything up to the angle is integer work, so the device is compared bit for bit
(tests/test_orb_distribute_sim.py, tests/test_gpu_orb_distribute.py); tests/test_orb_distribute_numpy.py holds this file to
answers worked by hand."""
import numpy as np

from orb_numpy import BORDER, F32, KEYPOINT_DTYPE, PATCH, Pyramid, fast_atan2, fast_score_map, feature_quota, moments

DEFAULTS = dict(ini_threshold=20, min_threshold=7, cell_size=30, edge_threshold=19)


# ------------------------------------------------------------------------------------------------ step 1: the cell table
def cell_table(w, h, cell_size=30, edge_threshold=19):
    """Cells of a w x h level as (row i, column j, x0, x1, y0, y1): the scored pixels are [x0, x1) x [y0, y1).  Also returns
    (minX, minY, width, height).  A level too small for one cell has an empty table."""
    W, E = cell_size, edge_threshold
    minX = minY = E - 3
    maxX, maxY = w - E + 3, h - E + 3
    width, height = maxX - minX, maxY - minY
    geom = (minX, minY, width, height)
    if width < W or height < W:          # nCols == 0 or nRows == 0
        return [], geom
    nCols, nRows = width // W, height // W
    wCell, hCell = -(-width // nCols), -(-height // nRows)
    cells = []
    for i in range(nRows):
        iniY = minY + i * hCell
        maxYc = min(iniY + hCell + 6, maxY)
        if iniY >= maxY - 3:
            continue
        for j in range(nCols):
            iniX = minX + j * wCell
            maxXc = min(iniX + wCell + 6, maxX)
            if iniX >= maxX - 6:
                continue
            cells.append((i, j, iniX + 3, maxXc - 3, iniY + 3, maxYc - 3))
    return cells, geom


# ------------------------------------------------------------------------------------------------ steps 2-5: candidates
def cell_survivors(score):
    """Step 3 on the score tile of one cell: >= 1 (the map is already 0 below min_threshold) and strictly greater than the 8
    neighbours, a neighbour outside the tile counting as 0.  Returns (ys, xs) inside the tile, row-major."""
    h, w = score.shape
    p = np.zeros((h + 2, w + 2), np.int64)
    p[1:-1, 1:-1] = score
    keep = score > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= score > p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    return np.nonzero(keep)


def level_candidates(framed, level, ini_threshold=20, min_threshold=7, cell_size=30, edge_threshold=19):
    """Steps 1-5 for one framed level: rows (x, y, level, score) in the order cell row, cell column, y, x."""
    H, Wd = framed.shape
    h, w = H - 2 * BORDER, Wd - 2 * BORDER
    cells, _ = cell_table(w, h, cell_size, edge_threshold)
    out = []
    if not cells:
        return np.zeros((0, 4), np.int64)
    E = edge_threshold
    full = fast_score_map(framed, E, w - E, E, h - E, min_threshold)    # the union of every cell's scored pixels
    for (_, _, x0, x1, y0, y1) in cells:
        if x1 <= x0 or y1 <= y0:
            continue
        tile = full[y0 - E:y1 - E, x0 - E:x1 - E]
        ys, xs = cell_survivors(tile)
        sc = tile[ys, xs]
        strong = sc >= ini_threshold
        if strong.any():                                              # step 4
            ys, xs, sc = ys[strong], xs[strong], sc[strong]
        for y, x, s in zip(ys, xs, sc):
            out.append((x + x0, y + y0, level, s))
    return np.array(out, np.int64).reshape(-1, 4)


# ------------------------------------------------------------------------------------------------ step 6: the quadtree
class _Node:
    __slots__ = ("x0", "x1", "y0", "y1", "idx")

    def __init__(self, x0, x1, y0, y1, idx):
        self.x0, self.x1, self.y0, self.y1, self.idx = x0, x1, y0, y1, idx


def _split(n, xs, ys):
    hx, hy = -(-(n.x1 - n.x0) // 2), -(-(n.y1 - n.y0) // 2)
    mx, my = n.x0 + hx, n.y0 + hy
    boxes = [(n.x0, mx, n.y0, my), (mx, n.x1, n.y0, my), (n.x0, mx, my, n.y1), (mx, n.x1, my, n.y1)]
    idx = [[], [], [], []]
    for i in n.idx:                   # every candidate of the node lies in exactly one of the four boxes
        assert n.x0 <= xs[i] < n.x1 and n.y0 <= ys[i] < n.y1
        idx[(xs[i] >= mx) + 2 * (ys[i] >= my)].append(i)
    return [_Node(*b, k) for b, k in zip(boxes, idx) if k]


def distribute(xs, ys, scores, width, height, N):
    """Step 6 on candidates given RELATIVE to (minX, minY), in candidate order: the indices of the kept ones, in leaf order."""
    xs, ys, scores = [int(v) for v in xs], [int(v) for v in ys], [int(v) for v in scores]
    nIni = max(1, (2 * width + height) // (2 * height))
    nodes = []
    for k in range(nIni):
        a, b = k * width // nIni, (k + 1) * width // nIni
        idx = [i for i in range(len(xs)) if a <= xs[i] < b and 0 <= ys[i] < height]
        if idx:
            nodes.append(_Node(a, b, 0, height, idx))
    assert sum(len(n.idx) for n in nodes) == len(xs)
    while True:
        S = [p for p, n in enumerate(nodes) if len(n.idx) > 1]
        if not S or len(nodes) >= N:
            break
        if len(nodes) + 3 * len(S) <= N:
            new = []
            for n in nodes:
                new.extend(_split(n, xs, ys) if len(n.idx) > 1 else [n])
            nodes = new
            continue
        # the sorted round: positions are those of the round's start, the children take their parent's place afterwards
        kids, length = {}, len(nodes)
        for p in sorted(S, key=lambda p: (-len(nodes[p].idx), p)):
            kids[p] = _split(nodes[p], xs, ys)
            length += len(kids[p]) - 1
            if length >= N:
                break
        nodes = [m for p, n in enumerate(nodes) for m in kids.get(p, [n])]
        if length >= N:
            break
    keep = []
    for n in nodes:
        best = n.idx[0]
        for i in n.idx[1:]:
            if scores[i] > scores[best]:
                best = i
        keep.append(best)
    return keep


# ------------------------------------------------------------------------------------------------ step 8: the grid cap
def grid_select(kps, image_rows, image_cols, grid_size=16, grid_max_per_cell=8, max_keypoints=1500):
    """geometry::selectUniformKptsByGrid: first come first kept, at most grid_max_per_cell per grid cell; stops one past
    max_keypoints."""
    rows, cols = image_rows // grid_size, image_cols // grid_size
    grid = np.zeros((rows, cols), np.int64)
    keep, cnt = [], 0
    for i, k in enumerate(kps):
        r, c = int(k["y"]) // grid_size, int(k["x"]) // grid_size
        assert 0 <= r < rows and 0 <= c < cols
        if grid[r, c] < grid_max_per_cell:
            keep.append(i)
            grid[r, c] += 1
            cnt += 1
            if cnt > max_keypoints:
                break
    return kps[keep]


# ------------------------------------------------------------------------------------------------ the detector
class OrbDistribute:
    def __init__(self, nfeatures=8000, scale_factor=1.2, nlevels=4, pyramid_interpolation=1, grid_size=16,
                 grid_max_per_cell=8, max_keypoints=1500, ini_threshold=20, min_threshold=7, cell_size=30, edge_threshold=19,
                 **_):
        self.nfeatures, self.scale_factor, self.nlevels = nfeatures, scale_factor, nlevels
        self.exact = pyramid_interpolation != 0
        self.grid = dict(grid_size=grid_size, grid_max_per_cell=grid_max_per_cell, max_keypoints=max_keypoints)
        self.dist = dict(ini_threshold=ini_threshold, min_threshold=min_threshold, cell_size=cell_size,
                         edge_threshold=edge_threshold)

    def pyramid(self, img, **gray_kw):
        return Pyramid(img, self.scale_factor, self.nlevels, self.exact, **gray_kw)

    def candidates(self, img, pyr=None, **gray_kw):
        """Step 5: (n, 4) rows (x, y, level, score), level-major."""
        pyr = pyr or self.pyramid(img, **gray_kw)
        return np.concatenate([level_candidates(pyr.raw[l], l, **self.dist) for l in range(self.nlevels)])

    def detect(self, img, pyr=None, cand=None, grid=True, **gray_kw):
        """Steps 1-8: the key points in output order (level-major, leaf order), after the grid cap when `grid`."""
        pyr = pyr or self.pyramid(img, **gray_kw)
        cand = self.candidates(img, pyr) if cand is None else cand
        quota = feature_quota(self.nfeatures, self.scale_factor, self.nlevels)
        E = self.dist["edge_threshold"]
        rows = []
        for l in range(self.nlevels):
            c = cand[cand[:, 2] == l]
            if len(c) == 0:
                continue
            w, h = pyr.sizes[l]
            _, (minX, minY, width, height) = cell_table(w, h, self.dist["cell_size"], E)
            kept = c[distribute(c[:, 0] - minX, c[:, 1] - minY, c[:, 3], width, height, quota[l])]
            m10, m01 = moments(pyr.raw[l], kept[:, 0], kept[:, 1])
            ang = fast_atan2(m01.astype(F32), m10.astype(F32))
            s = pyr.scales[l]
            for k, a in zip(kept, ang):
                rows.append((F32(k[0]) * s, F32(k[1]) * s, F32(PATCH) * s, a, F32(k[3]), l, -1))
        out = np.zeros(len(rows), KEYPOINT_DTYPE)
        for j, r in enumerate(rows):
            out[j] = r
        if grid:
            g = pyr.raw[0]
            out = grid_select(out, g.shape[0] - 2 * BORDER, g.shape[1] - 2 * BORDER, **self.grid)
        return out
