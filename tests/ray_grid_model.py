"""A model of the grid that c2d_poly_ray_casts_grid builds on the device and of the walk of one ray through it, written from DESIGN.md
§5.8 (the grid stages of the broad phase) and §5.16 and from the comments of csrc/c2d_ray_walk.hpp, not from the kernels: plain numpy
float64 (element-wise, unfused, in the written order) and Python integers.

grid_of(box) -> Grid: the extent histogram (bin = float bits >> 21), the cell-size pick, the bounds of the boxes below the pick, x0,
y0, ix, iy, gx, gy with the 65 534 cap, every box's kind (regular / outlier / wild), its key cy(yl) gx + cx(xl), and G.
walk(grid, ray) -> Walk: whether the ray is walked, W, the key rows and each row's key columns (ray_walk_begin and ray_walk_row, step
by step), and the number of sorted regular entries in those ranges — what the walk kernel counts as `visited`, capped as it caps it.
tests/test_ray_grid_walk_cases_cpu.py pins walk() against the header itself, integer for integer and W bit for bit."""
import collections

import numpy as np

F = np.float32
HIST_BINS = 1024
MAX_CELLS = 65535          # cells per axis
WALK_CAP = 1024            # sorted entries a ray may visit before it is listed
REGULAR, OUTLIER, WILD = 0, 1, 2

Grid = collections.namedtuple("Grid", "s x0 y0 ix iy gx gy G kind key in_bounds sorted_keys")
Walk = collections.namedtuple("Walk", "walked W row0 row1 col0 col1 visited")


def _cell(v, v0, inv, g):
    """cell of v: floor((v - v0) * inv) clamped to [0, g - 1] (a NaN goes to 0) -> int64"""
    with np.errstate(invalid="ignore"):
        t = (np.asarray(v, np.float64) - v0) * inv
        t = np.where(t > 0.0, np.floor(t), 0.0)
        top = float(g - 1)
        return np.where(t < top, t, top).astype(np.int64)


def grid_of(box):
    """box: (xl, xh, yl, yh, unboxed) of ray_grid_ref.boxes.  A box with a NaN or an infinite coordinate (an unboxed polygon, an
    infinite vertex, the empty box of a bad count) takes no part in the grid: its kind is WILD."""
    xl, xh, yl, yh = (np.asarray(v, F) for v in box[:4])
    n = len(xl)
    finite = np.isfinite(xl) & np.isfinite(xh) & np.isfinite(yl) & np.isfinite(yh) & ~np.asarray(box[4], bool)
    with np.errstate(all="ignore"):
        extent = np.maximum((xh - xl).astype(F), (yh - yl).astype(F))      # binary32, as the boxes are
    # 1. the extent histogram of the boxed polygons
    bins = extent[finite].view(np.uint32) >> 21
    hist = np.bincount(bins, minlength=HIST_BINS).astype(np.int64)
    # 2. the cell size: the upper edge of the smallest bin with at most max(4, n >> 16) boxes above it
    total = int(hist.sum())
    limit = max(4, total >> 16)
    above = np.concatenate([np.cumsum(hist[::-1])[::-1][1:], [0]])
    best = int(np.flatnonzero(above <= limit)[0])
    s = np.array([(best + 1 if best < 1018 else 1019) << 21], np.uint32).view(F)[0]
    # 3. the bounds of the boxes below the pick
    in_bounds = finite & (extent < s)
    any_in = bool(in_bounds.any())
    x0 = float(xl[in_bounds].min()) if any_in else 0.0
    y0 = float(yl[in_bounds].min()) if any_in else 0.0
    hx = float(xh[in_bounds].max()) if any_in else 0.0
    hy = float(yh[in_bounds].max()) if any_in else 0.0
    ex, ey = hx - x0, hy - y0
    # 4. cells of size s, or larger where the bounds would need more than 65 535 of them
    inv_s = 1.0 / float(s)
    top = float(MAX_CELLS - 1)
    ix = top / ex if ex * inv_s > top else inv_s
    iy = top / ey if ey * inv_s > top else inv_s
    gx, gy = int(np.floor(ex * ix)) + 1, int(np.floor(ey * iy)) + 1
    G = max(abs(x0), abs(hx), abs(y0), abs(hy)) if any_in else 0.0
    # 5. a box that spans more than two cells on an axis is wild; the others are keyed by the cell of their min corner
    cx0, cx1 = _cell(xl, x0, ix, gx), _cell(xh, x0, ix, gx)
    cy0, cy1 = _cell(yl, y0, iy, gy), _cell(yh, y0, iy, gy)
    regular = finite & (cx1 - cx0 <= 1) & (cy1 - cy0 <= 1)
    kind = np.where(regular, np.where(in_bounds, REGULAR, OUTLIER), WILD)
    key = np.where(regular, cy0 * gx + cx0, -1)
    return Grid(float(s), x0, y0, ix, iy, gx, gy, G, kind, key, in_bounds, np.sort(key[regular]))


def _mag(c, v):
    a = abs(v)
    return a if (a > c or a != a) else c


def walk(g, ray):
    """ray: (ox, oy, dx, dy), binary32 values.  Not walked (a non-finite ray, or one with c >= 2^60): Walk(False, ...) with nothing
    else set; the caller tests such a ray against everything."""
    ox, oy, dx, dy = (float(F(v)) for v in ray)
    with np.errstate(all="ignore"):
        bx, by = float(np.float64(ox) + np.float64(dx)), float(np.float64(oy) + np.float64(dy))
    c = _mag(_mag(_mag(_mag(0.0, ox), oy), bx), by)
    if not (c < 2.0 ** 60) or not (abs(dx) < np.inf) or not (abs(dy) < np.inf):
        return Walk(False, None, None, None, None, None, 0)
    W = 3.0 * (2.0 ** -20 * (g.G if g.G > c else c))
    lo = int(_cell(min(oy, by) - W, g.y0, g.iy, g.gy))
    row0 = lo - 1 if lo else 0
    row1 = int(_cell(max(oy, by) + W, g.y0, g.iy, g.gy))
    R = np.arange(row0, row1 + 1, dtype=np.int64)
    xa = np.full(len(R), min(ox, bx))
    xb = np.full(len(R), max(ox, bx))
    if dy != 0.0:
        Rd = R.astype(np.float64)
        with np.errstate(all="ignore"):
            ya = np.where(R == 0, -np.inf, (g.y0 + Rd / g.iy) - W)
            yb = np.where(R + 2 >= g.gy, np.inf, (g.y0 + (Rd + 2.0) / g.iy) + W)
            ta, tb = (ya - oy) / dy, (yb - oy) / dy
            ta = np.where(ta > 0.0, np.where(ta < 1.0, ta, 1.0), 0.0)
            tb = np.where(tb > 0.0, np.where(tb < 1.0, tb, 1.0), 0.0)
            pa, pb = ox + ta * dx, ox + tb * dx
        xa = np.maximum(xa, np.minimum(pa, pb))
        xb = np.minimum(xb, np.maximum(pa, pb))
    lo = _cell(xa - W, g.x0, g.ix, g.gx)
    col0 = np.where(lo > 0, lo - 1, 0)
    col1 = _cell(xb + W, g.x0, g.ix, g.gx)
    seen = np.searchsorted(g.sorted_keys, R * g.gx + col1, "right") - np.searchsorted(g.sorted_keys, R * g.gx + col0, "left")
    return Walk(True, W, row0, row1, col0, col1, min(int(seen.sum()), WALK_CAP))


def in_ranges(w, g, keys):
    """bool per key: the key lies in an enumerated range of the walk"""
    keys = np.asarray(keys, np.int64)
    row, col = keys // g.gx, keys % g.gx
    at = row - w.row0
    ok = (at >= 0) & (row <= w.row1)
    at = np.clip(at, 0, len(w.col0) - 1)
    return ok & (w.col0[at] <= col) & (col <= w.col1[at])
