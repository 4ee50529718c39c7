"""Scenes for the grid ray query (c2d_poly_ray_casts_grid) built so that the device's grid and walk decide: box corners and ray ends on
cell borders, the 65 535-cell cap on one axis and on both, offsets at which the walk's widening W is a fraction of a cell and several
cells, grids of one and two rows and of one column, rays a few float ulps either side of meets' threshold, and the near-collinear
construction on each of the three routes that evaluate meets.  Inputs only, no hand-written expectations: what the model
(tests/ray_grid_model.py) and the numpy references say of a scene is computed here once per process and shared.  A plain module on numpy.

The polygons of the lattice scenes are five shapes with vertices on multiples of 1/4 and a vertex box of exactly 1 x 1, so every box
falls into the extent bin [1, 1.25): the cell size is 1.25, five lattice steps, and no polygon is wild or an outlier.  All coordinates
of the polygons and of the rays' ends are exact in binary32 at every offset used here."""
import functools
from fractions import Fraction as Fr

import numpy as np

import ray_cases as cases
import ray_grid_cases as gcases
import ray_grid_model as model
import ray_grid_ref as gref
import ray_ref as ref

F = np.float32
Q = 0.25
SHAPES = {
    "square": [(0, 0), (4, 0), (4, 4), (0, 4)],
    "diamond": [(2, 0), (4, 2), (2, 4), (0, 2)],
    "octagon": [(1, 0), (3, 0), (4, 1), (4, 3), (3, 4), (1, 4), (0, 3), (0, 1)],
    "triangle": [(0, 0), (4, 1), (1, 4)],
    "skewed quad": [(0, 0), (3, 1), (4, 4), (1, 3)],
}      # in lattice steps, counter-clockwise
TABLE = ("borders", "cap_x", "cap_xy", "offset_17", "offset_20", "offset_21", "offset_22", "strip_y1", "strip_y2", "strip_x1", "grazing")
EXTRA = ("grazing_skew",)      # beyond the table: holds the third test of meets, sn, at its rounding
COLLINEAR = ("collinear_regular", "collinear_wild", "collinear_listed")
COMPARED_WITH_BRUTE_FORCE = ("cap_x", "cap_xy", "offset_17", "offset_20", "offset_21", "offset_22")
ROWS = 8


def lattice_polys(corners, rng, base=(0.0, 0.0)):
    """one shape per min corner (lattice steps, relative to base): a random shape, a random first vertex, every third one clockwise"""
    names = sorted(SHAPES)
    out = []
    for i, (cx, cy) in enumerate(corners):
        pts = SHAPES[names[int(rng.integers(len(names)))]]
        first = int(rng.integers(len(pts)))
        pts = pts[first:] + pts[:first]
        if i % 3 == 2:
            pts = pts[::-1]
        out.append([(base[0] + Q * (cx + x), base[1] + Q * (cy + y)) for x, y in pts])
    return cases.polys(*out, rows=ROWS)


def lattice_rays(n, rng, lo, hi, corners, base=(0.0, 0.0)):
    """n rays with both ends on the lattice, origins in [lo, hi] (lattice steps per axis) and ends clipped to it: a fifth each
    vertical, horizontal and points, the others oblique with |d| up to 12 per axis; every sixth origin is the middle of a polygon's box"""
    ox = rng.integers(lo[0], hi[0] + 1, n)
    oy = rng.integers(lo[1], hi[1] + 1, n)
    at = rng.integers(len(corners), size=n)
    mid = np.arange(n) % 6 == 5
    ox, oy = np.where(mid, corners[at, 0] + 2, ox), np.where(mid, corners[at, 1] + 2, oy)
    dx, dy = rng.integers(-48, 49, n), rng.integers(-48, 49, n)
    kind = np.arange(n) % 5
    dx = np.where((kind == 0) | (kind == 2), 0, dx)      # 0: vertical, 2: a point
    dy = np.where((kind == 1) | (kind == 2), 0, dy)      # 1: horizontal
    dx = np.clip(ox + dx, lo[0], hi[0]) - ox
    dy = np.clip(oy + dy, lo[1], hi[1]) - oy
    return _planes(ox, oy, dx, dy, base)


def _planes(ox, oy, dx, dy, base=(0.0, 0.0)):
    rays = (base[0] + Q * np.asarray(ox, np.float64), base[1] + Q * np.asarray(oy, np.float64), Q * np.asarray(dx, np.float64), Q * np.asarray(dy, np.float64))
    out = tuple(v.astype(F) for v in rays)
    assert all((a.astype(np.float64) == v).all() for a, v in zip(out, rays)), "a ray coordinate is not exact in binary32"
    return out


def _corners(n, rng, w, h):
    """n min corners on the lattice over w x h units (the boxes reach w and h exactly), the four corners of the area among them"""
    c = np.stack([rng.integers(0, 4 * (w - 1) + 1, n), rng.integers(0, 4 * (h - 1) + 1, n)], axis=1)
    c[:4] = [(0, 0), (4 * (w - 1), 0), (0, 4 * (h - 1)), (4 * (w - 1), 4 * (h - 1))]
    return c


def _exact(b):
    for x in b[:2]:
        assert (np.round(x.astype(np.float64) * 4) == x.astype(np.float64) * 4).all(), "a vertex left the lattice"
    return b


def _field(seed, n, w, h, n_rays, base=(0.0, 0.0), margin=(8, 8, 8, 8)):
    """n polygons over w x h at base and n_rays rays around them (margin: lattice steps beyond the area at x low, x high, y low, y high)"""
    rng = np.random.default_rng(seed)
    c = _corners(n, rng, w, h)
    b = _exact(lattice_polys(c, rng, base))
    rays = lattice_rays(n_rays, rng, (-margin[0], -margin[2]), (4 * w + margin[1], 4 * h + margin[3]), c, base)
    return rays, b


def _join(*parts):
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))


def _join_polys(*sets):
    return tuple(np.concatenate([s[i] for s in sets], axis=-1) for i in range(3))


def _cap(far):
    """two clusters of 300 over 40 x 40, the second at `far`; 200 rays in each cluster, 8 across the whole grid (both ways, between
    opposite corners too) and 40 from the middle of the empty span"""
    r1, b1 = _field(501, 300, 40, 40, 200)
    r2, b2 = _field(502, 300, 40, 40, 200, base=far)
    fx, fy = far
    across = [(0, 0, fx + 40, fy + 40), (fx + 40, fy + 40, -(fx + 40), -(fy + 40)), (0, 40, fx + 40, fy - 40), (fx + 40, fy, -(fx + 40), 40 - fy),
              (20, 20, fx, fy), (fx + 20, fy + 20, -fx, -fy), (0, 20, fx + 40, 0), (fx + 20, fy + 40, 0, -(fy + 40))]
    rng = np.random.default_rng(503)
    mx, my = np.round(fx / 2), np.round(fy / 2)
    middle = [(mx + Q * rng.integers(-40, 41), my + Q * rng.integers(-40, 41), Q * rng.integers(-48, 49) * (i % 3 != 0), Q * rng.integers(-48, 49) * (i % 3 != 1))
              for i in range(40)]
    extra = np.array(across + middle, np.float64)
    planes = tuple(extra[:, i].astype(F) for i in range(4))
    assert all((p.astype(np.float64) == extra[:, i]).all() for i, p in enumerate(planes))
    return _join(r1, r2, planes), _join_polys(b1, b2)


def _offset(k):
    """500 polygons over 60 x 60 whose boxes end at x = 2^k exactly and begin at y = -2^(k-1): the largest magnitude of the bounds is
    2^k, so W = 3 * 2^(k-20) for every ray that stays inside them; no ray end goes beyond x = 2^k"""
    base = (2.0 ** k - 60.0, -(2.0 ** (k - 1)))
    return _field(600 + k, 500, 60, 60, 500, base=base, margin=(8, 0, 8, 8))


def _nudged(v, j):
    """positive binary32 values moved by j units in the last place"""
    return (np.ascontiguousarray(v, F).view(np.int32) + j.astype(np.int32)).view(F)


GRAZING_ULPS = {"horizontal": (-4, 40), "vertical": (-4, 40), "oblique": (-4, 80)}


@functools.lru_cache(maxsize=None)
def _grazing(n=3000):
    """The `borders` polygons and n rays in three kinds, each past a random box q of the set at a signed number of float ulps j:
    horizontal over the top (oy = yh moved by j ulps, from xl - 2 to xl + 2), vertical past xh likewise, and at 45 degrees past the
    corner (xh, yh).  meets' widening m is 2^-20 of the largest magnitude, 8 float ulps of it: the ranges of j straddle it.
    -> (rays, b, q, kind) with kind 0 / 1 / 2 per ray"""
    _, b = scene("borders")
    xl, xh, yl, yh, _ = gref.boxes(b)
    rng = np.random.default_rng(701)
    q = rng.integers(len(xl), size=n)
    kind = np.arange(n) % 3
    j = np.zeros(n, np.int64)
    for i, name in enumerate(("horizontal", "vertical", "oblique")):
        lo, hi = GRAZING_ULPS[name]
        j[kind == i] = rng.integers(lo, hi + 1, int((kind == i).sum()))
    two, four = F(2.0), F(4.0)
    zero = np.zeros(n, F)
    ox = np.select([kind == 0, kind == 1], [xl[q] - two, _nudged(xh[q], j)], xh[q] - two)
    oy = np.select([kind == 0, kind == 1], [_nudged(yh[q], j), yl[q] - two], _nudged(yh[q] + two, j))
    dx = np.select([kind == 0, kind == 1], [zero + four, zero], zero + four)
    dy = np.select([kind == 0, kind == 1], [zero, zero + four], zero - four)
    return tuple(v.astype(F) for v in (ox, oy, dx, dy)), b, q, kind


def _widened(ox, oy, dx, dy, box):
    """the contract's m, hx, hy for one ray and one box, in binary64 as the contract writes them"""
    xl, xh, yl, yh = box
    C = max(abs(v) for v in (ox, oy, ox + dx, oy + dy, xl, xh, yl, yh))
    m = 2.0 ** -20 * C
    return (0.5 * xh - 0.5 * xl) + m, (0.5 * yh - 0.5 * yl) + m


@functools.lru_cache(maxsize=None)
def _grazing_skew(n=600):
    """The `borders` polygons and n long rays of general direction from next to the coordinate origin past a corner of a far box q
    (its lower right or its upper left one), placed so that the two sides of the contract's third test, sn, agree to a few units in
    the last place of binary64.  The ray's own box overlaps q's, so sx and sy are false and sn alone decides.  Its products
    dx (cy - oy) and dy (cx - ox) are some thousand times larger than their difference and not exact in binary64 (an origin of
    1e-6 against a box 10 to 50 away), so how they are rounded decides: a multiply-add in place of a multiply and an add changes
    the outcome for a share of the rays.  Built in three exact steps, each solving sn's equality for one coordinate and rounding it to
    binary32: dx, then oy (about 1e-6), then ox (about 1e-13), and ox moved by up to one and a half units in the last place of the products.
    -> (rays, b, q)"""
    _, b = scene("borders")
    xl, xh, yl, yh, _ = gref.boxes(b)
    rng = np.random.default_rng(702)
    far = np.flatnonzero((xl >= 10) & (yl >= 10))
    q = rng.choice(far, n)
    rows = []
    for i, j in enumerate(q):
        box = tuple(float(v[j]) for v in (xl, xh, yl, yh))
        cx, cy = 0.5 * box[0] + 0.5 * box[1], 0.5 * box[2] + 0.5 * box[3]
        corner = (box[1], box[2]) if i % 2 == 0 else (box[0], box[3])
        reach = rng.uniform(1.05, 1.4)
        dy = float(F(corner[1] * reach))
        dx = float(F(corner[0] * reach))
        ox, oy = 0.0, float(F(rng.uniform(-2e-6, 2e-6)))
        sign = 1 if dx * (cy - oy) - dy * (cx - ox) > 0 else -1

        def rhs():
            hx, hy = _widened(ox, oy, dx, dy, box)
            return Fr(hx) * Fr(abs(dy)), Fr(hy)

        # sign (dx U - dy V) = hx |dy| + hy dx, with U = cy - oy and V = cx - ox
        a, hy = rhs()
        dx = float(F(float((a + sign * Fr(dy) * (Fr(cx) - Fr(ox))) / (sign * (Fr(cy) - Fr(oy)) - hy))))
        a, hy = rhs()
        U = (a + hy * Fr(dx) + sign * Fr(dy) * (Fr(cx) - Fr(ox))) / (sign * Fr(dx))
        oy = float(F(float(Fr(cy) - U)))
        a, hy = rhs()
        V = (sign * Fr(dx) * (Fr(cy) - Fr(oy)) - a - hy * Fr(dx)) / (sign * Fr(dy))
        noise = 2.0 ** -52 * abs(dx * cy) / abs(dy)
        ox = float(F(float(Fr(cx) - V) + rng.uniform(-1.5, 1.5) * noise))
        rows.append((ox, oy, dx, dy))
    return cases.rays_of(*rows), b, q


# ---- the near-collinear construction on each route -------------------------------------------------------------------------------
N_COLLINEAR = 20_000
# Where the copies of the rotated square go, relative to it: all down and to the left of it, none within two units of the line of
# its edge 0 (direction (cos 0.37, sin 0.37)).  The square is then the last box of the bounds in x and in y, so its key lies in the
# last two rows and columns: the cells that the walk of a ray far beyond the bounds on the positive side, clamped, looks at.
COPIES = [(-2.0, -8.0), (-9.0, -1.0), (-5.0, -12.0), (-14.0, -2.0), (-1.0, -6.0), (-11.0, -15.0), (-16.0, -1.5), (-3.0, -14.0), (-7.0, -0.5)]
SMALL = 0.125


def _moved(pts, dx, dy, scale=1.0):
    return [(F(F(x) * F(scale) + F(dx)), F(F(y) * F(scale) + F(dy))) for x, y in pts]


def _collinear(route):
    rays, sq = gcases.near_collinear(n=N_COLLINEAR)
    pts = [(sq[0][e, 0], sq[1][e, 0]) for e in range(4)]
    copies = [_moved(pts, dx, dy) for dx, dy in COPIES]
    if route == "regular":
        return rays, cases.polys(pts, *copies, rows=4)
    if route == "wild":
        hundred = F(100.0)
        return tuple((r * hundred).astype(F) for r in rays), cases.polys(_moved(pts, 0.0, 0.0, 100.0), *copies, rows=4)
    # listed: the rays on the positive side of the square (about half of them), and 1025 small squares inside the rotated square's
    # box, in one of the last cells of the grid: every one of those rays looks at them and goes over the walk's cap
    side = rays[0] > F(0.0)
    last = cases.square(0.5, 1.0, SMALL)
    return tuple(r[side] for r in rays), cases.polys(pts, *copies, *([last] * 1025), rows=4)


@functools.lru_cache(maxsize=None)
def scene(name):
    """name -> (rays, b), read-only"""
    if name == "borders":
        out = _field(401, 600, 50, 50, 450)
    elif name == "cap_x":
        out = _cap((1e5, 5e4))
    elif name == "cap_xy":
        out = _cap((3.0 * 2 ** 20, 3.0 * 2 ** 19))
    elif name.startswith("offset_"):
        out = _offset(int(name[7:]))
    elif name == "strip_y1":
        out = _field(801, 300, 200, 1, 400)
    elif name == "strip_y2":
        out = _field(802, 300, 201, 2, 400)
    elif name == "strip_x1":
        out = _field(803, 300, 1, 201, 400)
    elif name == "grazing":
        out = _grazing()[:2]
    elif name == "grazing_skew":
        out = _grazing_skew()[:2]
    elif name.startswith("collinear_"):
        out = _collinear(name[10:])
    else:
        raise KeyError(name)
    for x in out[0] + tuple(out[1]):
        x.setflags(write=False)
    return out


def grazing_parts():
    """-> (index q of each ray's own box, kind of each ray)"""
    return _grazing()[2:]


@functools.lru_cache(maxsize=None)
def modelled(name):
    """name -> (the model's grid of the scene, the model's walk of every ray)"""
    rays, b = scene(name)
    g = model.grid_of(gref.boxes(b))
    return g, [model.walk(g, r) for r in zip(*rays)]


@functools.lru_cache(maxsize=None)
def grid_records(name):
    """the records of tests/ray_grid_ref.py for the scene, computed once, read-only"""
    want = gref.ray_casts(*scene(name))
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def brute_records(name):
    """the records of tests/ray_ref.py (the brute-force call's contract) for the scene, computed once, read-only"""
    want = ref.ray_casts(*scene(name))
    want.setflags(write=False)
    return want


def collinear_square_hits(name):
    """bool per ray of a collinear scene: the brute-force contract reports a hit on the rotated square (polygon 0)"""
    far = brute_records(name)
    return (far["hit"] == 1) & (far["poly"] == 0)


def grazing_meets_own_box(name="grazing"):
    """bool per ray of `grazing` or `grazing_skew`: the contract's meets against the box q the ray was built past"""
    rays, b = scene(name)
    q = grazing_parts()[0] if name == "grazing" else _grazing_skew()[2]
    box = gref.boxes(b)
    return gref._meets(*[v.astype(np.float64) for v in rays], *[v[q].astype(np.float64) for v in box[:4]])
