"""Inputs that the CPU tests of tests/overlap_ref.py and the GPU tests of the overlap queries share (a plain module on numpy only):
the hand-computed cases on a 1/16 grid, where every operation of the rule is exact in binary32, boxes on a grid as 4-gons and
as rectangle planes, and the seeded families in which edges of the two shapes lie on one line or nearly so (families())."""
import numpy as np

import overlap_ref as ref

F = np.float32
FIELDS = ("area", "iou", "cx", "cy", "area_a", "area_b", "hit", "flags", "pieces_a", "pieces_b")
THIRD = float(F(0.5) / F(1.5))          # fl(1/3)
MISS = (0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0, ref.NO_CENTROID, 0, 0)
TOUCH = (0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1, ref.NO_CENTROID, 0, 0)


def square(x0, y0, s=1.0, clockwise=False, first=0):
    """the square [x0, x0 + s] x [y0, y0 + s] as a vertex list, counter-clockwise from its lower left corner unless told otherwise"""
    pts = [(x0, y0), (x0 + s, y0), (x0 + s, y0 + s), (x0, y0 + s)]
    pts = pts[first:] + pts[:first]
    return pts[::-1] if clockwise else pts


def poly_set(polys, rows=16, junk=np.nan):
    """vertex lists -> (vx f32[rows][n], vy, k u8[n]) with `junk` in the slots behind each polygon's own vertices"""
    n = len(polys)
    vx, vy, k = np.full((rows, n), junk, F), np.full((rows, n), junk, F), np.zeros(n, np.uint8)
    for c, pts in enumerate(polys):
        k[c] = len(pts)
        vx[:len(pts), c], vy[:len(pts), c] = [p[0] for p in pts], [p[1] for p in pts]
    return vx, vy, k


# name -> (A, B, the record's fields in the order FIELDS)
EXACT = {
    # every edge of A lies on an edge of B that runs the same way: four pieces on A's side, none on B's
    "identical squares": (square(0, 0), square(0, 0), (1.0, 1.0, 0.5, 0.5, 1.0, 1.0, 1, 0, 4, 0)),
    "identical squares, B clockwise": (square(0, 0), square(0, 0, clockwise=True), (1.0, 1.0, 0.5, 0.5, 1.0, 1.0, 1, 0, 4, 0)),
    "identical squares, A clockwise from another corner": (square(0, 0, clockwise=True, first=2), square(0, 0), (1.0, 1.0, 0.5, 0.5, 1.0, 1.0, 1, 0, 4, 0)),
    # the shared side runs opposite ways in the two squares: it is dropped on both sides, and every other edge is clipped to nothing
    "squares sharing a full side": (square(0, 0), square(1, 0), TOUCH),
    "squares sharing a corner": (square(0, 0), square(1, 1), TOUCH),
    # B = A + (1/2, 0): A's bottom and top clipped to [1/2, 1], A's right side whole, B's left side whole: S = 1, M = (9/4, 3/2)
    "half shift": (square(0, 0), square(0.5, 0), (0.5, THIRD, 0.75, 0.5, 1.0, 1.0, 1, 0, 3, 1)),
    "half shift, both clockwise": (square(0, 0, clockwise=True), square(0.5, 0, clockwise=True, first=1), (0.5, THIRD, 0.75, 0.5, 1.0, 1.0, 1, 0, 3, 1)),
    # B = [0, 1/2]^2 inside A, two of its sides on A's: those are A's pieces (clipped to [0, 1/2]), the other two are B's
    "nested square sharing an edge": (square(0, 0), square(0, 0, 0.5), (0.25, 0.25, 0.25, 0.25, 1.0, 0.25, 1, 0, 2, 2)),
    "nested square inside": (square(0, 0, 2.0), square(0.5, 0.5), (1.0, 0.25, 1.0, 1.0, 4.0, 1.0, 1, 0, 0, 4)),
    # the frame is A's vertex 0, so the same shapes far from the origin give the same bits for the area
    "half shift at 100": (square(100, 100), square(100.5, 100), (0.5, THIRD, 100.75, 100.5, 1.0, 1.0, 1, 0, 3, 1)),
    "separated": (square(0, 0), square(3, 0.25), MISS),
    # a repeated vertex of B is a zero-length edge that imposes nothing; one of A is a zero-length piece that adds 0 to the sums
    "repeated vertex in B": (square(0, 0), [(0.5, 0), (1.5, 0), (1.5, 0), (1.5, 1), (0.5, 1), (0.5, 1)], (0.5, THIRD, 0.75, 0.5, 1.0, 1.0, 1, 0, 3, 1)),
    "repeated vertex in A, outside B": ([(0, 0), (0, 0), (1, 0), (1, 1), (0, 1)], square(0.5, 0), (0.5, THIRD, 0.75, 0.5, 1.0, 1.0, 1, 0, 3, 1)),
    # a point or a segment inside a square is hit and has no area
    "k = 1 in A": ([(0.5, 0.5)], square(0, 0), (0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1, ref.DEGENERATE | ref.NO_CENTROID, 0, 0)),
    "k = 2 in B": (square(0, 0), [(0.25, 0.25), (0.75, 0.5)], (0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1, ref.DEGENERATE | ref.NO_CENTROID, 0, 0)),
    "k = 2 in A, separated": ([(3, 3), (4, 3)], square(0, 0), (0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0, ref.NO_CENTROID, 0, 0)),
    "collinear triangle": ([(0.25, 0.25), (0.5, 0.5), (0.75, 0.75)], square(0, 0), (0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1, ref.DEGENERATE | ref.NO_CENTROID, 0, 0)),
}


def exact_sets(junk=np.nan, rows=16):
    """the cases of EXACT as two sets and the diagonal list -> a, b, want (OVERLAP_DT, from the table)"""
    a, b = poly_set([c[0] for c in EXACT.values()], rows, junk), poly_set([c[1] for c in EXACT.values()], rows, junk)
    want = np.zeros(len(EXACT), ref.OVERLAP_DT)
    for q, c in enumerate(EXACT.values()):
        for f, v in zip(FIELDS, c[2]):
            want[f][q] = v
    return a, b, want


def overlapping_grid_boxes(n=1024, seed=8402):
    """axis-aligned boxes on a 1/16 grid, each from a random first corner and in either winding; about a third of the pairs apart, a
    third crossing, the rest nested, equal or sharing sides -> (a, b) as 4-gon sets in 4 rows, (a, b) as planes f32[8][n]"""
    rng = np.random.default_rng(seed)
    g = lambda lo, hi: rng.integers(int(lo * 16), int(hi * 16) + 1, n) / 16.0  # noqa: E731
    x0, y0, wa, ha = g(-4, 4), g(-4, 4), g(0.25, 2), g(0.25, 2)
    kind = rng.integers(0, 6, n)
    bx, by, wb, hb = x0 + g(-2.5, 2.5), y0 + g(-2.5, 2.5), g(0.25, 2), g(0.25, 2)
    bx, by = np.where(kind == 0, x0, bx), np.where(kind == 0, y0, by)                     # equal corners, then equal boxes
    wb, hb = np.where(kind == 0, wa, wb), np.where(kind == 0, ha, hb)
    bx = np.where(kind == 1, x0 + wa, bx)                                                  # side by side
    wb, hb = np.where(kind == 2, wa / 2, wb), np.where(kind == 2, ha / 2, hb)              # nested, sharing a corner
    bx, by = np.where(kind == 2, x0, bx), np.where(kind == 2, y0, by)
    corner = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float64)
    out = []
    for px, py, w, h in ((x0, y0, wa, ha), (bx, by, wb, hb)):
        first, cw = rng.integers(0, 4, n), rng.random(n) < 0.5
        order = np.where(cw[:, None], (first[:, None] - np.arange(4)[None, :]) % 4, (first[:, None] + np.arange(4)[None, :]) % 4)
        c = corner[order]
        out.append(np.stack([px[:, None] + w[:, None] * c[..., 0], py[:, None] + h[:, None] * c[..., 1]], axis=-1).astype(F))
    four = np.full(n, 4, np.uint8)
    polys = [(np.ascontiguousarray(v[..., 0].T), np.ascontiguousarray(v[..., 1].T), four) for v in out]
    planes = [np.ascontiguousarray(v.reshape(n, 8).T) for v in out]
    return polys, planes


# ---- families where two edges of the two shapes lie nearly on one line ---------------------------------------------------------------
def exact_int(v):
    n, d = float(v).as_integer_ratio()          # a binary32 value times 2^149 is an integer
    return n * ((1 << 149) // d)


def convex_as_exact_values(x, y):
    """the binary32 vertices, as exact values, turn one way at every vertex (collinear triples allowed, not all of them)"""
    k = len(x)
    xi, yi = [exact_int(v) for v in x], [exact_int(v) for v in y]
    turns = []
    for i in range(k):
        ax, ay = xi[(i + 1) % k] - xi[i], yi[(i + 1) % k] - yi[i]
        bx, by = xi[(i + 2) % k] - xi[(i + 1) % k], yi[(i + 2) % k] - yi[(i + 1) % k]
        turns.append(ax * by - ay * bx)
    return (all(t >= 0 for t in turns) or all(t <= 0 for t in turns)) and any(t != 0 for t in turns)


def random_convex(rng, cx, cy, scale, kmax=16):
    """3..kmax vertices on an ellipse around (cx, cy) at jittered angles, in either winding, rounded to binary32"""
    k = int(rng.integers(3, kmax + 1))
    theta = (np.arange(k) + rng.uniform(-0.45, 0.45, k)) * (2 * np.pi / k) + rng.uniform(0, 2 * np.pi)
    ra, rb, phi = scale * rng.uniform(0.5, 1.5), scale * rng.uniform(0.5, 1.5), rng.uniform(0, np.pi)
    px, py = ra * np.cos(theta), rb * np.sin(theta)
    x, y = cx + px * np.cos(phi) - py * np.sin(phi), cy + px * np.sin(phi) + py * np.cos(phi)
    if rng.random() < 0.5:
        x, y = x[::-1], y[::-1]
    return x.astype(F), y.astype(F)


def steps32(v, n):
    """the binary32 values v moved by n steps each along the line of binary32 numbers (n an integer array, either sign)"""
    i = np.asarray(v, F).view(np.int32).astype(np.int64)
    o = np.where(i < 0, -(i & 0x7FFFFFFF), i) + n
    return np.where(o < 0, (-o) | 0x80000000, o).astype(np.uint32).view(F)


JITTER_STEPS = (0, 1, 2, 16, 256, 4096, 65536)
FAMILY_OFFSETS = (0.0, 10.0)
PER_OFFSET = 200
BOX_FAMILIES = ("aligned boxes", "nested aligned box")
NEIGHBOURS = ("tiny shift", "tiny rotation", "tiny scaling", "vertex on an edge", "shared vertex", "thin rectangle")


def _centre(rng, offset):
    ox, oy = offset * rng.choice([-1.0, 1.0]), offset * rng.uniform(-1.0, 1.0)
    return ox + rng.uniform(-1, 1), oy + rng.uniform(-1, 1)


def _box(c, th, lo, hi, first=0, clockwise=False):
    """the box {c + s * u + t * v: lo[0] <= s <= hi[0], lo[1] <= t <= hi[1]} (u the axis at angle th, v its left normal), in binary64"""
    u, v = np.array([np.cos(th), np.sin(th)]), np.array([-np.sin(th), np.cos(th)])
    pts = [np.asarray(c) + s * u + t * v for s, t in ((lo[0], lo[1]), (hi[0], lo[1]), (hi[0], hi[1]), (lo[0], hi[1]))]
    pts = pts[first:] + pts[:first]
    pts = pts[::-1] if clockwise else pts
    return np.array([p[0] for p in pts]), np.array([p[1] for p in pts])


def _relist(rng, x, y):
    """the same vertices from another first one, in the other winding"""
    r = int(rng.integers(1, len(x)))
    return np.roll(x, r)[::-1].copy(), np.roll(y, r)[::-1].copy()


def _aligned_boxes(rng, offset, q):
    c, th, L, W = _centre(rng, offset), rng.uniform(0, 2 * np.pi), rng.uniform(0.5, 2), rng.uniform(0.5, 2)
    s = rng.uniform(-0.9, 0.9) * L
    first, cw = ((0, False), (int(rng.integers(1, 4)), False), (int(rng.integers(0, 4)), True))[q % 3]      # the same order, another corner, the other winding
    a = _box(c, th, (-L / 2, -W / 2), (L / 2, W / 2))
    b = _box(c, th, (-L / 2 + s, -W / 2), (L / 2 + s, W / 2), first, cw)
    inter = (L - abs(s)) * W
    return a, b, inter, inter / (2 * L * W - inter)


def _nested_box(rng, offset, q):
    c, th, L, W = _centre(rng, offset), rng.uniform(0, 2 * np.pi), rng.uniform(0.5, 2), rng.uniform(0.5, 2)
    half = np.array([L / 2, W / 2])
    lo, hi = -half * rng.uniform(0.1, 0.9, 2), half * rng.uniform(0.1, 0.9, 2)
    side = int(rng.integers(0, 4))               # the side of A that the inner box lies on
    if side < 2:
        lo[side] = -half[side]
    else:
        hi[side - 2] = half[side - 2]
    a = _box(c, th, -half, half, int(rng.integers(0, 4)), rng.random() < 0.5)
    b = _box(c, th, lo, hi, int(rng.integers(0, 4)), rng.random() < 0.5)
    inter = float(np.prod(hi - lo))
    return a, b, inter, inter / (L * W)


def _triangle_on_an_edge(rng, offset, q):
    c = _centre(rng, offset)
    ax, ay = random_convex(rng, *c, 1.0)
    i = int(rng.integers(0, len(ax)))
    j = (i + 1) % len(ax)
    t = rng.uniform(-0.3, 1.3, 2)
    bx = np.array([ax[i] + t[0] * (float(ax[j]) - ax[i]), ax[i] + t[1] * (float(ax[j]) - ax[i]), c[0]], np.float64)
    by = np.array([ay[i] + t[0] * (float(ay[j]) - ay[i]), ay[i] + t[1] * (float(ay[j]) - ay[i]), c[1]], np.float64)
    if rng.random() < 0.5:
        bx, by = bx[::-1], by[::-1]
    return (ax, ay), (bx, by), None, None


def _jittered(k):
    """(65 536 steps at a coordinate of 10 are 1/16: more than a 16-gon's vertices stand out from their neighbours' chord, so the
    shapes of that family have at most 6 vertices, which keeps the share left out as not convex under 5 %)"""
    def draw(rng, offset, q):
        ax, ay = random_convex(rng, *_centre(rng, offset), 1.0, 16 if k < 65536 else 6)
        bx, by = (ax, ay) if q % 2 == 0 else _relist(rng, ax, ay)
        return (ax, ay), (steps32(bx, rng.integers(-k, k + 1, len(bx))), steps32(by, rng.integers(-k, k + 1, len(by)))), None, None
    return draw


def _tiny_shift(rng, offset, q):
    ax, ay = random_convex(rng, *_centre(rng, offset), 1.0)
    d, th = 10.0 ** rng.uniform(-8, -3), rng.uniform(0, 2 * np.pi)
    return (ax, ay), (ax + d * np.cos(th), ay + d * np.sin(th)), None, None


def _tiny_rotation(rng, offset, q):
    c = _centre(rng, offset)
    ax, ay = random_convex(rng, *c, 1.0)
    th = 10.0 ** rng.uniform(-8, -3) * rng.choice([-1.0, 1.0])
    dx, dy = ax - c[0], ay - c[1]
    return (ax, ay), (c[0] + dx * np.cos(th) - dy * np.sin(th), c[1] + dx * np.sin(th) + dy * np.cos(th)), None, None


def _tiny_scaling(rng, offset, q):
    c = _centre(rng, offset)
    ax, ay = random_convex(rng, *c, 1.0)
    s = 1.0 + 10.0 ** rng.uniform(-7, -2) * rng.choice([-1.0, 1.0])
    return (ax, ay), (c[0] + s * (ax - c[0]), c[1] + s * (ay - c[1])), None, None


def _vertex_on_an_edge(rng, offset, q):
    c = _centre(rng, offset)
    ax, ay = random_convex(rng, *c, 1.0)
    bx, by = random_convex(rng, c[0] + rng.uniform(-1, 1), c[1] + rng.uniform(-1, 1), 1.0)
    i, j, t = int(rng.integers(0, len(ax))), int(rng.integers(0, len(bx))), rng.uniform(0, 1)
    i1 = (i + 1) % len(ax)
    px, py = ax[i] + t * (float(ax[i1]) - ax[i]), ay[i] + t * (float(ay[i1]) - ay[i])
    return (ax, ay), (bx + (px - bx[j]), by + (py - by[j])), None, None


def _shared_vertex(rng, offset, q):
    c = _centre(rng, offset)
    ax, ay = random_convex(rng, *c, 1.0)
    bx, by = random_convex(rng, c[0] + rng.uniform(-1, 1), c[1] + rng.uniform(-1, 1), 1.0)
    i, j = int(rng.integers(0, len(ax))), int(rng.integers(0, len(bx)))
    bx, by = (bx + (float(ax[i]) - bx[j])).astype(F), (by + (float(ay[i]) - by[j])).astype(F)
    bx[j], by[j] = ax[i], ay[i]
    return (ax, ay), (bx, by), None, None


def _thin_rectangle(rng, offset, q):
    c = _centre(rng, offset)
    ax, ay = random_convex(rng, *c, 1.0)
    h = 10.0 ** rng.uniform(-6, -2)
    mid = (c[0] + rng.uniform(-0.3, 0.3), c[1] + rng.uniform(-0.3, 0.3))
    return (ax, ay), _box(mid, rng.uniform(0, 2 * np.pi), (-2.0, -h), (2.0, h), int(rng.integers(0, 4)), rng.random() < 0.5), None, None


def _family_draws():
    draws = {"aligned boxes": _aligned_boxes, "nested aligned box": _nested_box, "triangle on an edge": _triangle_on_an_edge}
    draws.update({f"equal shapes, {k} steps": _jittered(k) for k in JITTER_STEPS})
    draws.update(zip(NEIGHBOURS, (_tiny_shift, _tiny_rotation, _tiny_scaling, _vertex_on_an_edge, _shared_vertex, _thin_rectangle)))
    return draws


class Family:
    """one family's kept pairs: a, b as polygon sets in 16 rows (pair q is column q of both), the centre offset of each pair, the
    share of the draws left out as not convex; for the box families also the planes f32[8][n] and the analytic area and IoU of the
    boxes as drawn (binary64, before the vertices were rounded to binary32) with L + W of the larger box"""

    def __init__(self, name, pairs, offsets, left_out, analytic):
        self.name, self.offsets, self.left_out = name, np.array(offsets), left_out
        self.a, self.b = poly_set([list(zip(*p[0])) for p in pairs]), poly_set([list(zip(*p[1])) for p in pairs])
        self.n = len(pairs)
        self.planes = self.area = self.iou = None
        if name in BOX_FAMILIES:
            self.planes = tuple(np.ascontiguousarray(np.stack([s[v % 2][v // 2] for v in range(8)])) for s in (self.a, self.b))
            self.area, self.iou = np.array([x[0] for x in analytic]), np.array([x[1] for x in analytic])


U = 2.0 ** -24


def analytic_tolerances(f, q, c_area):
    """how far the area and the IoU of binary32 boxes may lie from the analytic values of the boxes as drawn.  Rounding moves each
    coordinate by at most u |x|, so each vertex by at most d = sqrt(2) u M (M the pair's largest |coordinate|) and each box stays
    within Hausdorff distance d of itself; the area of the intersection then moves by at most (perimeter_A + perimeter_B) d (plus
    terms in d^2: the factor 1.01).  On top comes the rule's own c_area u D^2.  The IoU is I / (A + B - I): an error e in each of
    the three areas moves it by at most 4 e / (A + B - I), and its own operations by a few u."""
    ax, ay, bx, by = (np.asarray(v[:4, q], np.float64) for v in (f.a[0], f.a[1], f.b[0], f.b[1]))
    M = max(np.abs(v).max() for v in (ax, ay, bx, by))
    D = max(np.abs(v - r).max() for v, r in ((ax, ax[0]), (ay, ay[0]), (bx, ax[0]), (by, ay[0])))
    perimeter = sum(np.hypot(np.roll(x, -1) - x, np.roll(y, -1) - y).sum() for x, y in ((ax, ay), (bx, by)))
    tol = c_area * U * D * D + 1.01 * perimeter * np.sqrt(2.0) * U * M
    union = f.area[q] / f.iou[q]
    return tol, 4 * tol / union + 4 * U


def check_against_the_analytic_boxes(f, got, c_area, what):
    """the records of a box family against the analytic area and IoU, within analytic_tolerances(); -> the worst shares of them used"""
    worst_area = worst_iou = 0.0
    for q in range(f.n):
        tol_area, tol_iou = analytic_tolerances(f, q, c_area)
        worst_area = max(worst_area, abs(float(got["area"][q]) - f.area[q]) / tol_area)
        worst_iou = max(worst_iou, abs(float(got["iou"][q]) - f.iou[q]) / tol_iou)
    print(what, "worst |area - analytic| / tolerance", worst_area, "worst |iou - analytic| / tolerance", worst_iou)
    assert worst_area <= 1 and worst_iou <= 1, (what, worst_area, worst_iou)
    return worst_area, worst_iou


_FAMILIES = {}


def families():
    """name -> Family, every one from its own seeded stream, PER_OFFSET draws at each centre offset of FAMILY_OFFSETS"""
    if not _FAMILIES:
        for index, (name, draw) in enumerate(_family_draws().items()):
            rng = np.random.default_rng([2601, index])
            pairs, offsets, analytic, out = [], [], [], 0
            for offset in FAMILY_OFFSETS:
                for q in range(PER_OFFSET):
                    a, b, area, iou = draw(rng, offset, q)
                    a, b = tuple(np.asarray(v, np.float64).astype(F) for v in a), tuple(np.asarray(v, np.float64).astype(F) for v in b)
                    if convex_as_exact_values(*a) and convex_as_exact_values(*b):
                        pairs.append((a, b))
                        offsets.append(offset)
                        analytic.append((area, iou))
                    else:
                        out += 1
            _FAMILIES[name] = Family(name, pairs, offsets, out / (len(FAMILY_OFFSETS) * PER_OFFSET), analytic)
    return _FAMILIES
