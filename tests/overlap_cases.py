"""Inputs that the CPU tests of tests/overlap_ref.py and the GPU tests of the overlap queries share (a plain module on numpy only):
the hand-computed cases on a 1/16 grid, where every operation of the rule is exact in binary32, and boxes on a grid as 4-gons and
as rectangle planes."""
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
