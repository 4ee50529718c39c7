"""CPU tests that pin tests/distance_ref.py — the numpy restatement of the distance contract of include/c2d.h that the GPU tests
compare c2d_poly_pair_distances / c2d_rect_pair_distances with — on hand-computed cases whose expected values are exact in binary32
and on properties of the dense sets of tests/contact_cases.py (300 x 311 polygons, all 93 300 pairs; the GPU tests run the same
batch): against contact_ref's depth, against the polygons' own boundaries and against a float64 brute force."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contact_cases as cases  # noqa: E402
import contact_ref  # noqa: E402
import distance_ref as ref  # noqa: E402

F = np.float32
FIELDS = ("dist", "ax", "ay", "bx", "by", "edge", "vert", "hit", "flags")
SQRT2 = float(np.sqrt(F(2)))
HIT = (0.0, 0.0, 0.0, 0.0, 0.0, 0xFFFF, 0xFFFF, 1, 0)


def poly(*pts):
    """one polygon as a set of one: (vx [16][1], vy, k)"""
    vx, vy = np.zeros((16, 1), F), np.zeros((16, 1), F)
    for r, (x, y) in enumerate(pts):
        vx[r, 0], vy[r, 0] = x, y
    return vx, vy, np.array([len(pts)], np.uint8)


def square(x0, y0, s=1.0):
    return poly((x0, y0), (x0 + s, y0), (x0 + s, y0 + s), (x0, y0 + s))


def one(a, b):
    d = ref.poly_distances(a, b, [0], [0])[0]
    assert d["reserved0"] == 0 and d["reserved1"] == 0
    return tuple(d[f].item() for f in FIELDS)


TRIANGLE = ((2, 5), (3, 7), (1, 7))       # counter-clockwise, its lowest vertex first


def test_boxes_face_to_face_the_first_of_the_ties_wins():
    """A = [0, 1]^2, B = A + (1.25, 0).  Side 0, edge 0 of A, (0, 0) -> (1, 0), against B's vertex 0 = (1.25, 0): s = 1.25 >= len2 = 1,
    region 1, the closest point is (1, 0) and d2 = 1/16.  Edge 1 reaches the same d2 from (1.25, 0) in region 0 and from (1.25, 1) in
    region 1, and B's edge 3 reaches it from A's vertices 1 and 2 in regions 1 and 0, all with the same bits: none replaces the first."""
    assert one(square(0, 0), square(1.25, 0)) == (0.25, 1.0, 0.0, 1.25, 0.0, 0, 0, 0, 0)


def test_boxes_diagonal_vertex_to_vertex():
    """B = A + (2, 2): the first candidate is edge 0 against (2, 2) with d2 = 5; edge 1, (1, 0) -> (1, 1), reaches (1, 1) in region 1
    (s = 2 >= 1) with d2 = 2 and takes over; edge 2 reaches the same vertex in region 0 and ties.  B = A - (2, 2): edge 0 against
    B's vertex 2 = (-1, -1) has s = -1 <= 0, region 0, the closest point is (0, 0), d2 = 2, and everything later ties or loses."""
    assert one(square(0, 0), square(2, 2)) == (SQRT2, 1.0, 1.0, 2.0, 2.0, 1, 0, 0, 0)
    assert one(square(0, 0), square(-2, -2)) == (SQRT2, 0.0, 0.0, -1.0, -1.0, 0, 2, 0, 0)


def test_vertex_over_the_middle_of_an_edge():
    """A = [0, 4]^2, B a triangle whose vertex 0 = (2, 5) hangs one unit over the middle of A's edge 2, (4, 4) -> (0, 4): q = (-2, 1),
    s = 8, len2 = 16, t = 1/2, the closest point (4 + t * -4, 4 + t * 0) = (2, 4), d2 = 1.  Before it: edge 0 gives 25 (t = 1/2),
    edge 1 gives 5 at (4, 4) in region 1.  No candidate of side 1 comes below 5."""
    assert one(square(0, 0, 4.0), poly(*TRIANGLE)) == (1.0, 2.0, 4.0, 2.0, 5.0, 2, 0, 0, ref.INTERIOR)


def test_the_same_with_a_and_b_swapped():
    """The triangle's own edges stay at d2 = 5 (reached first by its edge 0 against the box's vertex 2, region 0); side 1 finds the
    box's edge 2 against the triangle's vertex 0: the vertex is now A's point, the closest point B's."""
    assert one(poly(*TRIANGLE), square(0, 0, 4.0)) == (1.0, 2.0, 5.0, 2.0, 4.0, 2, 0, 0, ref.EDGE_ON_B | ref.INTERIOR)


def test_single_points_are_hit():
    """k = 1 against k = 1: the pairwise test has zero-length axes only, which never separate, so hit = 1 and the record is the hit
    record whatever the two points are.  One point (0.5, -2) against the unit box is separated by the box's axes: the point's only
    edge is (p -> p), len2 = 0, region 0, d2 = 4.25 against (0, 0) and (1, 0); then the box's edge 0 finds the point in region 2
    (t = 1/2) at d2 = 4."""
    assert one(poly((0, 0)), poly((3, 4))) == HIT
    assert one(poly((0.5, -2)), square(0, 0)) == (2.0, 0.5, -2.0, 0.5, 0.0, 0, 0, 0, ref.EDGE_ON_B | ref.INTERIOR)


def test_two_vertices_against_a_box():
    """A = the segment (0, 0) -> (2, 0) as a 2-gon, B = [0.5, 1.5] x [1, 2].  Edge 0 against B's vertex 0 = (0.5, 1): s = 1, t = 1/4,
    the closest point (0.5, 0), d2 = 1; B's vertex 1 ties at (1.5, 0); the closing edge 1, (2, 0) -> (0, 0), reaches both again and
    ties."""
    assert one(poly((0, 0), (2, 0)), square(0.5, 1)) == (1.0, 0.5, 0.0, 0.5, 1.0, 0, 0, 0, ref.INTERIOR)


def test_clockwise_polygon():
    """A = the unit box listed clockwise, (0, 0), (0, 1), (1, 1), (1, 0); B = [1.25, 2.25] x [0, 1].  Edge 0 (the left side) gives
    1.5625; edge 1, (0, 1) -> (1, 1), gives 1.0625 against (1.25, 0) and then 1/16 against B's vertex 3 = (1.25, 1) in region 1;
    edge 2 ties."""
    assert one(poly((0, 0), (0, 1), (1, 1), (1, 0)), square(1.25, 0)) == (0.25, 1.0, 1.0, 1.25, 1.0, 1, 3, 0, 0)


def test_hit_pair():
    assert one(square(0, 0), square(0.5, 0.5)) == HIT
    assert one(square(0, 0), square(1, 0)) == HIT          # touching is hit (strict <)


def test_nan_and_infinite_pairs():
    """All coordinates NaN: no axis has ordered first projections, so hit = 1 and the record is the hit record.  NO_CANDIDATE needs a
    pair that the pairwise test separates and whose every d2 is NaN: A's edges are (1, -1), (-1, 2), (0, -1) and B is the single
    point (inf, inf) — A's axis (1, 1) separates (1 < inf), every s is inf - inf or 0 * inf, and B's own edge is inf - inf.
    A usable d2 of +inf: B = the single point (inf, 0) against the unit box; edge 0 has s = +inf, region 1, d2 = +inf, and wins as the
    first usable candidate."""
    nan = float("nan")
    inf = float("inf")
    assert one(poly((nan, nan), (nan, nan), (nan, nan)), poly((nan, nan), (nan, nan), (nan, nan))) == HIT
    assert one(poly((0, 0), (1, -1), (0, 1)), poly((inf, inf))) == (inf, 0.0, 0.0, 0.0, 0.0, 0xFFFF, 0xFFFF, 0, ref.NO_CANDIDATE)
    assert one(square(0, 0), poly((inf, 0))) == (inf, 1.0, 0.0, inf, 0.0, 0, 0, 0, 0)


def test_rectangles_and_bad_pairs():
    """the rectangle form is the same rule on the four vertices of the planes; an index outside its set gives the BAD_PAIR record"""
    def planes(x0, y0):
        return np.array([[x0], [y0], [x0 + 1], [y0], [x0 + 1], [y0 + 1], [x0], [y0 + 1]], F)

    d = ref.rect_distances(planes(0, 0), planes(1.25, 0), [0, 0, 1], [0, 1, 0])
    assert tuple(d[0][f].item() for f in FIELDS) == (0.25, 1.0, 0.0, 1.25, 0.0, 0, 0, 0, 0)
    for q in (1, 2):
        assert tuple(d[q][f].item() for f in FIELDS) == (0.0, 0.0, 0.0, 0.0, 0.0, 0xFFFF, 0xFFFF, 0, ref.BAD_PAIR)
    bad_k = poly((0, 0), (1, 0), (0, 1))
    bad_k[2][0] = 17
    d = ref.poly_distances(bad_k, square(3, 3), [0, 5], [0, 0])
    assert (d["flags"] == ref.BAD_PAIR).all() and (d["edge"] == 0xFFFF).all() and (d["hit"] == 0).all()
    assert ref.same(d, d).all() and ref.DISTANCE_DT.itemsize == 32


# ---- properties on the dense sets ---------------------------------------------------------------------------------------------------

# The reference's own float32-versus-float64 deviation on the dense sets, over ALL 74 606 separated pairs (measured by this file;
# the test prints the figures it sees): the worst |dist - dist64| is 8.65e-7.  The error is set by the ulp of the coordinates (up to
# 6.5 here, ulp 4.8e-7), not by the distance, so it is bounded absolutely; relative to the distance it reaches 5.1e-4 on the pairs that
# are 1e-3 apart, and no relative bound is asserted.  The brute-force comparison allows 4 x the figure, as DESIGN.md 5.12 did.
DEV_ABS = 8.65e-7
# the same for a witness point's distance from its own polygon's boundary (float64 point-to-segment distances): 3.71e-7
DEV_BOUNDARY = 3.71e-7


def _verts64(s, idx):
    """-> x, y f64 [m][16] with the slots at and beyond k repeating vertex 0, and k [m]"""
    vx, vy, k = s
    k = k[idx].astype(np.int64)
    x, y = vx[:, idx].T.astype(np.float64), vy[:, idx].T.astype(np.float64)
    pad = np.arange(x.shape[1])[None, :] >= k[:, None]
    return np.where(pad, x[:, :1], x), np.where(pad, y[:, :1], y), k


def _point_to_boundary64(px, py, x, y):
    """float64 distance of one point per row from the closed polyline of that row (padding edges are zero-length copies of vertex 0)"""
    x1, y1 = np.roll(x, -1, axis=1), np.roll(y, -1, axis=1)
    ex, ey = x1 - x, y1 - y
    len2 = ex * ex + ey * ey
    s = (px[:, None] - x) * ex + (py[:, None] - y) * ey
    t = np.clip(s / np.where(len2 > 0, len2, 1.0), 0.0, 1.0)
    return np.hypot(px[:, None] - (x + t * ex), py[:, None] - (y + t * ey)).min(axis=1)


def _distance64(xa, ya, xb, yb):
    """float64 brute force: the smallest vertex-to-segment distance, both ways"""
    best = np.full(len(xa), np.inf)
    for (px, py), (qx, qy) in (((xa, ya), (xb, yb)), ((xb, yb), (xa, ya))):
        for v in range(qx.shape[1]):
            best = np.minimum(best, _point_to_boundary64(qx[:, v], qy[:, v], px, py))
    return best


@pytest.fixture(scope="module")
def dense(wl):
    a, b = cases.dense_poly_sets(wl)
    pairs = cases.all_pairs(a[0].shape[1], b[0].shape[1])
    i, j = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    return a, b, i, j, ref.poly_distances(a, b, i, j), contact_ref.poly_contacts(a, b, i, j)


def test_dense_batch_covers_every_branch(dense):
    """The shares of the committed seeds (prototype: 20 % hit; of the separated pairs side 0 71 %, regions 0 / 1 / 2 9 % / 34 % / 57 %),
    each class asserted at no less than half its share; no NaN, no NO_CANDIDATE, no BAD_PAIR in this batch."""
    _, _, _, _, d, c = dense
    assert np.array_equal(d["hit"], c["hit"]) and len(d) == 93300
    sep = d["hit"] == 0
    assert (d["flags"][sep] & (ref.NO_CANDIDATE | ref.BAD_PAIR) == 0).all() and np.isfinite(d["dist"]).all()
    side1 = (d["flags"][sep] & ref.EDGE_ON_B) != 0
    interior = (d["flags"][sep] & ref.INTERIOR) != 0
    xa, ya, ka = _verts64(dense[0], dense[2][sep])
    xb, yb, kb = _verts64(dense[1], dense[3][sep])
    # regions 0 and 1 are told apart by which end of the winning edge the closest point is
    ex = np.where(side1, xb[np.arange(sep.sum()), d["edge"][sep]], xa[np.arange(sep.sum()), d["edge"][sep]])
    ey = np.where(side1, yb[np.arange(sep.sum()), d["edge"][sep]], ya[np.arange(sep.sum()), d["edge"][sep]])
    cx, cy = np.where(side1, d["bx"][sep], d["ax"][sep]), np.where(side1, d["by"][sep], d["ay"][sep])
    region0 = ~interior & (cx == ex) & (cy == ey)
    shares = {"hit": 1 - sep.mean(), "side 0": 1 - side1.mean(), "side 1": side1.mean(), "region 0": region0.mean(),
              "region 1": (~interior & ~region0).mean(), "region 2": interior.mean()}
    print("shares:", {k: round(float(v), 4) for k, v in shares.items()})
    for name, share in (("hit", 0.20), ("side 0", 0.71), ("side 1", 0.29), ("region 0", 0.09), ("region 1", 0.34), ("region 2", 0.57)):
        assert shares[name] >= share / 2, (name, shares[name])
    assert (d["dist"][sep] > 0).all() and (d["dist"][~sep] == 0).all()


def test_dense_distance_is_at_least_the_contact_bound(dense):
    """-depth <= dist on every separated pair (include/c2d.h: "-depth is a lower bound of the distance"), with the float32 slack of
    1e-5 * dist + 1e-6; the worst excess seen is printed."""
    _, _, _, _, d, c = dense
    sep = d["hit"] == 0
    assert (c["depth"][sep] < 0).all()
    dist, low = d["dist"][sep].astype(np.float64), -c["depth"][sep].astype(np.float64)
    print("worst -depth - dist:", float((low - dist).max()), "vertex-to-vertex pairs where -depth < 0.999 dist:", int((low < 0.999 * dist).sum()))
    assert (low <= dist + 1e-5 * dist + 1e-6).all()
    assert (low < 0.999 * dist).sum() > 0.2 * sep.sum()      # the bound is not the distance: what the query is for


def test_dense_witness_points_and_float64_brute_force(dense):
    a, b, i, j, d, _ = dense
    sep = d["hit"] == 0
    xa, ya, _ = _verts64(a, i[sep])
    xb, yb, _ = _verts64(b, j[sep])
    on_a = _point_to_boundary64(d["ax"][sep].astype(np.float64), d["ay"][sep].astype(np.float64), xa, ya)
    on_b = _point_to_boundary64(d["bx"][sep].astype(np.float64), d["by"][sep].astype(np.float64), xb, yb)
    print("witness points off their boundaries by at most:", float(on_a.max()), float(on_b.max()))
    assert max(on_a.max(), on_b.max()) <= 4 * DEV_BOUNDARY
    # the two points are dist apart
    gap = np.hypot(d["ax"][sep].astype(np.float64) - d["bx"][sep], d["ay"][sep].astype(np.float64) - d["by"][sep])
    d64 = _distance64(xa, ya, xb, yb)
    err = np.abs(d["dist"][sep] - d64)
    print("float32 reference against float64 brute force over", int(sep.sum()), "separated pairs: worst absolute", float(err.max()), "worst relative",
          float((err / d64).max()), "; |points' gap - dist| worst", float(np.abs(gap - d["dist"][sep]).max()))
    assert (err <= 4 * DEV_ABS).all()
    assert (np.abs(gap - d64) <= 4 * DEV_ABS + 4 * DEV_BOUNDARY).all()
