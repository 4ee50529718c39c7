"""CPU tests that pin tests/contact_ref.py — the numpy restatement of the contact contract of include/c2d.h that the GPU tests
compare c2d_poly_pair_contacts / c2d_rect_pair_contacts with — on hand-computed cases, and its `hit` on the oracle."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contact_cases as cases  # noqa: E402
import contact_ref as ref  # noqa: E402

F = np.float32


def poly(*pts):
    """one polygon as a set of one: (vx [16][1], vy, k)"""
    vx, vy = np.zeros((16, 1), F), np.zeros((16, 1), F)
    for r, (x, y) in enumerate(pts):
        vx[r, 0], vy[r, 0] = x, y
    return vx, vy, np.array([len(pts)], np.uint8)


def square(x0, y0, s=1.0):
    return poly((x0, y0), (x0 + s, y0), (x0 + s, y0 + s), (x0, y0 + s))


def one(a, b):
    return ref.poly_contacts(a, b, [0], [0])[0]


def test_offset_unit_squares():
    """B = A + (0.75, 0).  Axis 0 of A is (0, 1): both project to [0, 1], d = 1.  Axis 1 is (-1, 0): A projects to [-1, 0], B to
    [-1.75, -0.75], o1 = 1.75, o2 = 0.25, d = 0.25 from o2, so the normal is -(-1, 0) = (1, 0).  Axis 3 = (1, 0) and B's axes 5
    and 7 give 0.25 as well: the first of equals, axis 1, stays."""
    c = one(square(0, 0), square(0.75, 0))
    assert (c["depth"], c["nx"], c["ny"], c["axis"], c["hit"], c["flags"]) == (0.25, 1.0, 0.0, 1, 1, 0)


def test_touching_squares_have_depth_zero_and_hit(oracle):
    a, b = square(0, 0), square(1, 0)
    c = one(a, b)
    assert c["depth"] == 0 and (c["nx"], c["ny"]) == (1.0, 0.0) and c["axis"] == 1 and c["flags"] == 0
    want, _ = oracle.sat_poly_pairs(np.stack([a[0], b[0]]), np.stack([a[1], b[1]]), np.stack([a[2], b[2]]))
    assert c["hit"] == want[0] == 1     # strict < does not separate touching shapes


def test_identical_squares_first_axis_wins():
    c = one(square(2, 3), square(2, 3))
    assert (c["depth"], c["nx"], c["ny"], c["axis"], c["hit"]) == (1.0, 0.0, 1.0, 0, 1)   # axis 0 = (0, 1), o1 == o2: the + sign


def test_triangle_inside_a_square():
    """Square [0, 4]^2, triangle (1, 1), (2, 1), (1, 2).  Axis 0 = (0, 4): A projects to [0, 16], the triangle to [4, 8]; o1 = 12,
    o2 = 8, d = 8 / 4 = 2 from o2: normal (0, -1) — the shortest way out is down.  Axes 1, 2, 3, 4 and 6 give 2 as well, axis 5
    gives 3 / sqrt(2)."""
    c = one(square(0, 0, 4.0), poly((1, 1), (2, 1), (1, 2)))
    assert (c["depth"], c["nx"], c["ny"], c["axis"], c["hit"], c["flags"]) == (2.0, 0.0, -1.0, 0, 1, 0)


def test_separated_pair():
    c = one(square(0, 0), square(3, 0))   # axis 1 = (-1, 0): o2 = -3 + 1 = -2
    assert (c["depth"], c["nx"], c["ny"], c["axis"], c["hit"], c["flags"]) == (-2.0, 1.0, 0.0, 1, 0, 0)


def test_points():
    c = one(poly((0, 0)), poly((5, 5)))           # two points: only zero axes
    assert c["flags"] == ref.NO_AXIS and c["axis"] == 0xFFFF and c["depth"] == np.inf and (c["nx"], c["ny"]) == (0, 0) and c["hit"] == 1
    c = one(poly((5, 0.5)), square(0, 0))         # the square supplies the axes: ka = 1, so its edge 1 is axis 2
    assert (c["depth"], c["nx"], c["ny"], c["axis"], c["hit"], c["flags"]) == (-4.0, -1.0, 0.0, 2, 0, 0)
    c = one(poly((0, 0), (1, 0)), poly((3, 3)))   # a segment: its first edge (0, 1) sees the point 3 above
    assert (c["depth"], c["nx"], c["ny"], c["axis"], c["hit"]) == (-3.0, 0.0, 1.0, 0, 0)


def test_bad_pairs():
    a, b = square(0, 0), square(0.5, 0)
    bad_k = (b[0], b[1], np.array([17], np.uint8))
    got = ref.poly_contacts(a, b, [0, 1, -1, 0], [0, 0, 0, 1])
    assert got["flags"].tolist() == [0, ref.BAD_PAIR, ref.BAD_PAIR, ref.BAD_PAIR]
    assert ref.poly_contacts(a, bad_k, [0], [0])["flags"][0] == ref.BAD_PAIR
    c = got[1]
    assert (c["depth"], c["nx"], c["ny"], c["axis"], c["hit"]) == (0, 0, 0, 0xFFFF, 0)


def test_rect_axes_are_edge_vectors():
    """rectangles 2 x 1 at the origin and at (1.5, 0): axis 0 is the edge VECTOR (2, 0), projections 2x: A [-2, 2], B [1, 5],
    o1 = 1, o2 = 7, d = 1 / 2; axis 1 = (0, 1) gives 1."""
    a = np.array([[-1, -0.5, 1, -0.5, 1, 0.5, -1, 0.5]], F).T
    b = a + np.array([[1.5, 0] * 4], F).T
    c = ref.rect_contacts(a, b, [0], [0])[0]
    assert (c["depth"], c["nx"], c["ny"], c["axis"], c["hit"], c["flags"]) == (0.5, 1.0, 0.0, 0, 1, 0)


def test_hit_is_the_oracles_boolean(oracle, wl):
    """a few thousand random pairs, then the hard batches (non-finite vertices, extreme scales, degenerate polygons)"""
    a, b = cases.dense_poly_sets(wl, n=60)
    pairs = cases.all_pairs(60, 71)
    batches = {"dense": (a, b, pairs, True)}
    batches.update(cases.hard_poly_batches(wl))
    seen = 0
    for name, (sa, sb, pr, finite) in batches.items():
        i, j = pr[:, 0].astype(np.int64), pr[:, 1].astype(np.int64)
        got = ref.poly_contacts(sa, sb, i, j)
        want, _ = oracle.sat_poly_pairs(np.stack([sa[0][:, i], sb[0][:, j]]), np.stack([sa[1][:, i], sb[1][:, j]]), np.stack([sa[2][i], sb[2][j]]))
        assert np.array_equal(got["hit"], want), name
        if finite:
            live = got["flags"] == 0
            assert np.array_equal(got["hit"][live] == 1, got["depth"][live] >= 0), name
        seen += len(pr)
    assert seen > 20_000
    ra, rb = cases.rect_sets(oracle, wl, n=70)
    qa, qb = cases.quad_sets(70)
    na = wl.inject_non_finite(ra, seed=5, frac=0.3)
    pr = cases.all_pairs(70, 70)
    i, j = pr[:, 0].astype(np.int64), pr[:, 1].astype(np.int64)
    for name, (sa, sb) in {"rects": (ra, rb), "quads": (qa, qb), "non_finite": (na, rb)}.items():
        got = ref.rect_contacts(sa, sb, i, j)
        want, _ = oracle.sat_rect_pairs_verts(np.concatenate([sa[:, i], sb[:, j]]))
        assert np.array_equal(got["hit"], want), name
        if name != "non_finite":
            live = got["flags"] == 0
            assert np.array_equal(got["hit"][live] == 1, got["depth"][live] >= 0), name
    assert (ref.rect_contacts(qa, qb, i, j)["flags"] == ref.NO_AXIS).any()   # two quads that are points


def test_well_conditioned_batch_meets_its_own_filter(oracle, wl):
    """The generator of the GPU translation property: at least 90 % of its hit pairs have depth > 1e-3, and moving B by
    (depth + 1e-3 * 8) * normal separates every one of them (here with the reference's contacts and the oracle's boolean)."""
    a, b = cases.well_conditioned_poly_sets(wl)
    n = a[0].shape[1]
    pr = cases.all_pairs(n, n)
    i, j = pr[:, 0].astype(np.int64), pr[:, 1].astype(np.int64)
    c = ref.poly_contacts(a, b, i, j)
    hits = c["hit"] == 1
    keep = hits & (c["depth"] > 1e-3) & (c["flags"] == 0)
    assert hits.sum() > 500 and keep.sum() >= 0.9 * hits.sum()
    step = c["depth"][keep] + F(1e-3 * 8)
    moved = cases.translated(b, j[keep], step * c["nx"][keep], step * c["ny"][keep])
    after, _ = oracle.sat_poly_pairs(np.stack([a[0][:, i[keep]], moved[0]]), np.stack([a[1][:, i[keep]], moved[1]]), np.stack([a[2][i[keep]], moved[2]]))
    assert not after.any()
