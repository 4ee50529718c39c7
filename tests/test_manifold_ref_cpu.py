"""CPU tests that pin tests/manifold_ref.py — the numpy restatement of the manifold contract of include/c2d.h that the GPU tests
compare c2d_poly_pair_manifolds with — on hand-computed cases whose expected values are exact in binary32, on properties of a
seeded random batch, and on the conditions that batch has to meet (tests/manifold_cases.py; the GPU tests run the same batch)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contact_ref  # noqa: E402
import manifold_cases as cases  # noqa: E402
import manifold_ref as ref  # noqa: E402

F = np.float32
FIELDS = ("x0", "y0", "d0", "x1", "y1", "d1", "feature", "count", "flags", "reserved")


def poly(*pts):
    """one polygon as a set of one: (vx [16][1], vy, k)"""
    vx, vy = np.zeros((16, 1), F), np.zeros((16, 1), F)
    for r, (x, y) in enumerate(pts):
        vx[r, 0], vy[r, 0] = x, y
    return vx, vy, np.array([len(pts)], np.uint8)


def square(x0, y0, s=1.0):
    return poly((x0, y0), (x0 + s, y0), (x0 + s, y0 + s), (x0, y0 + s))


def one(a, b):
    c, m = ref.poly_manifolds(a, b, [0], [0])
    return c[0], tuple(m[0][f].item() for f in FIELDS)


DIAMOND = ((3.5, 2), (5.5, 0), (7.5, 2), (5.5, 4))      # counter-clockwise, its left corner first


def test_boxes_face_to_face():
    """A = [0, 1]^2, B = A + (0.75, 0).  The contact is axis 1 of A, (-1, 0), from o2 (pos false), depth 0.25: R = A, r = 1,
    sigma = -1, F = minA = -1.  B projects to -0.75, -1.75, -1.75, -0.75: the deepest (largest) is vertex 0, and vertex 3 ties
    without replacing it.  p_prv = -0.75 is strictly deeper than p_nxt = -1.75, so u = prv = 3 and the incident edge is 3 (from
    vertex 3 to vertex 0).  tau = y; the reference edge (1, 0) - (1, 1) gives the slab [0, 1], and both ends lie on its rim."""
    c, m = one(square(0, 0), square(0.75, 0))
    assert (c["depth"], c["axis"]) == (0.25, 1)
    assert m == (0.75, 0.0, 0.25, 0.75, 1.0, 0.25, 3, 2, 0, 0)


def test_boxes_face_to_face_one_end_clipped():
    """The same with B half a unit higher: tau_w = 0.5 stays, tau_u = 1.5 > hi = 1 is clipped with s = (1 - 1.5) / (0.5 - 1.5) = 0.5
    to (0.75, 1.5 + (0.5 - 1.5) * 0.5) = (0.75, 1); equal depths."""
    c, m = one(square(0, 0), square(0.75, 0.5))
    assert (c["depth"], c["axis"]) == (0.25, 1)
    assert m == (0.75, 0.5, 0.25, 0.75, 1.0, 0.25, 3, 2, ref.P1_CLIPPED, 0)


def test_corner_into_a_face():
    """A = [0, 4]^2; the diamond's left corner (3.5, 2) is half a unit inside A's right face.  Axis 1 of A, (-4, 0): A projects to
    [-16, 0], the diamond to -14, -22, -30, -22; o2 = -14 + 16 = 2, d = 2 / 4 (the diamond's own axes give 5 / sqrt(8)).  sigma = -1,
    F = -16, w = 0; nxt and prv tie at -22, so u = nxt = 1 and the incident edge is 0.  tau = 4 y, slab [0, 16]: tau_w = 8, tau_u = 0
    (on the rim, not below it).  d0 = (-14 + 16) / 4, d1 = (-22 + 16) / 4: the second point is reported with its negative depth."""
    c, m = one(square(0, 0, 4.0), poly(*DIAMOND))
    assert (c["depth"], c["nx"], c["ny"], c["axis"]) == (0.5, 1.0, 0.0, 1)
    assert m == (3.5, 2.0, 0.5, 5.5, 0.0, -1.5, 0, 2, 0, 0)


def test_clockwise_incident_polygon_with_the_deepest_vertex_last():
    """The diamond clockwise, starting at its top: (5.5, 4), (7.5, 2), (5.5, 0), (3.5, 2).  The deepest vertex is w = 3 = k - 1; its
    next is vertex 0 (the wrap) at (5.5, 4), its previous vertex 2 at (5.5, 0); they tie, so u = nxt and the feature is edge 3.
    tau_u = 16 is on the rim."""
    c, m = one(square(0, 0, 4.0), poly((5.5, 4), (7.5, 2), (5.5, 0), (3.5, 2)))
    assert (c["depth"], c["axis"]) == (0.5, 1)
    assert m == (3.5, 2.0, 0.5, 5.5, 4.0, -1.5, 3, 2, 0, 0)


def test_reference_on_b():
    """The pair of test_corner_into_a_face exchanged: the square is B, its edge 1 is axis ka + 1 = 5.  o1 = maxA - minB = -14 + 16
    = 2 (pos true), so the normal (-1, 0) points from the diamond to the square; sigma = -1 ((R is A) != pos), F = minB = -16."""
    c, m = one(poly(*DIAMOND), square(0, 0, 4.0))
    assert (c["depth"], c["nx"], c["ny"], c["axis"]) == (0.5, -1.0, 0.0, 5)
    assert m == (3.5, 2.0, 0.5, 5.5, 0.0, -1.5, 0, 2, ref.REF_IS_B, 0)


def test_short_reference_edge_under_a_long_incident_edge():
    """A = [0, 1]^2 one unit below the long edge (-3, 2) - (5, 2) of a triangle.  Axis 0 of A, (0, 1): o1 = maxA - minB = 1 - 2,
    depth -1 (pos true; the triangle's own edge ties later), sigma = +1, F = maxA = 1.  The triangle projects to 2, 2, 8: w = 0,
    u = nxt = 1.  tau = x, slab [0, 1]: tau_w = -3 is clipped with s = 3 / 8 to (0, 2), tau_u = 5 with s = (1 - 5) / (-3 - 5) = 0.5
    to (1, 2).  Both depths are (1 - 2) / 1."""
    c, m = one(square(0, 0), poly((-3, 2), (5, 2), (1, 8)))
    assert (c["depth"], c["nx"], c["ny"], c["axis"], c["hit"]) == (-1.0, 0.0, 1.0, 0, 0)
    assert m == (0.0, 2.0, -1.0, 1.0, 2.0, -1.0, 0, 2, ref.P0_CLIPPED | ref.P1_CLIPPED, 0)


def test_outside_slab():
    """Unit squares corner to corner: B = A + (2, 2).  Axis 0 of A, (0, 1), depth 1 - 2 = -1 (axis 1 ties later).  B's edge (2, 2) -
    (3, 2) has tau = x = 2 and 3, both above hi = 1: one point, the deepest vertex as it is."""
    c, m = one(square(0, 0), square(2, 2))
    assert (c["depth"], c["axis"], c["hit"]) == (-1.0, 0, 0)
    assert m == (2.0, 2.0, -1.0, 0.0, 0.0, 0.0, 0, 1, ref.OUTSIDE_SLAB, 0)


def test_incident_point_and_segment():
    """kI = 1: the point (5, 0.5) against the unit square (contact: axis 2 = the square's edge 1, depth -4, normal (-1, 0)): one point,
    feature 0, no clip, d0 = (p - F) / len = (-5 + 1) / 1.  A point inside the square: axis 1 = edge 0, depth 0.25.
    kI = 2: the segment (3, 1) - (6, 3) into [0, 4]^2: axis 1, d = (-12 + 16) / 4 = 1; nxt = prv = 1, so u = nxt and the feature
    is edge 0; the far end is reported at (-24 + 16) / 4 = -2."""
    c, m = one(poly((5, 0.5)), square(0, 0))
    assert (c["depth"], c["axis"]) == (-4.0, 2)
    assert m == (5.0, 0.5, -4.0, 0.0, 0.0, 0.0, 0, 1, ref.REF_IS_B, 0)
    c, m = one(poly((0.5, 0.25)), square(0, 0))
    assert (c["depth"], c["axis"]) == (0.25, 1)
    assert m == (0.5, 0.25, 0.25, 0.0, 0.0, 0.0, 0, 1, ref.REF_IS_B, 0)
    c, m = one(square(0, 0, 4.0), poly((3, 1), (6, 3)))
    assert (c["depth"], c["axis"]) == (1.0, 1)
    assert m == (3.0, 1.0, 1.0, 6.0, 3.0, -2.0, 0, 2, 0, 0)


def test_bad_pairs_and_no_axis_have_the_empty_manifold():
    a, b = square(0, 0), square(0.5, 0)
    c, m = ref.poly_manifolds(a, b, [0, 1, -1, 0], [0, 0, 0, 1])
    assert c["flags"].tolist() == [0, contact_ref.BAD_PAIR, contact_ref.BAD_PAIR, contact_ref.BAD_PAIR]
    assert m["count"].tolist() == [2, 0, 0, 0] and m["feature"].tolist()[1:] == [0xFFFF] * 3
    assert m[1:].tobytes() == ref.empty(3).tobytes()
    c, m = ref.poly_manifolds(poly((0, 0)), poly((5, 5)), [0], [0])       # two points: no usable axis
    assert c["flags"][0] == contact_ref.NO_AXIS and m.tobytes() == ref.empty(1).tobytes()
    bad_k = (b[0], b[1], np.array([17], np.uint8))
    assert ref.poly_manifolds(a, bad_k, [0], [0])[1].tobytes() == ref.empty(1).tobytes()
    assert ref.poly_manifolds(a, (b[0][:, :0], b[1][:, :0], b[2][:0]), [0], [0])[1].tobytes() == ref.empty(1).tobytes()


def test_contacts_are_contact_refs():
    a, b = square(0, 0), poly(*DIAMOND)
    assert ref.poly_manifolds(a, b, [0, 0], [0, 5])[0].tobytes() == contact_ref.poly_contacts(a, b, [0, 0], [0, 5]).tobytes()


# ---- the random batch ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def batch(wl):
    a, b = cases.random_colliding_batch(wl)
    idx = np.arange(cases.BATCH)
    c, m, info = ref.poly_manifolds(a, b, idx, idx, details=True)
    return a, b, c, m, info


# What tests/manifold_ref.py alone yields on the batch (measured on the CPU; each asserted with room to spare, none below 2 %):
#   colliding 63.9 %, REF_IS_B 51.0 %, sigma > 0 39.9 %, u == prv 50.5 %, P0_CLIPPED 10.3 %, P1_CLIPPED 25.1 %, both 4.3 %,
#   OUTSIDE_SLAB 21.1 %, w == 0 17.2 %, w == kI - 1 18.0 %
MIN_SHARE = {"colliding": 0.5, "REF_IS_B": 0.4, "REF_IS_A": 0.4, "sigma > 0": 0.3, "sigma < 0": 0.3, "u == prv": 0.4, "u == nxt": 0.4,
             "P0_CLIPPED": 0.05, "P1_CLIPPED": 0.15, "both clipped": 0.02, "OUTSIDE_SLAB": 0.1, "w == 0": 0.1, "w == kI - 1": 0.1}


def test_the_batch_holds_every_case(batch):
    a, b, c, m, info = batch
    assert info["live"].all() and (m["count"] >= 1).all()
    assert a[2].min() == 3 and a[2].max() == 16 and b[2].min() == 3 and b[2].max() == 16
    fl = m["flags"]
    share = {"colliding": c["hit"] == 1, "REF_IS_B": fl & ref.REF_IS_B != 0, "REF_IS_A": fl & ref.REF_IS_B == 0, "sigma > 0": info["up"], "sigma < 0": ~info["up"],
             "u == prv": info["u"] == info["prv"], "u == nxt": info["u"] == info["nxt"], "P0_CLIPPED": fl & ref.P0_CLIPPED != 0,
             "P1_CLIPPED": fl & ref.P1_CLIPPED != 0, "both clipped": fl & 6 == 6, "OUTSIDE_SLAB": fl & ref.OUTSIDE_SLAB != 0, "w == 0": info["w"] == 0,
             "w == kI - 1": info["w"] == info["k_i"] - 1}
    got = {name: float(np.mean(v)) for name, v in share.items()}
    print(got)
    for name, least in MIN_SHARE.items():
        assert least >= 0.02 and got[name] >= least, (name, got[name], least)
    # mixed winding on both sides (the sign of the shoelace sum)
    for vx, vy, k in (a, b):
        real = np.arange(16)[:, None] < k[None, :]
        nx_ = np.where(np.arange(16)[:, None] + 1 < k[None, :], np.roll(vx, -1, axis=0), vx[:1])
        ny_ = np.where(np.arange(16)[:, None] + 1 < k[None, :], np.roll(vy, -1, axis=0), vy[:1])
        area = np.where(real, vx.astype(np.float64) * ny_ - nx_ * vy.astype(np.float64), 0).sum(axis=0)
        assert 0.2 < np.mean(area < 0) < 0.5


def test_unclipped_point_0_has_the_contacts_depth(batch):
    _, _, c, m, _ = batch
    plain = m["flags"] & ref.P0_CLIPPED == 0
    assert plain.sum() > 3000
    assert np.array_equal(m["d0"][plain].view(np.uint32), c["depth"][plain].view(np.uint32))


def geometry64(a, b, m, info):
    """float64 views of the batch: per pair and point (0, 1) the distance by which tau leaves the slab (in length units: over |n|),
    the distance from the point to the incident edge `feature`, and the distance from the point to the same clip made in float64"""
    n = len(m)
    cols = np.arange(n)
    ref_b = info["ref_b"]
    d = np.float64
    rx, ry = np.where(ref_b, b[0], a[0]).astype(d), np.where(ref_b, b[1], a[1]).astype(d)
    ix, iy = np.where(ref_b, a[0], b[0]).astype(d), np.where(ref_b, a[1], b[1]).astype(d)
    nx, ny, length = info["nx"].astype(d), info["ny"].astype(d), np.hypot(info["nx"].astype(d), info["ny"].astype(d))
    tau = lambda x, y: ny * x - nx * y                                                    # noqa: E731
    t0, t1 = tau(rx[info["r"], cols], ry[info["r"], cols]), tau(rx[info["r1"], cols], ry[info["r1"], cols])
    lo, hi = np.minimum(t0, t1), np.maximum(t0, t1)
    f0 = m["feature"].astype(np.int64)
    f1 = (f0 + 1) % info["k_i"]
    ex0, ey0, ex1, ey1 = ix[f0, cols], iy[f0, cols], ix[f1, cols], iy[f1, cols]
    ends = {0: (info["w"], info["u"]), 1: (info["u"], info["w"])}
    out = {}
    for q in (0, 1):
        x, y = m[f"x{q}"].astype(d), m[f"y{q}"].astype(d)
        t = tau(x, y)
        leaves = np.maximum(np.maximum(lo - t, t - hi), 0) / length
        ux, uy = ex1 - ex0, ey1 - ey0
        s = np.clip(((x - ex0) * ux + (y - ey0) * uy) / (ux * ux + uy * uy), 0, 1)
        off_edge = np.hypot(x - (ex0 + s * ux), y - (ey0 + s * uy))
        g, h = ends[q]
        xg, yg, xh, yh = ix[g, cols], iy[g, cols], ix[h, cols], iy[h, cols]
        tg, th = tau(xg, yg), tau(xh, yh)
        moved = (tg < lo) | (tg > hi)
        with np.errstate(all="ignore"):
            s64 = (np.where(tg < lo, lo, hi) - tg) / (th - tg)
        x64, y64 = np.where(moved, xg + (xh - xg) * s64, xg), np.where(moved, yg + (yh - yg) * s64, yg)
        out[q] = leaves, off_edge, np.hypot(x - x64, y - y64)
    return out


# The reference's own float32-versus-float64 deviation on this batch: the largest distance between a point of a two-point manifold
# and the same clip made in float64 (same axis, same w and u).  Measured: 1.3064e-6 (coordinates up to about 6: under 3 ulp); the slab and edge
# residuals themselves measure 5.2e-7 and 2.6e-7.
F32_DEVIATION = 1.31e-6


def test_points_lie_in_the_slab_and_on_the_incident_edge(batch):
    """for every two-point manifold (one-point manifolds are the deepest vertex itself, by definition outside the slab or alone)"""
    a, b, _, m, info = batch
    g = geometry64(a, b, m, info)
    two = m["count"] == 2
    assert two.sum() > 3000
    deviation = max(g[q][2][two].max() for q in (0, 1))
    print("float32 versus float64:", deviation, "slab:", max(g[q][0][two].max() for q in (0, 1)), "edge:", max(g[q][1][two].max() for q in (0, 1)))
    assert deviation <= F32_DEVIATION                         # (measured 1.3064e-6)
    tol = 4 * F32_DEVIATION
    for q in (0, 1):
        leaves, off_edge, _ = g[q]
        assert leaves[two].max() <= tol, (q, leaves[two].max())           # tau inside [lo, hi]
        assert off_edge[two].max() <= tol, (q, off_edge[two].max())       # on the incident edge `feature`
    one_point = ~two
    assert g[0][1][one_point].max() == 0                                  # the deepest vertex is an end of its edge
