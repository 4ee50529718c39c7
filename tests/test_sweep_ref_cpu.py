"""CPU tests that pin tests/sweep_ref.py — the numpy restatement of the sweep contract of include/c2d.h that the GPU tests compare
c2d_poly_pair_sweeps / c2d_rect_pair_sweeps with — on hand-computed cases whose expected values are exact in binary32 and on
properties of the dense sets of tests/contact_cases.py (300 x 311 polygons, all 93 300 pairs, both sets moving by up to +-4 per
component): against contact_ref's boolean, against a float64 run of the same rule, against the shapes at the time of impact and
against a 401-sample brute force."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contact_cases as cases  # noqa: E402
import contact_ref  # noqa: E402
import distance_ref  # noqa: E402
import ray_ref  # noqa: E402
import sweep_ref as ref  # noqa: E402

F = np.float32
FIELDS = ("toi", "nx", "ny", "axis", "hit", "flags")
INF = float("inf")
MISS = (INF, 0.0, 0.0, 0xFFFF, 0, 0)
START = (0.0, 0.0, 0.0, 0xFFFF, 1, ref.START_OVERLAP)
BAD = (0.0, 0.0, 0.0, 0xFFFF, 0, ref.BAD_PAIR)


def poly(*pts):
    """one polygon as a set of one: (vx [16][1], vy, k)"""
    vx, vy = np.zeros((16, 1), F), np.zeros((16, 1), F)
    for r, (x, y) in enumerate(pts):
        vx[r, 0], vy[r, 0] = x, y
    return vx, vy, np.array([len(pts)], np.uint8)


def square(x0, y0, s=1.0):
    return poly((x0, y0), (x0 + s, y0), (x0 + s, y0 + s), (x0, y0 + s))


def planes(x0, y0):
    return np.array([[x0], [y0], [x0 + 1], [y0], [x0 + 1], [y0 + 1], [x0], [y0 + 1]], F)


def move(dx, dy):
    return None if dx is None else (np.array([dx], F), np.array([dy], F))


def one(a, b, ma=(None, None), mb=(None, None), call=ref.poly_sweeps):
    s = call(a, b, [0], [0], move(*ma), move(*mb))[0]
    return tuple(s[f].item() for f in FIELDS)


def test_boxes_closing_the_first_of_the_tied_axes_wins():
    """A = [0, 1]^2, B = A + (2, 0) (a gap of 1), B moves by (-4, 0): r = (-4, 0).  A's axis 0 = (0, 1) has v = 0 and o1 = o2 = 1: it
    bounds nothing.  A's axis 1 = (-1, 0): v = 4 > 0, A projects to [-1, 0] and B to [-3, -2], o1 = 3, o2 = -1, lo = 1 / 4, hi = 3 / 4:
    t_in = 1/4 on axis 1 with v > 0, so the normal is -(-1, 0) = (1, 0).  A's axis 3 = (1, 0) and B's axes 5 and 7 reach the same lo
    with the same bits and do not replace it.  As planes the axes are the edge vectors: axis 0 = (1, 0), v = -4 < 0, o1 = -1, o2 = 3,
    lo = 1/4, and the normal is +(1, 0)."""
    assert one(square(0, 0), square(2, 0), mb=(-4, 0)) == (0.25, 1.0, 0.0, 1, 1, 0)
    assert one(planes(0, 0), planes(2, 0), mb=(-4, 0), call=ref.rect_sweeps) == (0.25, 1.0, 0.0, 0, 1, 0)


def test_the_same_with_a_and_b_exchanged_and_with_the_motion_split():
    """A = the box at (2, 0) moving by (-4, 0), B = the unit box standing still: r = (4, 0); A's axis 1 = (-1, 0) has v = -4 < 0,
    A projects to [-3, -2], B to [-1, 0], o1 = -1, lo = 1/4, and the normal is +(-1, 0): B lies to the left of A.  A moving by
    (1, 0) and B by (-3, 0) is the first case again."""
    assert one(square(2, 0), square(0, 0), ma=(-4, 0)) == (0.25, -1.0, 0.0, 1, 1, 0)
    assert one(square(0, 0), square(2, 0), ma=(1, 0), mb=(-3, 0)) == (0.25, 1.0, 0.0, 1, 1, 0)
    assert one(planes(0, 0), planes(2, 0), ma=(1, 0), mb=(-3, 0), call=ref.rect_sweeps) == (0.25, 1.0, 0.0, 0, 1, 0)


def test_a_motion_that_stops_short_and_one_parallel_to_the_gap():
    """B moves by (-1/2, 0): axis 1 has v = 1/2 and lo = 2 > t_out = 1: a miss.  B moves by (0, 3): axis 0 = (0, 1) has v = 3,
    lo = -1/3, hi = 1/3; axis 1 = (-1, 0) has v = 0 and o2 = -1 < 0: `never`."""
    assert one(square(0, 0), square(2, 0), mb=(-0.5, 0)) == MISS
    assert one(square(0, 0), square(2, 0), mb=(0, 3)) == MISS
    assert one(planes(0, 0), planes(2, 0), mb=(0, 3), call=ref.rect_sweeps) == MISS


def test_a_diagonal_pass_that_grazes_one_vertex():
    """A = [0, 1]^2, B = [2, 3] x [0, 1] moving by (-2, 2).  Axis 0 = (0, 1): v = 2, o1 = o2 = 1, lo = -1/2, hi = 1/2: t_out = 1/2.
    Axis 1 = (-1, 0): v = 2, o1 = 3, o2 = -1, lo = 1/2, hi = 3/2: t_in = 1/2.  At t = 1/2 the two boxes share the one point (1, 1) and
    nothing else during the step: t_in == t_out is a hit."""
    assert one(square(0, 0), square(2, 0), mb=(-2, 2)) == (0.5, 1.0, 0.0, 1, 1, 0)
    assert one(square(0, 0), square(2, 0), mb=(-2, 2.5)) == MISS       # y parts at t = 0.4, before x meets at t = 0.5


def test_zero_motion_and_start_overlap():
    """no motion: a separated pair is a miss (axis 1: v = 0, o2 < 0), a touching pair is hit0 (strict <), whichever way "no motion" is
    said; a pair that overlaps at t = 0 is the START_OVERLAP record whatever the motion"""
    for ma, mb in (((None, None), (None, None)), ((0, 0), (None, None)), ((0, 0), (0, 0)), ((3, -2), (3, -2))):
        assert one(square(0, 0), square(2, 0), ma, mb) == MISS
        assert one(square(0, 0), square(1, 0), ma, mb) == START
    assert one(square(0, 0), square(0.5, 0.5), mb=(-4, 1)) == START
    assert one(square(0, 0), square(0.5, 0.5), mb=(100, 100)) == START
    assert one(planes(0, 0), planes(0.5, 0.5), mb=(100, 100), call=ref.rect_sweeps) == START


def test_a_hit_whose_t_in_kept_its_start():
    """A = [-1, 0] x [0, 1], B = [g, 1] x [0, 1] with g = 2^-140: separated at t = 0 (0 < g).  B moves by (-2^100, 0): on A's axis 1
    = (1, 0), v = -2^100, o1 = -g, lo = 2^-240 rounds to 0 and does not replace t_in = +0; hi = -2 / -2^100 = 2^-99.  A hit at toi = 0
    with no axis, and START_OVERLAP clear."""
    g = 2.0 ** -140
    assert one(square(-1, 0), poly((g, 0), (1, 0), (1, 1), (g, 1)), mb=(-2.0 ** 100, 0)) == (0.0, 0.0, 0.0, 0xFFFF, 1, 0)


def test_clockwise_polygon_and_nan_vertices():
    """A = the unit box listed clockwise: its axis 0 = (-1, 0) is the first closing axis (v = 4, lo = 1/4), normal -(-1, 0).
    A with the vertex (1, 1) replaced by NaN: the axes of the two edges at that vertex have a NaN v and are ignored; axis 3 = (1, 0)
    sees A in [0, 1] (fmin / fmax skip the NaN), v = -4, o1 = -1, lo = 1/4.  All NaN: no axis separates at t = 0, the pair is hit0."""
    nan = float("nan")
    assert one(poly((0, 0), (0, 1), (1, 1), (1, 0)), square(2, 0), mb=(-4, 0)) == (0.25, 1.0, 0.0, 0, 1, 0)
    assert one(poly((0, 0), (1, 0), (nan, nan), (0, 1)), square(2, 0), mb=(-4, 0)) == (0.25, 1.0, 0.0, 3, 1, 0)
    assert one(poly((nan, nan), (nan, nan), (nan, nan)), square(2, 0), mb=(-4, 0)) == START
    # a NaN motion: every v is NaN (0 * NaN), every axis is ignored, nothing sets `never`: the rule's answer is a hit at +0 with no axis
    assert one(square(0, 0), square(2, 0), mb=(nan, 0)) == (0.0, 0.0, 0.0, 0xFFFF, 1, 0)


def test_bad_pairs():
    s = ref.rect_sweeps(planes(0, 0), planes(2, 0), [0, 0, 1, -1], [0, 1, 0, 0], None, move(-4, 0))
    assert tuple(s[0][f].item() for f in FIELDS) == (0.25, 1.0, 0.0, 0, 1, 0)
    assert all(tuple(s[q][f].item() for f in FIELDS) == BAD for q in (1, 2, 3))
    bad_k = poly((0, 0), (1, 0), (0, 1))
    bad_k[2][0] = 17
    s = ref.poly_sweeps(bad_k, square(3, 3), [0, 5], [0, 0], move(1, 1), None)
    assert all(tuple(r[f].item() for f in FIELDS) == BAD for r in s)
    assert ref.same(s, s).all() and ref.SWEEP_DT.itemsize == 16
    empty = (np.zeros((16, 0), F), np.zeros((16, 0), F), np.zeros(0, np.uint8))
    assert tuple(ref.poly_sweeps(empty, square(0, 0), [0], [0])[0][f].item() for f in FIELDS) == BAD


# A moving point (k = 1) against the unit box is the ray query's segment o -> o + r against that box.  On these 2000 seeded points the
# float32 toi and the float32 t of tests/ray_ref.py each differ from their own float64 run by at most 2.97e-8 (measured by this file,
# which prints what it sees), and the two float64 runs agree to 1e-15; the test allows 4 x that figure between the two float32 results.
DEV_POINT = 2.97e-8


def test_a_moving_point_is_the_ray_query():
    rng = np.random.default_rng(9102)
    n = 2000
    ox, oy = rng.uniform(-3, 3, n).astype(F), rng.uniform(-3, 3, n).astype(F)
    dx, dy = rng.uniform(-4, 4, n).astype(F), rng.uniform(-4, 4, n).astype(F)
    pts = (np.zeros((16, n), F), np.zeros((16, n), F), np.ones(n, np.uint8))
    pts[0][0], pts[1][0] = ox, oy
    box = square(0, 0)
    idx, zero = np.arange(n), np.zeros(n, np.int64)
    sweeps = {d: ref.poly_sweeps(pts, box, idx, zero, (dx, dy), None, dtype=d) for d in (np.float32, np.float64)}
    rays = {d: ray_ref.ray_casts((ox, oy, dx, dy), box, dtype=d, with_t=True) for d in (np.float32, np.float64)}
    s32, (r32, t32), s64, (_, t64) = sweeps[np.float32], rays[np.float32], sweeps[np.float64], rays[np.float64]
    assert np.array_equal(s32["hit"], r32["hit"]) and 100 < s32["hit"].sum() < n - 100
    inside = (r32["flags"] & ray_ref.START_INSIDE) != 0
    assert np.array_equal((s32["flags"] & ref.START_OVERLAP) != 0, inside)
    hit = s32["hit"] == 1
    print("moving point: |toi - toi64|", float(np.abs(s32["toi"][hit] - s64["toi"][hit]).max()), "|t - t64|", float(np.abs(t32[hit] - t64[hit]).max()),
          "|toi64 - t64|", float(np.abs(s64["toi"][hit] - t64[hit]).max()), "|toi - t|", float(np.abs(s32["toi"][hit].astype(np.float64) - t32[hit]).max()))
    assert (np.abs(s32["toi"][hit].astype(np.float64) - t32[hit]) <= 4 * DEV_POINT).all()
    assert (np.abs(s64["toi"][hit] - t64[hit]) <= 1e-12).all()


# ---- properties on the dense sets ---------------------------------------------------------------------------------------------------

# The reference's own float32-versus-float64 deviation on the dense sets with both sets moving by up to +-4 per component (measured by
# this file on all 11 329 moving hits; the tests print the figures they see): the worst |toi - toi64| is 1.14e-5.  The error grows as
# the motion shrinks (an absolute error of the overlap divided by a smaller v), so it is bounded absolutely.
DEV_TOI = 1.14e-5
# B moved by toi * r (float64 toi of the float64 rule, the moved vertices rounded to float32) is this far from touching A at most:
# distance_ref's dist where the moved pair is separated, contact_ref's depth where it is hit.  7.3e-7, about 1.5 ulp of the largest
# coordinate; the float32 rule's own toi gives 9.4e-7.
DEV_TOUCH = 7.3e-7
MOTION = 4.0


@pytest.fixture(scope="module")
def dense(wl):
    a, b = cases.dense_poly_sets(wl)
    pairs = cases.all_pairs(a[0].shape[1], b[0].shape[1])
    i, j = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    rng = np.random.default_rng(9101)
    ma = tuple(rng.uniform(-MOTION, MOTION, a[0].shape[1]).astype(F) for _ in range(2))
    mb = tuple(rng.uniform(-MOTION, MOTION, b[0].shape[1]).astype(F) for _ in range(2))
    return a, b, i, j, ma, mb, ref.poly_sweeps(a, b, i, j, ma, mb), contact_ref.poly_contacts(a, b, i, j)


def _moved(b, j, tx, ty):
    """polygons b[j] translated by (tx, ty) in float64, rounded to float32: one polygon per pair"""
    return (b[0][:, j].astype(np.float64) + tx).astype(F), (b[1][:, j].astype(np.float64) + ty).astype(F), b[2][j]


def test_dense_batch_covers_every_class_and_agrees_with_the_contact_reference(dense):
    """start overlap 20.0 %, moving hits 12.1 %, misses 67.8 % on the committed seeds, each asserted at >= 5 %; START_OVERLAP is set
    exactly where contact_ref says hit; with no motion, hit is hit0 on every pair"""
    a, b, i, j, _, _, s, c = dense
    assert len(s) == 93300 and (s["flags"] & ref.BAD_PAIR == 0).all()
    start = (s["flags"] & ref.START_OVERLAP) != 0
    shares = {"start overlap": start.mean(), "moving hit": ((s["hit"] == 1) & ~start).mean(), "miss": (s["hit"] == 0).mean()}
    print("shares:", {k: round(float(v), 4) for k, v in shares.items()})
    assert all(v >= 0.05 for v in shares.values()), shares
    assert np.array_equal(start, c["hit"] == 1)
    assert (s["toi"][start] == 0).all() and (s["axis"][start] == 0xFFFF).all() and (s["hit"][start] == 1).all()
    moving = (s["hit"] == 1) & ~start
    assert (s["axis"][moving] != 0xFFFF).all() and (s["toi"][moving] > 0).all() and (s["toi"][moving] <= 1).all()
    assert np.allclose(np.hypot(s["nx"][moving], s["ny"][moving]), 1.0, atol=1e-6)
    assert np.isinf(s["toi"][s["hit"] == 0]).all()
    for still in (ref.poly_sweeps(a, b, i, j, None, None), ref.poly_sweeps(a, b, i, j, (np.zeros(300, F), np.zeros(300, F)), None)):
        assert np.array_equal(still["hit"], c["hit"]) and np.array_equal((still["flags"] & ref.START_OVERLAP) != 0, c["hit"] == 1)


def test_dense_float32_against_float64_and_the_shapes_at_the_time_of_impact(dense):
    a, b, i, j, ma, mb, s, _ = dense
    s64 = ref.poly_sweeps(a, b, i, j, ma, mb, dtype=np.float64)
    assert np.array_equal(s["hit"], s64["hit"]) and np.array_equal(s["axis"], s64["axis"]) and np.array_equal(s["flags"], s64["flags"])
    moving = (s["hit"] == 1) & (s["flags"] == 0)
    dev = np.abs(s["toi"][moving].astype(np.float64) - s64["toi"][moving])
    print("float32 rule against float64 rule over", int(moving.sum()), "moving hits: worst |toi - toi64|", float(dev.max()),
          "normals", float(max(np.abs(s["nx"][moving] - s64["nx"][moving]).max(), np.abs(s["ny"][moving] - s64["ny"][moving]).max())))
    assert (dev <= 4 * DEV_TOI).all()
    # at toi the shapes touch: B moved by toi * r is neither apart from A nor inside it, up to the slack
    rx, ry = (mb[0][j] - ma[0][i])[moving].astype(np.float64), (mb[1][j] - ma[1][i])[moving].astype(np.float64)
    n = int(moving.sum())
    idx = np.arange(n)
    at = (a[0][:, i[moving]], a[1][:, i[moving]], a[2][i[moving]])
    for name, rec in (("float64", s64), ("float32", s)):
        toi = rec["toi"][moving].astype(np.float64)
        bt = _moved(b, j[moving], toi * rx, toi * ry)
        d, c = distance_ref.poly_distances(at, bt, idx, idx), contact_ref.poly_contacts(at, bt, idx, idx)
        gap = np.where(d["hit"] == 1, -c["depth"].astype(np.float64), d["dist"].astype(np.float64))
        print(name, "toi: B at toi is from", float(gap.min()), "to", float(gap.max()), "from touching A")
        assert (np.abs(gap) <= 4 * DEV_TOUCH).all(), name


def test_dense_against_401_sampled_instants(dense):
    """every 50th pair: contact_ref's boolean at t = q / 400.  The samples never hit where the rule misses; they may step over a
    grazing pass on at most 0.5 % of the pairs; where both hit, the first hit sample lies 0 to one step above the rule's toi."""
    a, b, i, j, ma, mb, s, _ = dense
    i, j, s = i[::50], j[::50], s[::50]
    rx, ry = (mb[0][j] - ma[0][i]).astype(np.float64), (mb[1][j] - ma[1][i]).astype(np.float64)
    m = len(i)
    idx = np.arange(m)
    at = (a[0][:, i], a[1][:, i], a[2][i])
    sampled, first = np.zeros(m, bool), np.full(m, np.inf)
    for q in range(401):
        t = q / 400.0
        h = contact_ref.poly_contacts(at, _moved(b, j, t * rx, t * ry), idx, idx)["hit"] == 1
        first = np.where(h & ~sampled, t, first)
        sampled |= h
    rule = s["hit"] == 1
    stepped_over = int((rule & ~sampled).sum())
    both = rule & sampled
    late = first[both] - s["toi"][both]
    print("sampled pairs", m, "rule hits", int(rule.sum()), "stepped over by the samples", stepped_over, "first sample - toi from", float(late.min()), "to",
          float(late.max()))
    assert not (sampled & ~rule).any()
    assert stepped_over <= 0.005 * m
    assert (late >= -4 * DEV_TOI).all() and (late <= 1 / 400 + 4 * DEV_TOI).all()
