"""CPU tests that pin tests/ray_ref.py — the numpy restatement of the ray contract of include/c2d.h that the GPU tests compare
c2d_poly_ray_casts with — in three ways: hand-computed cases whose expected values are exact in binary32, properties of the ray
scene (311 polygons, 2 000 segments; the GPU tests run the same scene) with the same rule in float64 beside it, and an independent
cross-check: the segments as 2-gons through tests/contact_ref.py's pairwise boolean, on all 622 000 (segment, polygon) pairs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contact_ref  # noqa: E402
import ray_cases as cases  # noqa: E402
import ray_ref as ref  # noqa: E402

F = np.float32
HAND = cases.hand_cases()


def test_the_reference_speaks_of_the_same_record_as_the_cases():
    assert tuple(ref.RAY_HIT_DT.names) == cases.FIELDS and ref.RAY_HIT_DT.itemsize == 16
    assert (ref.START_INSIDE, ref.NONE16, ref.NONE32) == (cases.INSIDE, cases.NONE16, cases.NONE32)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_computed_cases(name):
    """The unit square is (0, 0), (1, 0), (1, 1), (0, 1): edge 0 the bottom, 1 the right side, 2 the top, 3 the left side.

    nearer_of_two_crossings   o = (-1, 0.5), d = (4, 0).  Edge 3, (0, 1) -> (0, 0): e = (0, -1), w = (1, 0.5), den = 4 * -1 - 0 = -4,
        tn = 1 * -1 - 0.5 * 0 = -1, un = 1 * 0 - 0.5 * 4 = -2: usable on the negative side, t = 1/4, u = 1/2.  Edge 1 gives den = 4,
        tn = 2, t = 1/2 and loses; edges 0 and 2 are parallel (den = 0).  tn has both signs (edge 0: +0.5, edge 3: -1): not inside.
    through_a_vertex          o = (-1, -1), d = (4, 4).  Edge 0: den = -4, tn = -1, un = 0: t = 1/4, u = -0.  Edge 3: den = -4,
        tn = -1, un = -4: t = 1/4, u = 1.  The same t: edge 0 stays.
    along_an_edge             o = (-1, 0), d = (4, 0): edges 0 and 2 have den = 0; edge 3 gives t = 1/4 at u = 1 (its end (0, 0)),
        edge 1 t = 1/2 at u = 0.
    ending_on_an_edge_...     d = (1, 0): edge 3 has den = -1 = tn, t = 1.  d = (0.75, 0): den = -0.75 > tn = -1: unusable.
    origin_inside_...         (0.5, 0.5): every tn = +0.5.  (0, 0.5) on edge 3: its tn is a zero, the others are positive — whichever
        way the ray goes.  (1, 1), a vertex: two zeros, two positive.
    point_queries             d = (0, 0): every den is 0, so only the inside candidate exists.  (2, 2): tn = 2 on edge 0, -1 on edge 1.
    clockwise                 the left side is now edge 0, upwards: den = 4, tn = 1, un = 2.  Inside, every tn is negative.
    k1_is_never_hit           the only edge has length 0: den = 0 and tn = +-0, no sign at all.
    k2_crossed                (0, -1) -> (0, 1) and back: both edges give t = 1/2 at u = 1/2, edge 0 stays; tn = 2 and -2: not inside.
    identical_squares         three copies: polygon 0 wins on the edge and as the container.
    nearer_square_later...    polygon 0 is the square at x = 5 (t = 6/8), polygon 1 the unit square (t = 1/8).
    non_finite_rays           a NaN or an infinity in the origin makes tn NaN or of the wrong sign on every edge with den != 0.
    nan_vertices_...          vertices 0 and 2 NaN: every edge touches one, and a NaN tn rules out "inside"; the clean square at
        x = 3 is hit at t = 4/8.  With vertex 0 alone NaN, edges 1 and 2 are clean, and edge 1 is hit at t = 2/8."""
    rays, b, want = HAND[name]
    got = ref.ray_casts(rays, b)
    assert cases.as_tuples(got) == [tuple(w) for w in want]
    # the same through col_base, and the per-polygon boolean agrees with the record's hit
    based = ref.ray_casts(rays, b, col_base=1000)
    assert np.array_equal(based["poly"], np.where(got["hit"] == 1, got["poly"] + 1000, cases.NONE32))
    assert np.array_equal(ref.touched(rays, b).any(axis=1), got["hit"] == 1)


def test_every_hand_case_of_the_contract_is_present():
    assert len(HAND) == 14
    one = ref.ray_casts(*HAND["through_a_vertex"][:2])
    assert np.signbit(one["u"][0]) and one["u"][0] == 0     # -0 / -4: the zero's sign is not part of the contract


def test_empty_inputs():
    rays, b, _ = HAND["nearer_of_two_crossings"]
    none = tuple(x[:, :0] for x in b[:2]) + (b[2][:0],)
    assert cases.as_tuples(ref.ray_casts(rays, none)) == [cases.NO_HIT]
    assert len(ref.ray_casts(tuple(r[:0] for r in rays), b)) == 0
    assert ref.touched(rays, none).shape == (1, 0)


def test_a_bad_vertex_count_is_in_no_hit():
    rays, _, _ = HAND["nearer_square_later_in_the_set"]
    for bad in (0, 17, 200):
        vx, vy, k = cases.polys(cases.UNIT, cases.square(5.0))
        k[0] = bad
        assert cases.as_tuples(ref.ray_casts(rays, (vx, vy, k))) == [(1, 0.75, 0.5, 3, 1, 0)]
    vx, vy, _ = cases.polys(cases.UNIT, rows=4)
    assert cases.as_tuples(ref.ray_casts(rays, (vx, vy, None))) == [(0, 0.125, 0.5, 3, 1, 0)]      # no count plane: k = rows


@pytest.fixture(scope="module")
def scene(wl):
    rays, b = cases.ray_scene(wl)
    got = ref.ray_casts(rays, b)
    got.setflags(write=False)
    return rays, b, got


def test_scene_shares(scene):
    """A prototype of the contract gives 55.2 % hit, 11.0 % START_INSIDE and 44.2 % edge hits on this scene, with polygons of every k
    from 3 to 16 among the winners; each share is asserted at half its value."""
    rays, b, got = scene
    assert len(got) == 2000 and b[0].shape == (16, 311)
    hit, inside = got["hit"] == 1, got["flags"] == ref.START_INSIDE
    assert hit.mean() > 0.276 and inside.mean() > 0.055 and (hit & ~inside).mean() > 0.221
    assert set(b[2][got["poly"][hit]]) == set(range(3, 17))
    assert (got["t"][hit] >= 0).all() and (got["t"][hit] <= 1).all() and (got["t"][~hit] == np.inf).all()
    edge = hit & ~inside
    assert (got["edge"][edge] < b[2][got["poly"][edge]]).all() and (got["u"][edge] >= 0).all() and (got["u"][edge] <= 1).all()


def test_scene_against_the_same_rule_in_float64(scene):
    """The rule in float64 agrees on hit, poly and edge for all 2 000 rays, and t stays within 4 x 2.3e-7 of the float64 t (2.3e-7
    is the worst deviation a prototype of the contract showed on this scene; t <= 1, and tn and den each carry a few roundings of
    coordinates of magnitude below 64 times lengths below 24)."""
    rays, b, got = scene
    got64, t64 = ref.ray_casts(rays, b, dtype=np.float64, with_t=True)
    for f in ("hit", "poly", "edge", "flags"):
        assert np.array_equal(got[f], got64[f]), f
    hit = got["hit"] == 1
    worst = float(np.abs(got["t"][hit].astype(np.float64) - t64[hit]).max())
    print(f"worst |t - t64| = {worst:.3e}")
    assert worst <= 4 * 2.3e-7


def test_scene_against_the_pairwise_test_on_segments_as_2gons(scene):
    """Independent of the ray arithmetic: a segment is the 2-gon (o, o + d), and "the segment touches the polygon" is the pairwise
    SAT boolean of tests/contact_ref.py.  On all 622 000 (segment, polygon) pairs it equals "inside or some usable edge" — no pair
    left out.  (A prototype: 2 012 true on both sides.)"""
    rays, b, got = scene
    touched = ref.touched(rays, b)
    segs = cases.segments_as_2gons(rays, rows=16)
    i, j = np.divmod(np.arange(2000 * 311), 311)
    sat = contact_ref.poly_contacts(segs, b, i, j)["hit"].reshape(2000, 311) == 1
    print(f"touched {int(touched.sum())}, pairwise {int(sat.sum())}, differing {int((touched != sat).sum())}")
    assert touched.shape == sat.shape == (2000, 311)
    assert np.array_equal(touched, sat)
    assert np.array_equal(touched.any(axis=1), got["hit"] == 1)
    rows = np.flatnonzero(got["hit"] == 1)
    assert touched[rows, got["poly"][rows]].all()
