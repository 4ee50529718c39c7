"""GPU tests of c2d_poly_ray_casts_grid where its grid decides (tests/ray_grid_walk_cases.py; tests/test_ray_grid_walk_cases_cpu.py proves
each construction on the CPU): box corners and ray ends on cell borders, the 65 535-cell cap, offsets at which the walk's widening is a
fraction of a cell and several cells, grids of one and two rows and of one column, rays a few ulps either side of meets' threshold, and
the near-collinear construction on each of the three routes that evaluate meets.  Every call is banded, run twice for equal bytes and
compared with tests/ray_grid_ref.py field for field.  On the table's scenes the call's counters are exact: `candidates` is the
reference's count of met pairs, and `visited` is the total of tests/ray_grid_model.py — the one number that ties the grid and the walk
the device builds to the model, and through the CPU test to csrc/c2d_ray_walk.hpp."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ray_grid_model as model  # noqa: E402
import ray_grid_ref as gref  # noqa: E402
import ray_grid_walk_cases as wc  # noqa: E402
import ray_ref as ref  # noqa: E402
from pair_list_harness import Uploaded  # noqa: E402
from ray_harness import RaysOnDevice, assert_same, cast, twice_grid as twice  # noqa: E402

pytestmark = pytest.mark.gpu


def run(eng, name, pick=None, what=None):
    """the scene's rays (those of `pick`) against its polygons: run twice, compared with the grid reference -> (records, counters,
    the brute-force call's records of the same run for the scenes that are compared with it)"""
    rays, b = wc.scene(name)
    want = wc.grid_records(name)
    if pick is not None:
        rays, want = tuple(r[pick] for r in rays), want[pick]
    what = what or name
    n = len(rays[0])
    dr, ub = RaysOnDevice(eng, rays), Uploaded(eng, b)
    try:
        got = twice(eng, dr, n, ub.set, what)
        stats = eng.poly_ray_casts_grid_stats()
        brute = cast(eng, dr, n, ub.set) if name in wc.COMPARED_WITH_BRUTE_FORCE + wc.COLLINEAR else None
    finally:
        dr.free()
        ub.free()
    assert_same(got, want, what)
    return got, stats, brute


def exact_counters(name, stats, pick=None, what=None):
    """no listed ray, no outlier, and both counters exact: with no outlier, no wild polygon and no listed ray every sorted entry is
    visited at most once per ray and every met box is visited, so `candidates` is an equality and not a bound"""
    rays, b = wc.scene(name)
    _, walks = wc.modelled(name)
    pick = np.ones(len(walks), bool) if pick is None else pick
    cand = int(gref.candidates(tuple(r[pick] for r in rays), b).sum())
    visited = int(sum(w.visited for w, p in zip(walks, pick) if p))
    print(f"{what or name}: {int(pick.sum())} rays, model: visited {visited}, candidates {cand}; device: {stats}")
    assert stats["listed"] == 0 and stats["outliers"] == 0, (what or name, stats)
    assert stats["candidates"] == cand, (what or name, stats, cand)
    assert stats["visited"] == visited, (what or name, stats, visited)


@pytest.mark.parametrize("name", [n for n in wc.TABLE if n != "grazing"])
def test_scene(eng, name):
    """borders, the cap on one axis and on both, the four offsets, the three strips; the offset and cap scenes also equal the
    brute-force call of the same run (touched implies met there: tests/test_ray_grid_walk_cases_cpu.py)"""
    got, stats, brute = run(eng, name)
    exact_counters(name, stats)
    if name in wc.COMPARED_WITH_BRUTE_FORCE:
        assert got.tobytes() == brute.tobytes(), f"{name}: differs from c2d_poly_ray_casts"
    eng.check_async()


@pytest.mark.parametrize("name", ["grazing", "grazing_skew"])
def test_grazing(eng, name):
    """grazing: rays a few float ulps either side of the threshold of meets against their own box; grazing_skew: long rays of general
    direction for which the two sides of sn agree to a few units in the last place of binary64, so that the rounding of its products
    decides.  Three calls each, so that a missed box and a falsely met one cannot cancel in the sum: the rays that meet their own
    box, those that do not, and all of them"""
    own = wc.grazing_meets_own_box(name)
    for what, pick in ((f"{name}: rays that meet", own), (f"{name}: rays that do not meet", ~own), (f"{name}: all rays", None)):
        _, stats, _ = run(eng, name, pick=pick, what=what)
        exact_counters(name, stats, pick=pick, what=what)
    eng.check_async()


@pytest.mark.parametrize("name", wc.COLLINEAR)
def test_near_collinear(eng, name):
    """rays on the line of an edge of the rotated square, far away from it: the brute-force call reports the far hits of its contract,
    the grid call reports none of them — decided by meets on the sorted box (collinear_regular), on the box made on the way for a wild
    polygon (collinear_wild) and in the list kernel (collinear_listed)"""
    got, stats, brute = run(eng, name)
    assert_same(brute, wc.brute_records(name), f"{name}: c2d_poly_ray_casts")
    far = wc.collinear_square_hits(name)
    differ = ~ref.same(got, brute)
    print(f"{name}: {int(far.sum())} far hits on the square by the reference, the two calls differ in {int(differ.sum())} records; {stats}")
    assert far.sum() >= 20 and differ.sum() >= far.sum() and differ[far].all()
    assert (got["hit"][differ] == 0).all()
    # the counters: every walk's visited entries are the model's (a listed ray's aborted walk counts the cap); no sorted box is met
    rays, b = wc.scene(name)
    g, walks = wc.modelled(name)
    visited = int(sum(w.visited for w in walks))
    cand = int(gref.candidates(rays, b)[:, g.kind != model.WILD].sum()) if name != "collinear_listed" else 0
    print(f"{name}: model: visited {visited}, candidates among the sorted boxes {cand}")
    assert stats["outliers"] == 0 and stats["visited"] == visited and stats["candidates"] == cand, (stats, visited, cand)
    if name == "collinear_listed":
        assert stats["listed"] >= len(far), stats
    else:
        assert stats["listed"] == 0, stats
    eng.check_async()
