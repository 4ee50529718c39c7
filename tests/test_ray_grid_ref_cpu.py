"""CPU tests of tests/ray_grid_ref.py, the numpy restatement of the contract of c2d_poly_ray_casts_grid (include/c2d.h "ray queries
through a grid"): the hand cases keep their hand-written records; on the project's ray scenes, at every scale, a polygon the
brute-force rule touches is met by its ray (so there the two calls agree) while the candidates stay a small share of all pairs; the
near-collinear construction pins where the two calls differ; unboxed polygons and non-finite rays."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ray_cases as cases  # noqa: E402
import ray_grid_cases as gcases  # noqa: E402
import ray_grid_ref as gref  # noqa: E402
import ray_ref as ref  # noqa: E402

F = np.float32


@pytest.mark.parametrize("name", sorted(cases.hand_cases()))
def test_hand_cases_keep_their_records(name):
    rays, b, want = cases.hand_cases()[name]
    got = gref.ray_casts(rays, b)
    assert cases.as_tuples(got) == [tuple(w) for w in want], name
    assert not (ref.touched(rays, b) & ~gref.candidates(rays, b)).any(), "a touched polygon is no candidate"


@pytest.mark.parametrize("scale", [1.0, 1e-30, 1e-10, 1e10, 1e30])
def test_touched_implies_met_on_the_ray_scene(wl, scale):
    """622 000 pairs: every touched pair is a candidate, the candidates stay below 1 % of the pairs, and the records are the
    brute-force reference's, byte for byte"""
    rays, b = cases.ray_scene(wl)
    rays, b = tuple((r * F(scale)).astype(F) for r in rays), (b[0] * F(scale), b[1] * F(scale), b[2])
    touched, cand = ref.touched(rays, b), gref.candidates(rays, b)
    assert touched.size == 622_000 and touched.sum() > (1500 if 1e-20 < scale < 1e20 else -1)   # (at 1e-30 every product underflows)
    assert not (touched & ~cand).any()
    assert touched.sum() <= cand.sum() < 0.01 * cand.size
    assert gref.ray_casts(rays, b, col_base=5).tobytes() == ref.ray_casts(rays, b, col_base=5).tobytes()


def test_touched_implies_met_on_the_sparse_scene(wl):
    """the bench's 4096-polygon scene with its first 1000 rays (the GPU tests run all 4000 against the brute-force call)"""
    rays, b = gcases.sparse_scene(wl)
    rays = tuple(r[:1000] for r in rays)
    touched, cand = ref.touched(rays, b), gref.candidates(rays, b)
    assert touched.size == 4_096_000 and touched.sum() > 2_500
    assert not (touched & ~cand).any()
    assert touched.sum() <= cand.sum() < 0.01 * cand.size
    assert gref.ray_casts(rays, b).tobytes() == ref.ray_casts(rays, b).tobytes()


def test_near_collinear_rays_are_where_the_two_calls_differ():
    """400 000 rays on the line of an edge of a rotated square, 50 .. 2000 away from it: the brute-force rule reports more than a
    thousand hits there (den, tn and un are rounding noise); none of those polygons meets its ray, and the grid reference reports no
    hit at all."""
    rays, b = gcases.near_collinear()
    far = ref.ray_casts(rays, b)
    hits = far["hit"] == 1
    print(f"far hits of the brute-force rule: {int(hits.sum())} of {len(hits)}, START_INSIDE {int((far['flags'] == ref.START_INSIDE).sum())}")
    assert hits.sum() >= 1000
    met = gref.meets(rays, b)[:, 0]
    assert not met[hits].any()
    assert not met.any()
    assert (gref.ray_casts(rays, b)["hit"] == 0).all()


def test_unboxed_polygons_are_candidates_of_every_ray(wl):
    rays, b = cases.ray_scene(wl, n_rays=300)
    vx, vy, k = (x.copy() for x in b)
    nan_at = [3, 77, 200]
    for j in nan_at:
        vx[int(k[j]) - 1, j] = np.nan          # the last live vertex
    vy[0, 120] = np.nan
    vx[15, 50] = np.nan if k[50] < 16 else vx[15, 50]      # a padded slot: not live, the polygon keeps its box
    s = (vx, vy, k)
    box = gref.boxes(s)
    assert set(np.flatnonzero(box[4])) == set(nan_at + [120])
    cand = gref.candidates(rays, s)
    assert cand[:, nan_at + [120]].all() and not cand[:, 50].all()
    # the clean edges of an unboxed polygon are still hit, as in the brute-force call
    assert gref.ray_casts(rays, s).tobytes() == ref.ray_casts(rays, s).tobytes()
    # a bad count: no candidate of any ray
    k2 = k.copy()
    k2[10] = 0
    assert not gref.candidates(rays, (vx, vy, k2))[:, 10].any()


def test_non_finite_rays_meet_everything_and_hit_nothing(wl):
    _, b = cases.ray_scene(wl)
    nan, inf = np.nan, np.inf
    o = -500.0      # outside every polygon: a NaN direction leaves the inside rule, which does not look at d, alone
    rays = cases.rays_of((nan, o, 1, 0), (o, nan, 1, 0), (o, o, nan, 0), (o, o, 1, nan), (inf, o, 1, 0), (o, -inf, 1, 0), (inf, o, -inf, 0), (o, o, inf, 0))
    assert gref.meets(rays, b).all()
    got = gref.ray_casts(rays, b)
    assert (got["hit"][:7] == 0).all()
    # (an infinite direction from a finite origin can hit, with u = inf / inf: as in the brute-force call)
    assert ref.same(got, ref.ray_casts(rays, b)).all()
    # an infinite box meets every ray
    vx = b[0].copy()
    vx[0, 7] = inf
    assert gref.meets(cases.rays_of((0, 0, 1, 1), (-40, 3, 0, 0)), (vx, b[1], b[2]))[:, 7].all()
