"""Inputs shared by the CPU and GPU tests of the ray queries (c2d_poly_ray_casts): the ray scene, the hand-computed cases with their
expected records (exact in binary32; tests/test_ray_ref_cpu.py derives each), and the segments as 2-gons for the cross-checks against
code the project already trusts.  A plain module on numpy only."""
import functools

import numpy as np

F = np.float32
NONE16, NONE32, INSIDE = 0xFFFF, 0xFFFFFFFF, 1
FIELDS = ("poly", "t", "u", "edge", "hit", "flags")
NO_HIT = (NONE32, np.inf, 0.0, NONE16, 0, 0)
NAN, INF = float("nan"), float("inf")


def polys(*vertex_lists, rows=16):
    """polygons given as vertex lists -> a set (vx [rows][n], vy, k)"""
    n = len(vertex_lists)
    vx, vy, k = np.zeros((rows, n), F), np.zeros((rows, n), F), np.zeros(n, np.uint8)
    for j, pts in enumerate(vertex_lists):
        k[j] = len(pts)
        for r, (x, y) in enumerate(pts):
            vx[r, j], vy[r, j] = x, y
    return vx, vy, k


def square(x0=0.0, y0=0.0, s=1.0):
    """counter-clockwise from (x0, y0): edge 0 the bottom, 1 the right side, 2 the top, 3 the left side"""
    return [(x0, y0), (x0 + s, y0), (x0 + s, y0 + s), (x0, y0 + s)]


def rays_of(*rows):
    """rays given as (ox, oy, dx, dy) rows -> the four planes"""
    a = np.array(rows, F).reshape(-1, 4)
    return tuple(np.ascontiguousarray(a[:, c]) for c in range(4))


UNIT = square()
CLOCKWISE = [UNIT[0], UNIT[3], UNIT[2], UNIT[1]]     # edge 0 the left side (upwards), 1 the top, 2 the right side, 3 the bottom


def hand_cases():
    """name -> (rays, set b, [expected record per ray]); every number is exact in binary32"""
    one = polys(UNIT)
    nan02 = [(NAN, NAN), UNIT[1], (NAN, NAN), UNIT[3]]      # every edge touches a NaN vertex
    nan0 = [(NAN, NAN), UNIT[1], UNIT[2], UNIT[3]]          # edges 1 and 2 are clean
    return {
        "nearer_of_two_crossings": (rays_of((-1, 0.5, 4, 0)), one, [(0, 0.25, 0.5, 3, 1, 0)]),
        "through_a_vertex": (rays_of((-1, -1, 4, 4)), one, [(0, 0.25, 0.0, 0, 1, 0)]),
        "along_an_edge": (rays_of((-1, 0, 4, 0)), one, [(0, 0.25, 1.0, 3, 1, 0)]),
        "ending_on_an_edge_and_short_of_it": (rays_of((-1, 0.5, 1, 0), (-1, 0.5, 0.75, 0)), one, [(0, 1.0, 0.5, 3, 1, 0), NO_HIT]),
        "origin_inside_and_on_the_boundary": (rays_of((0.5, 0.5, 4, 0), (0, 0.5, 4, 0), (0, 0.5, -4, 0), (1, 1, 1, 1)), one,
                                              [(0, 0.0, 0.0, NONE16, 1, INSIDE)] * 4),
        "point_queries": (rays_of((0.5, 0.5, 0, 0), (2, 2, 0, 0), (0, 0, 0, 0)), one,
                          [(0, 0.0, 0.0, NONE16, 1, INSIDE), NO_HIT, (0, 0.0, 0.0, NONE16, 1, INSIDE)]),
        "clockwise": (rays_of((-1, 0.5, 4, 0), (0.5, 0.5, 4, 0), (2, 2, 0, 0)), polys(CLOCKWISE),
                      [(0, 0.25, 0.5, 0, 1, 0), (0, 0.0, 0.0, NONE16, 1, INSIDE), NO_HIT]),
        "k1_is_never_hit": (rays_of((0, 0.5, 1, 0), (0.5, 0.5, 1, 0), (0.5, 0.5, 0, 0)), polys([(0.5, 0.5)]), [NO_HIT] * 3),
        "k2_crossed": (rays_of((-1, 0, 2, 0), (-1, 2, 2, 0)), polys([(0, -1), (0, 1)]), [(0, 0.5, 0.5, 0, 1, 0), NO_HIT]),
        "identical_squares": (rays_of((-1, 0.5, 4, 0), (0.5, 0.5, 0, 0)), polys(UNIT, UNIT, UNIT),
                              [(0, 0.25, 0.5, 3, 1, 0), (0, 0.0, 0.0, NONE16, 1, INSIDE)]),
        "nearer_square_later_in_the_set": (rays_of((-1, 0.5, 8, 0)), polys(square(5.0), UNIT), [(1, 0.125, 0.5, 3, 1, 0)]),
        "non_finite_rays": (rays_of((NAN, 0.5, 4, 0), (-1, 0.5, NAN, 0), (INF, 0.5, 4, 0), (-1, -INF, 4, 0)), one, [NO_HIT] * 4),
        "nan_vertices_beside_a_clean_polygon": (rays_of((-1, 0.5, 8, 0), (0.5, 0.5, 0, 0)), polys(nan02, square(3.0)),
                                                [(1, 0.5, 0.5, 3, 1, 0), NO_HIT]),
        "nan_vertex_with_clean_edges": (rays_of((-1, 0.5, 8, 0)), polys(nan0, square(3.0)), [(0, 0.25, 0.5, 1, 1, 0)]),
    }


def as_tuples(records):
    return [tuple(r[f].item() for f in FIELDS) for r in records]


@functools.lru_cache(maxsize=None)
def ray_scene(wl, n_rays=2000):
    """The ray scene: 311 convex polygons with 3..16 vertices in a box of +-48 and 2000 segments of length below 24 that start
    anywhere in it -> (rays, b), read-only"""
    b = wl.random_convex_polygon_set(311, seed=7102, kmin=3, kmax=16, extent=48.0, rows=16)
    rng = np.random.default_rng(9001)
    lo, hi = float(b[0][0].min()), float(b[0][0].max())
    ox = rng.uniform(lo, hi, n_rays)
    oy = rng.uniform(lo, hi, n_rays)
    ang = rng.uniform(0.0, 2.0 * np.pi, n_rays)
    length = rng.uniform(0.0, 24.0, n_rays)
    rays = tuple((v).astype(F) for v in (ox, oy, length * np.cos(ang), length * np.sin(ang)))
    for x in rays + tuple(b):
        x.setflags(write=False)
    return rays, b


def segments_as_2gons(rays, rows=2):
    """the segments as polygons with the two vertices o and o + d (the sum rounded to float32) -> a set (vx [rows][n], vy, k)"""
    ox, oy, dx, dy = rays
    n = len(ox)
    vx, vy = np.zeros((rows, n), F), np.zeros((rows, n), F)
    vx[0], vy[0], vx[1], vy[1] = ox, oy, ox + dx, oy + dy
    return vx, vy, np.full(n, 2, np.uint8)
