"""Inputs shared by the CPU and GPU tests of c2d_poly_ray_casts_grid beyond tests/ray_cases.py: the 4096-polygon sparse scene of the
bench, the near-collinear construction that pins where the grid call and the brute-force call differ, and scenes built so that a ray
visits a chosen number of sorted grid entries.  A plain module on numpy only."""
import functools

import numpy as np

import ray_cases as cases

F = np.float32
WALK_CAP = 1024          # kRayWalkCap of csrc/c2d_ray_grid.hip: a ray that would visit more sorted entries goes to the list


@functools.lru_cache(maxsize=None)
def sparse_scene(wl, n_b=4096, n_rays=4000):
    """csrc/tools/ray_bench.py's scene: n_b convex polygons over +-extent, extent = 200 sqrt(n_b / 32768), and segments of length below
    24 that start anywhere in it -> (rays, b), read-only"""
    extent = 200.0 * np.sqrt(n_b / 32768)
    b = wl.random_convex_polygon_set(n_b, seed=0xC505, extent=extent)
    rng = np.random.default_rng(0x5E6)
    ox, oy = rng.uniform(-extent, extent, n_rays), rng.uniform(-extent, extent, n_rays)
    ang, length = rng.uniform(0.0, 2.0 * np.pi, n_rays), rng.uniform(0.0, 24.0, n_rays)
    rays = tuple(v.astype(F) for v in (ox, oy, length * np.cos(ang), length * np.sin(ang)))
    for x in rays + tuple(b):
        x.setflags(write=False)
    return rays, b


def nudged(v, rng, ulps=3):
    """float32 values moved by -ulps..+ulps units in the last place"""
    bits = np.ascontiguousarray(v, F).view(np.int32).astype(np.int64)
    step = rng.integers(-ulps, ulps + 1, len(bits))
    return (bits + np.where(bits < 0, -step, step)).astype(np.int32).view(F)


def near_collinear(n=400_000, seed=1701, angle=0.37):
    """The unit square rotated by `angle` about the origin, and n rays of length 0.2 .. 5 that lie, up to 3 ulp per coordinate, on the
    line of its edge 0, 50 .. 2000 away from the square on either side -> (rays, b)"""
    c, s = np.cos(angle), np.sin(angle)
    pts = [(F(x * c - y * s), F(x * s + y * c)) for x, y in cases.UNIT]
    b = cases.polys(pts)
    rng = np.random.default_rng(seed)
    (x0, y0), (x1, y1) = [(float(p[0]), float(p[1])) for p in pts[:2]]
    ux, uy = x1 - x0, y1 - y0
    norm = np.hypot(ux, uy)
    ux, uy = ux / norm, uy / norm
    away = rng.uniform(50.0, 2000.0, n)
    side = rng.random(n) < 0.5
    start = np.where(side, 1.0 + away, -away - 5.0)            # the whole ray stays at least 50 off the edge's ends
    length = rng.uniform(0.2, 5.0, n) * np.where(rng.random(n) < 0.5, 1.0, -1.0)
    start = np.where(length < 0, start + 5.0, start)
    rays = (x0 + ux * start, y0 + uy * start, ux * length, uy * length)
    return tuple(nudged(v.astype(F), rng) for v in rays), b


def cluster_scene(n_cluster, spread=40):
    """n_cluster copies of one small square at the origin among spread x spread unit-spaced squares of the same size that begin 20
    cells away: a point ray at the cluster visits exactly the n_cluster entries of the cluster's cell (its neighbours are empty)
    -> (set b, the ray planes of two point rays in the cluster and one segment far from it)"""
    small = 0.25
    far = [cases.square(20.0 + 2.0 * (i % spread), 20.0 + 2.0 * (i // spread), small) for i in range(spread * spread)]
    b = cases.polys(*([cases.square(0.0, 0.0, small)] * n_cluster + far))
    rays = cases.rays_of((0.125, 0.125, 0, 0), (-0.5, 0.125, 1.0, 0), (20.1, 20.1, 3.0, 1.0))
    return b, rays
