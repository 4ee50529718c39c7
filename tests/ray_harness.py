"""What the GPU tests of c2d_poly_ray_casts and c2d_poly_ray_casts_grid have of their own: ray planes on the device at chosen 4-byte
offsets, and the grid check.  The call between guard bands, the call run twice and the comparison are the frame's
(tests/best_key_harness.py), bound to the two ray queries here.  A plain module on numpy and the numpy references only: it never
loads libc2d.so."""
import functools

import numpy as np

import best_key_harness as best
import ray_grid_ref as gref
import ray_ref as ref
from pair_list_harness import Uploaded

DT = ref.RAY_HIT_DT


class RaysOnDevice:
    """the four planes ox, oy, dx, dy in one allocation, plane p shifted by offsets[p] floats, NaN in the gaps"""

    def __init__(self, eng, rays, offsets=(0, 0, 0, 0)):
        self.n = len(rays[0])
        width = self.n + max(offsets) + 1
        host = np.full((4, width), np.nan, np.float32)
        for p in range(4):
            host[p, offsets[p]: offsets[p] + self.n] = rays[p]
        self.d = eng.to_device(host)
        self.ptrs = [self.d.row(p) + 4 * offsets[p] for p in range(4)]

    def free(self):
        self.d.free()


cast = functools.partial(best.call, best.RAY_CASTS)            # cast(eng, rays, n_rays, b_set, col_base=0, capacity=None, expect_error=False) -> DT[capacity]
cast_grid = functools.partial(best.call, best.RAY_CASTS_GRID)  # the same through c2d_poly_ray_casts_grid
twice = functools.partial(best.twice, best.RAY_CASTS)          # twice(eng, rays, n_rays, b_set, what, **kw): the call, run twice: the same bytes
twice_grid = functools.partial(best.twice, best.RAY_CASTS_GRID)
assert_same = functools.partial(best.assert_same, best.RAY_CASTS)      # assert_same(got, want, what): "... first at ray q ..."


def check_grid(eng, rays, b, what, n_rays=None, uploaded=None, on_device=None, **kw):
    """upload (unless handed in), run c2d_poly_ray_casts_grid twice, compare with the grid reference -> (records, the call's counters)"""
    n = len(rays[0]) if n_rays is None else n_rays
    dr = RaysOnDevice(eng, rays) if on_device is None else on_device
    ub = Uploaded(eng, b) if uploaded is None else uploaded
    try:
        got = twice_grid(eng, dr, n, ub.set, what, **kw)
        stats = eng.poly_ray_casts_grid_stats()
        assert_same(got, gref.ray_casts(tuple(r[:n] for r in rays), b, col_base=kw.get("col_base", 0)), what)
    finally:
        if on_device is None:
            dr.free()
        if uploaded is None:
            ub.free()
    return got, stats
