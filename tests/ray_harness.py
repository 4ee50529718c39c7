"""The frame of the GPU tests of c2d_poly_ray_casts: ray planes on the device at chosen 4-byte offsets, and cast() with guard bands
around the output (tests/pair_list_harness.py: banded / unband).  A plain module on numpy and the numpy reference only: it never
loads libc2d.so, so tests/ray_graph_check.py can import it after torch."""
import numpy as np

import pair_list_harness as h
import ray_ref as ref

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


def cast(eng, rays, n_rays, b_set, col_base=0, capacity=None, expect_error=False):
    """c2d_poly_ray_casts on the first n_rays rays of a RaysOnDevice into a banded output of `capacity` records -> RAY_HIT_DT[capacity];
    the bands and every record at or beyond n_rays must be untouched; under expect_error the synchronise reports status -1, once"""
    return h.banded_call(eng, DT, n_rays, lambda ptr: eng.poly_ray_casts(rays.ptrs, n_rays, b_set, ptr, col_base=col_base), capacity, expect_error)


def assert_same(got, want, what):
    ok = ref.same(got, want)
    if not ok.all():
        q = int(np.flatnonzero(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {len(want)} records differ; first at ray {q}: got {got[q]}, want {want[q]}")
