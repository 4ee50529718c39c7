"""What belongs to c2d_poly_sweep_broad_pairs alone in its tests (test_gpu_sweep_broad.py, tools/sweep_broad_fuzz.py, the grid casts'
scenes): the motions, the moving sparse scene, and check() against the reference (tests/sweep_broad_ref.py).  The device set with its
guarded motion planes, the list call between guard entries and the judge are tests/pair_search_harness.py's.  numpy only."""
import numpy as np

import pair_search_harness as psh
import sweep_broad_ref as ref


def motion(n, seed, lo=3.0, hi=9.0):
    """one displacement per polygon: a random direction, lo .. hi long (the scenes' polygons are about 3 across)"""
    rng = np.random.default_rng(seed)
    ang, mag = rng.uniform(0, 2 * np.pi, n), rng.uniform(lo, hi, n)
    return (mag * np.cos(ang)).astype(np.float32), (mag * np.sin(ang)).astype(np.float32)


def sparse_scene(wl, n, seed, rows=16, kmax=16, density=1.0):
    """(set, motion): the sparse scene of the polygon broad phase's tests, moving by one to three polygon sizes"""
    return psh.sparse_set(wl, n, seed, rows=rows, kmax=kmax, density=density), motion(n, seed + 7)


def check(eng, a, b, ma, mb, upper=False, min_pairs=1, want=None, place_a=(1, 3), place_b=(2, 0), with_k=True):
    """the list of (a, ma) against (b, mb) — b None: the set against itself, the same memory and the same planes — equals the
    reference; returns (list, reference list)"""
    A = psh.DeviceSet(eng, a, ma, offset=place_a[0], stride=a[0].shape[1] + place_a[1], with_k=with_k)
    B = A if b is None else psh.DeviceSet(eng, b, mb, offset=place_b[0], stride=b[0].shape[1] + place_b[1], with_k=with_k)
    try:
        got, total = psh.run(eng, psh.sweep_broad(eng, A, B, upper))
    finally:
        A.free()
        if B is not A:
            B.free()
    if want is None:
        want = ref.pairs(a, a if b is None else b, ma, ma if b is None else mb, upper=upper)
    why = psh.compare(got, total, want)
    assert why is None, why
    assert total >= min_pairs, total
    return got, want
