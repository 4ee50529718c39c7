"""CPU tests that pin tests/sweep_broad_ref.py — the judge of c2d_poly_sweep_broad_pairs — on the reference alone: what it must say
of scenes at rest, of a bullet, of equal motions and of the upper triangle, and that its two routes (all pairs through
sweep_ref.poly_sweeps; the same after dropping pairs its own pick misses on single axes) give one list."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cast_cases as cases  # noqa: E402
import sweep_broad_ref as ref  # noqa: E402
import sweep_ref  # noqa: E402

F32 = np.float32


def scene(wl, n, seed, extent=20.0, rows=16, kmax=16):
    s = wl.random_convex_polygon_set(n, seed=seed, kmin=min(3, kmax), kmax=kmax, extent=extent, rows=rows)
    rng = np.random.default_rng(seed)
    ang, mag = rng.uniform(0, 2 * np.pi, n), rng.uniform(3, 9, n)
    return s, ((mag * np.cos(ang)).astype(F32), (mag * np.sin(ang)).astype(F32))


def test_zero_motion_is_the_static_cross_list(oracle, wl):
    (a, _), (b, _) = scene(wl, 300, 1), scene(wl, 211, 2, rows=7, kmax=7)
    a = (a[0], a[1], a[2].copy())
    a[2][[3, 77]] = [0, 17]                                   # absent polygons are in no pair of either list
    static = ref.static_pairs(oracle, a, b)
    assert 300 < len(static) < 300 * 211 // 4
    assert not np.isin(static[:, 0], [3, 77]).any()
    zeros = lambda n: (np.zeros(n, F32), np.zeros(n, F32))    # noqa: E731
    for ma, mb in ((None, None), (zeros(300), zeros(211)), (None, zeros(211)), (zeros(300), None)):
        assert np.array_equal(ref.pairs(a, b, ma, mb), static)
    assert np.array_equal(ref.pairs(a, a, None, None, upper=True), ref.static_pairs(oracle, a, a, upper=True))


def test_a_bullet_is_listed(oracle):
    """a thin bullet crosses a thin wall within the step: separated at t = 0 and at t = 1, and at 16 sampled instants between"""
    a = cases.polys([(0, 0), (0.25, 0), (0.25, 0.25), (0, 0.25)])
    b = cases.polys([(10, -5), (10.25, -5), (10.25, 5), (10, 5)], cases.box(40, 40))
    ma = cases.move((20.4, 0))
    assert ref.pairs(a, b, ma, None).tolist() == [[0, 0]]
    assert len(ref.static_pairs(oracle, a, b)) == 0
    for t in np.linspace(0, 1, 16):
        moved = ((a[0] + F32(t) * ma[0]).astype(F32), (a[1] + F32(t) * ma[1]).astype(F32), a[2])
        assert len(ref.static_pairs(oracle, moved, b)) == 0, t
    assert ref.pairs(a, b, None, cases.move((-20.4, 0), (0, 0))).tolist() == [[0, 0]]       # the wall flies, the bullet rests
    assert ref.pairs(a, b, cases.move((5, 0)), None).tolist() == []                          # too slow to arrive


def test_equal_motions_give_the_static_list(oracle, wl):
    (a, _), (b, _) = scene(wl, 200, 3), scene(wl, 150, 4)
    d = (np.full(200, 7.5, F32), np.full(200, -3.25, F32)), (np.full(150, 7.5, F32), np.full(150, -3.25, F32))
    static = ref.static_pairs(oracle, a, b)
    assert len(static) > 100 and np.array_equal(ref.pairs(a, b, *d), static)


def test_upper_is_the_upper_triangle_of_the_full_list(wl):
    a, ma = scene(wl, 260, 5)
    full = ref.pairs(a, a, ma, ma)
    upper = ref.pairs(a, a, ma, ma, upper=True)
    assert np.array_equal(upper, full[full[:, 1] > full[:, 0]]) and len(upper) > 200
    assert (full[:, 0] == full[:, 1]).sum() == 260                                           # every polygon overlaps itself at t = 0
    # one set against itself with OTHER motions is two sets: more pairs than its own motion gives
    other = (ma[0][::-1].copy(), ma[1][::-1].copy())
    assert not np.array_equal(ref.pairs(a, a, ma, other), full)


def test_both_routes_give_one_list(wl):
    (a, ma), (b, mb) = scene(wl, 400, 6, extent=40.0), scene(wl, 300, 7, extent=40.0, rows=9, kmax=9)
    b = (b[0], b[1], b[2].copy())
    b[2][[0, 250, 299]] = [0, 10, 255]
    b[2][[7, 8]] = [1, 2]                                      # a point and a segment
    mb[0][5], ma[1][9] = np.nan, np.inf
    for upper, (x, y, mx, my) in ((False, (a, b, ma, mb)), (True, (a, a, ma, ma)), (False, (b, a, mb, None))):
        direct = ref.pairs(x, y, mx, my, upper=upper, direct_limit=1 << 40)
        staged = ref.pairs(x, y, mx, my, upper=upper, direct_limit=0, chunk=1 << 16)
        assert np.array_equal(direct, staged) and len(direct) > 300
        ii, jj = direct[:, 0].astype(np.int64), direct[:, 1].astype(np.int64)
        assert (sweep_ref.poly_sweeps(x, y, ii, jj, mx, my)["hit"] == 1).all()
        assert (np.diff(ii * y[0].shape[1] + jj) > 0).all(), "row-major, no pair twice"
