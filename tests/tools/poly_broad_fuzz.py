#!/usr/bin/env python3
"""Differential fuzz of c2d_sat_poly_broad_pairs against c2d_sat_poly_cross_pairs (itself pinned to the oracle by
tests/test_gpu_sat_poly_cross.py): random set sizes, row layouts, vertex-count ranges, densities, strides and pointer offsets, self
and two-set mode, clockwise polygons, points and segments, outliers, NaN / inf in real slots, junk in the padded slots.  Prints its
seed; a mismatch names its configuration.
usage: poly_broad_fuzz.py [configs] [seed]"""
import os
import sys

import numpy as np

TESTS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (TESTS, os.path.dirname(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)
from __graft_entry__ import load_package  # noqa: E402
import importlib  # noqa: E402
import pair_search_harness as psh  # noqa: E402

pkg = load_package()
wl = importlib.import_module("c2d_amd.workloads")


LAST = {}   # hits / misses of the last configuration, for the exploring leg's "not vacuous" check


def random_set(rng, n, rows):
    kmax = int(rng.integers(1, rows + 1))
    kmin = int(rng.integers(1, kmax + 1))
    density = float(rng.choice([0.5, 1.0, 2.0, 4.0, 16.0]))
    if n > 3000:
        density = min(density, 4.0)   # (large and dense at once is the cross form's scene: millions of pairs per configuration)
    extent = 200.0 * np.sqrt(max(n, 16) / 32768) / density
    vx, vy, k = wl.random_convex_polygon_set(n, seed=int(rng.integers(1 << 30)), kmin=kmin, kmax=kmax, extent=extent, rows=rows)
    vx, vy = vx.copy(), vy.copy()
    for q in np.flatnonzero(rng.random(n) < 0.2):          # clockwise
        kk = int(k[q])
        vx[:kk, q], vy[:kk, q] = vx[:kk, q][::-1].copy(), vy[:kk, q][::-1].copy()
    odd = np.flatnonzero(rng.random(n) < 0.02)             # outliers, huge coordinates, non-finite real vertices
    for q in odd:
        what = int(rng.integers(0, 4))
        r = int(rng.integers(0, k[q]))
        if what == 0:
            vx[:, q] *= np.float32(10.0 ** rng.integers(2, 7))
        elif what == 1:
            vy[:, q] += np.float32(rng.choice([1e30, 2.0 ** 60, -2.0 ** 61, 1e-30]))
        else:
            (vx if what == 2 else vy)[r, q] = rng.choice(np.array([np.nan, np.inf, -np.inf, 3e38], np.float32))
    junk = np.array([np.nan, np.inf, -np.inf, 3e38, -1e-40, 0.0], np.float32)
    pad = np.arange(rows)[:, None] >= k[None, :]
    vx[pad], vy[pad] = rng.choice(junk, int(pad.sum())), rng.choice(junk, int(pad.sum()))
    return (vx, vy, k), f"rows {rows} k {kmin}..{kmax} density {density}"


def upload(eng, s, offset, stride):
    """(c2d_poly_set, the device arrays to free) in pair_search_harness.DeviceSet's layout, for the tools that manage their own buffers"""
    u = psh.DeviceSet(eng, s, offset=offset, stride=stride)
    return u.set, (u.d, u.dk)


def one(eng, rng, idx, announce=None):
    """One configuration; `announce(text)` is called with its description BEFORE any GPU work, so that a fault names its input.
    Returns (ok, (description, hits))."""
    sizes = [1, 2, 63, 64, 65, 257, 2049, int(rng.integers(1, 3000)), int(rng.integers(3000, 12_000))]
    n_a, n_b = int(rng.choice(sizes)), int(rng.choice(sizes))
    self_mode, upper = bool(rng.random() < 0.4), bool(rng.random() < 0.5)
    a, da = random_set(rng, n_a, int(rng.integers(1, 17)))
    A = B = psh.DeviceSet(eng, a, offset=int(rng.integers(0, 4)), stride=n_a + int(rng.integers(0, 9)))
    if self_mode:
        desc = f"config {idx}: self n {n_a} {da} upper {upper}"
    else:
        b, db = random_set(rng, n_b, int(rng.integers(1, 17)))
        B = psh.DeviceSet(eng, b, offset=int(rng.integers(0, 4)), stride=n_b + int(rng.integers(0, 9)))
        desc = f"config {idx}: {n_a} x {n_b}, A {da}, B {db}, upper {upper}"
    if announce is not None:
        announce(desc)
    try:                                                       # (each: a count-only call, then the list between guard entries)
        want, want_n = psh.run(eng, psh.poly_cross(eng, A, B, upper))
        got, got_n = psh.run(eng, psh.poly_broad(eng, A, B, upper))
    finally:
        A.free()
        if B is not A:
            B.free()
    why = psh.compare(got, got_n, want)
    LAST.update(hits=want_n, misses=(n_a * B.n if not upper else sum(max(0, B.n - 1 - i) for i in range(n_a))) - want_n)
    if why is not None:
        print(f"MISMATCH {desc}: cross counts {want_n}; {why}")
    return why is None, (desc, want_n)


def main():
    configs = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 2026
    print(f"poly_broad_fuzz: {configs} configurations, seed {seed}", flush=True)
    rng = np.random.default_rng(seed)
    eng = pkg.Engine(0)
    fails = hits = 0
    for i in range(configs):
        ok, info = one(eng, rng, i)
        fails += not ok
        hits += info[-1]
        if (i + 1) % 50 == 0:  # a sign of life for long runs
            print(f"  {i + 1} / {configs} configurations, {fails} failures so far", flush=True)
    print(f"{configs} configurations, {fails} failures; {hits} colliding pairs compared")
    eng.check_async()
    eng.close()
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    main()
