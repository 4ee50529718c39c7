#!/usr/bin/env python3
"""Differential fuzz of c2d_sat_rect_broad_pairs against c2d_sat_rect_cross_pairs (itself held to the oracle by cross_fuzz.py and
tests/test_gpu_sat_cross.py), as poly_broad_fuzz.py does for polygons: count and list bytes.  Self and two-set mode, upper on or off,
sizes on both sides of the wave, of the 2048-entry sort tile and up to 12 000; on top of a random scene it draws piles — clusters
whose rows have more than 16 hits (the short route's limit), more than 512 (the middle route's) and more than 1024 sorted
candidates — and wild and absent objects: boxes that cover the scene, coordinates at and beyond 2^60, NaN / inf, points, rectangles
at 1e30 that meet nothing.  Now and then the capacity is below the total: the list must be the prefix with nothing written behind it.
compare() is the judge (a pure function on host arrays, tests/test_fuzz_compare_cpu.py).  Prints its seed; a mismatch names its
configuration.
usage: broad_fuzz.py [configs] [seed]     (no seed: the commit's, tests/tools/fuzz_seed.py)"""
import importlib
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.dirname(HERE), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
from __graft_entry__ import load_package  # noqa: E402
from pair_search_harness import GUARD, SENTINEL  # noqa: E402  (the guard entries around a list, as run() of the harness lays them)

pkg = load_package()
wl = importlib.import_module("c2d_amd.workloads")
F = np.float32
PILES = [0, 0, 20, 40, 600, 1100, 1300]        # members per side: beyond 16 hits, beyond 512, beyond 1024 candidates
LAST = {}


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fuzz_seed = _tool("fuzz_seed")


def compare(got, got_total, want, want_total, capacity):
    """got, want: u32 [GUARD + capacity + GUARD][2] as the broad call and the cross call left buffers of SENTINEL bytes; the totals:
    what each added to a zeroed counter -> the list of complaints"""
    out = []
    if got_total != want_total:
        out.append(f"the broad phase counts {got_total}, the cross form {want_total}")
    if got.shape != (capacity + 2 * GUARD, 2) or want.shape != got.shape:
        return out + [f"list buffers of shapes {got.shape}, {want.shape} for a capacity of {capacity}"]
    g, w = got.view(np.uint64).reshape(-1), want.view(np.uint64).reshape(-1)
    n = min(capacity, want_total)
    for name, flat in (("broad", g), ("cross", w)):
        if not (flat[:GUARD] == SENTINEL).all():
            out.append(f"{name}: written in front of the list")
        if not (flat[GUARD + n:] == SENTINEL).all():
            out.append(f"{name}: written behind the list (past the capacity or past the total)")
    differ = np.flatnonzero(g[GUARD: GUARD + n] != w[GUARD: GUARD + n])
    if len(differ):
        q = int(differ[0])
        out.append(f"{len(differ)} of {n} list entries differ; first at {q}: broad {got[GUARD + q].tolist()}, cross {want[GUARD + q].tolist()}")
    return out


def random_scene(rng, n, oracle, extent, pile, centre):
    """f32 [8][n]: random poses in a box of +-extent; the first `pile` of them heaped around `centre`; a few wild ones -> planes, wild"""
    pp = wl.random_obb_pose_planes(n, seed=int(rng.integers(1 << 30)), extent=extent)[:5].copy()
    m = min(pile, n)
    if m:
        spread = float(rng.choice([0.05, 1.5]))       # all of them collide / their boxes overlap and some collide
        where = rng.permutation(n)[:m]
        pp[0, where] = centre[0] + rng.uniform(-spread, spread, m)
        pp[1, where] = centre[1] + rng.uniform(-spread, spread, m)
    s = oracle.rects_from_poses(*pp).copy()
    wild = 0
    with np.errstate(all="ignore"):
        for q in np.flatnonzero(rng.random(n) < float(rng.choice([0.0, 0.002, 0.02]))):
            what = int(rng.integers(0, 6))
            wild += 1
            if what == 0:
                s[:, q] = np.array([-1, -1, 1, -1, 1, 1, -1, 1], F) * F(extent * rng.choice([0.3, 2.0, 1e4]))      # a box over the scene
            elif what == 1:
                s[:, q] += F(rng.choice([1e30, 2.0 ** 60, -2.0 ** 61, 1e-30]))
            elif what == 2:
                s[int(rng.integers(0, 8)), q] = rng.choice(np.array([np.nan, np.inf, -np.inf, 3e38], F))
            elif what == 3:
                s[:, q] = np.nan
            elif what == 4:
                s[:, q] = np.tile(s[:2, q], 4)                                                                      # a point
            else:
                s[:, q] *= F(10.0 ** rng.integers(2, 7))
    return s, wild


def one(eng, rng, idx, announce=None, oracle=None):
    """One configuration; `announce(text)` is called with its description BEFORE any GPU work.  Returns (ok, (description, hits))."""
    if oracle is None:
        from oracle import cpu as oracle
    sizes = [1, 2, 63, 64, 65, 257, 2047, 2049, int(rng.integers(1, 3000)), int(rng.integers(3000, 12_001))]
    n_a, n_b = int(rng.choice(sizes)), int(rng.choice(sizes))
    self_mode, upper = bool(rng.random() < 0.4), bool(rng.random() < 0.5)
    pile = int(rng.choice(PILES))
    density = float(rng.choice([0.5, 1.0, 2.0, 4.0]))
    extent = 400.0 * np.sqrt(max(n_a if self_mode else max(n_a, n_b), 64) / 32768) / density
    centre = rng.uniform(-extent / 2, extent / 2, 2)
    a, wild = random_scene(rng, n_a, oracle, extent, pile, centre)
    if self_mode:
        b, n_b = a, n_a
    else:
        b, wild_b = random_scene(rng, n_b, oracle, extent, pile, centre)
        wild += wild_b
    short = bool(rng.random() < 0.3)
    desc = (f"config {idx}: {'self mode n ' + str(n_a) if self_mode else f'two sets {n_a} x {n_b}'}, upper {upper}, extent {extent:.1f}, "
            f"pile {min(pile, n_a, n_b)}, wild {wild}, capacity {'below the total' if short else 'the total'}")
    if announce is not None:
        announce(desc)
    da = eng.to_device(a)
    db = da if self_mode else eng.to_device(b)
    pa, pb = [da.row(k) for k in range(8)], [db.row(k) for k in range(8)]
    d_cnt = eng.zeros(4, np.uint64)
    bufs = []
    try:
        eng.sat_rect_cross_pairs(pa, n_a, pb, n_b, None, 0, d_cnt.ptr, upper=upper)          # count-only calls
        eng.sat_rect_broad_pairs(pa, n_a, pb, n_b, None, 0, d_cnt.ptr + 8, upper=upper)
        want_n, got_n = (int(x) for x in d_cnt.get()[:2])
        cap = want_n // 3 if short else want_n
        for _ in range(2):
            bufs.append(eng.empty((cap + 2 * GUARD, 2), np.uint32))
            eng.memset(bufs[-1], 0xA5, bufs[-1].nbytes)
        eng.sat_rect_cross_pairs(pa, n_a, pb, n_b, bufs[0].ptr + 8 * GUARD, cap, d_cnt.ptr + 16, upper=upper)
        eng.sat_rect_broad_pairs(pa, n_a, pb, n_b, bufs[1].ptr + 8 * GUARD, cap, d_cnt.ptr + 24, upper=upper)
        eng.synchronize()
        eng.check_async()
        totals = [int(x) for x in d_cnt.get()]
        want, got = bufs[0].get(), bufs[1].get()
    finally:
        for x in [da, d_cnt] + bufs + ([] if self_mode else [db]):
            x.free()
    complaints = compare(got, totals[3], want, totals[2], cap)
    if not (want_n == got_n == totals[2]):
        complaints.append(f"count-only calls: cross {want_n}, broad {got_n}; with a buffer the cross form counts {totals[2]}")
    tested = n_a * n_b if not upper else sum(max(0, n_b - 1 - i) for i in range(min(n_a, n_b)))
    LAST.update(hits=want_n, misses=tested - want_n)
    if complaints:
        print(f"MISMATCH {desc}: " + "; ".join(complaints))
    return not complaints, (desc, want_n)


def main():
    configs = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed, origin = (int(sys.argv[2]), "the command line") if len(sys.argv) > 2 else fuzz_seed.commit_seed()
    print(f"broad_fuzz: {configs} configurations, seed {seed} ({origin})", flush=True)
    from oracle import cpu as oracle
    eng = pkg.Engine(0)
    fails = hits = 0
    for i in range(configs):
        ok, info = one(eng, np.random.default_rng([seed, i]), i, None, oracle)
        fails += not ok
        hits += info[-1]
        if (i + 1) % 50 == 0:
            print(f"  {i + 1} / {configs} configurations, {fails} failures so far", flush=True)
    print(f"{configs} configurations, {fails} failures; {hits} colliding pairs compared")
    eng.close()
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    main()
