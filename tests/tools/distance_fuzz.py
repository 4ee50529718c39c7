#!/usr/bin/env python3
"""Differential fuzz of c2d_poly_pair_distances / c2d_rect_pair_distances against the CPU restatement of their contract
(tests/distance_ref.py, pinned by tests/test_distance_ref_cpu.py), after contact_fuzz.py: random set sizes, row layouts,
vertex-count ranges, densities, strides and pointer offsets, bases, list lengths and device counts, clockwise polygons, points and
segments, outliers, NaN / inf in real slots, junk in the padded slots, tied shapes (poly_broad_fuzz.py's random sets); rectangles as
random quads, one time in three on a 1/16 grid (exact ties), some with non-finite vertices.  This file is the generator; the call
and the judge are pair_list_fuzz.py's.  Prints its seed; a mismatch names its configuration.
usage: distance_fuzz.py [configs] [seed]     (no seed: the commit's, tests/tools/fuzz_seed.py)"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("pair_list_fuzz", os.path.join(HERE, "pair_list_fuzz.py"))
plf = importlib.util.module_from_spec(spec)
spec.loader.exec_module(plf)            # the back half of every list-driven fuzz tool: run(), its judge, main(); it puts tests/ on the path
h, wl, pbf = plf.h, plf.wl, plf.pbf
contact_fuzz = plf.tool("contact_fuzz")      # its random list

LAST = {}   # hits / misses of the last configuration, for the exploring leg's "not vacuous" check


def random_quads(rng, n):
    q = (rng.uniform(-3, 3, (1, n)) + rng.uniform(-2, 2, (8, n))).astype(np.float32)
    if rng.random() < 0.33:
        q = (np.round(q * 16) / 16).astype(np.float32)
    return q


def random_sets(rng, n_a, n_b):
    """two rectangle sets (random quads) three times in ten, else two polygon sets with where their planes go -> a, b, place (None for
    rectangles: plf.run), their description"""
    if rng.random() < 0.3:
        a = random_quads(rng, n_a)
        b = a if (n_a == n_b and rng.random() < 0.3) else random_quads(rng, n_b)
        if rng.random() < 0.3:
            a = wl.inject_non_finite(a, seed=int(rng.integers(1 << 30)), frac=0.1)
        return a, b, None, f"rectangles {n_a} x {n_b}"
    a, da = pbf.random_set(rng, n_a, int(rng.integers(1, 17)))
    same = bool(rng.random() < 0.3)
    b, db = (a, da) if same else pbf.random_set(rng, n_b, int(rng.integers(1, 17)))
    place = [(int(rng.integers(0, 4)), int(rng.integers(0, 9))) for _ in range(1 if same else 2)]      # (offset, stride - n) of a set's planes
    return a, b, place, f"polygons {n_a} x {b[0].shape[1]}, A {da}, B {'= A' if same else db}"


def one(eng, rng, idx, announce=None):
    """One configuration; `announce(text)` is called with its description BEFORE any GPU work.  Returns (ok, (description, records))."""
    n_a, n_b = (int(rng.choice([1, 2, 63, 64, 65, 257, int(rng.integers(1, 600))])) for _ in range(2))
    length = int(rng.choice([1, 63, 64, 65, 257, int(rng.integers(1, 5000))]))
    rb, cb = (int(rng.choice([0, 0, 7, 1 << 20, (1 << 32) - 700])) for _ in range(2))
    cap = length + int(rng.choice([0, 0, 1, 100]))
    n_dev = rng.choice([None, length, max(length - 1, 0), length // 2, cap + 5])
    a, b, place, what = random_sets(rng, n_a, n_b)
    desc = f"config {idx}: {what}, list {length} in {cap}, count {n_dev}, bases {rb}, {cb}"
    if announce is not None:
        announce(desc)
    pairs = contact_fuzz.random_list(rng, n_a, (b.shape if place is None else b[0].shape)[1], length)
    ok, info, wants = plf.run(eng, h.DISTANCES, desc, a, b, pairs, cap, n_dev, rb, cb, place)
    LAST.update(plf.hits_and_misses(wants))
    return ok, info


if __name__ == "__main__":
    plf.main("distance_fuzz", one, "records")
