#!/usr/bin/env python3
"""Differential fuzz of c2d_poly_pair_manifolds against the CPU restatement of its contract (tests/manifold_ref.py, pinned by
tests/test_manifold_ref_cpu.py) under the equality tests/pair_list_harness.py's MANIFOLDS entry uses, on contact_fuzz.py's polygon
configurations: its random sets (sizes, row layouts, strides and pointer offsets, clockwise polygons, points and segments, outliers,
NaN / inf, junk in the padded slots, the same memory on both sides), its lists (row-major, a few entries out of their set), bases,
capacities and device counts, and one configuration in five its near-tied polygons at a power-of-two scale.  This file is the
generator; the call and the judge are pair_list_fuzz.py's: both outputs record by record, the guard bands around both buffers,
every record at or beyond min(n_pairs, *d_n_pairs) untouched, a bad entry reported once.  Prints its seed; a mismatch names
its configuration.
usage: manifold_fuzz.py [configs] [seed]     (no seed: the commit's, tests/tools/fuzz_seed.py)"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("pair_list_fuzz", os.path.join(HERE, "pair_list_fuzz.py"))
plf = importlib.util.module_from_spec(spec)
spec.loader.exec_module(plf)            # the back half of every list-driven fuzz tool: run(), its judge, main(); it puts tests/ on the path
h, pbf = plf.h, plf.pbf
cfz = plf.tool("contact_fuzz")         # its generators: random_list, and through it contact_cases' near-ties
cases = cfz.cases

LAST = {}


def one(eng, rng, idx, announce=None, oracle=None):
    """One configuration; `announce(text)` is called with its description BEFORE any GPU work.  Returns (ok, (description, pairs)).
    (`oracle` is not used: the reference is numpy.)"""
    n_a, n_b = (int(rng.choice([1, 2, 63, 64, 65, 257, int(rng.integers(1, 600))])) for _ in range(2))
    length = int(rng.choice([1, 63, 64, 65, 257, int(rng.integers(1, 5000))]))
    near_tie = bool(rng.random() < 0.2)
    if near_tie:
        n_a = n_b = length = int(rng.integers(200, 600))
    rb, cb = (int(rng.choice([0, 0, 7, 1 << 20, (1 << 32) - 700])) for _ in range(2))
    cap = length + int(rng.choice([0, 0, 1, 100]))
    n_dev = rng.choice([None, length, max(length - 1, 0), length // 2, cap + 5])
    place = [(int(rng.integers(0, 4)), int(rng.integers(0, 9))) for _ in range(2)]
    if near_tie:
        lo = float(rng.uniform(-28.0, -20.0))
        g_log2, k, seed = (lo, lo + float(rng.uniform(2.0, 10.0))), int(rng.integers(-52, 53)), int(rng.integers(1 << 30))
        a, b = (cases.scaled_poly_set(x, k) for x in cases.near_tie_poly_sets(n_a, seed, g_log2))
        what = f"near-ties, polygons {n_a} x {n_b} (generator seed {seed}, |g| in 2^{g_log2[0]:.1f} .. 2^{g_log2[1]:.1f}, scale 2^{k})"
        order = rng.permutation(n_a)
        pairs = np.stack([order, order], axis=1).astype(np.int64)
    else:
        a, da = pbf.random_set(rng, n_a, int(rng.integers(1, 17)))
        same = bool(rng.random() < 0.3)
        b, db = (a, da) if same else pbf.random_set(rng, n_b, int(rng.integers(1, 17)))
        n_b = b[0].shape[1]
        what = f"polygons {n_a} x {n_b}, A {da}, B {'= A' if same else db}"
        pairs = cfz.random_list(rng, n_a, n_b, length)
    desc = f"config {idx}: {what}, list {length} in {cap}, count {n_dev}, bases {rb}, {cb}"
    if announce is not None:
        announce(desc)
    ok, info, wants = plf.run(eng, h.MANIFOLDS, desc, a, b, pairs, cap, n_dev, rb, cb, place)
    LAST.update(plf.hits_and_misses(wants))
    return ok, info


if __name__ == "__main__":
    plf.main("manifold_fuzz", one, "manifolds")
