#!/usr/bin/env python3
"""Differential fuzz of c2d_poly_pair_overlaps / c2d_rect_pair_overlaps against the CPU restatement of their contract
(tests/overlap_ref.py, pinned by tests/test_overlap_ref_cpu.py), after distance_fuzz.py and with its random sets: random set sizes,
row layouts, vertex-count ranges, densities, strides and pointer offsets, bases, list lengths and device counts, clockwise polygons,
points and segments, outliers, NaN / inf in real slots, junk in the padded slots, tied shapes; rectangles as random quads, one time in
three on a 1/16 grid (shared sides and corners, exact ties), some with non-finite vertices.  This file is the generator; the call and
the judge are pair_list_fuzz.py's, on the row of tests/overlap_query.py.  Prints its seed; a mismatch names its configuration.
usage: overlap_fuzz.py [configs] [seed]     (no seed: the commit's, tests/tools/fuzz_seed.py)"""
import importlib.util
import os

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("pair_list_fuzz", os.path.join(HERE, "pair_list_fuzz.py"))
plf = importlib.util.module_from_spec(spec)
spec.loader.exec_module(plf)            # the back half of every list-driven fuzz tool: run(), its judge, main(); it puts tests/ on the path
from overlap_query import OVERLAPS  # noqa: E402

distance_fuzz = plf.tool("distance_fuzz")    # its random sets
contact_fuzz = plf.tool("contact_fuzz")      # its random list

LAST = {}   # hits / misses of the last configuration, for the exploring leg's "not vacuous" check


def one(eng, rng, idx, announce=None):
    """One configuration; `announce(text)` is called with its description BEFORE any GPU work.  Returns (ok, (description, records))."""
    n_a, n_b = (int(rng.choice([1, 2, 63, 64, 65, 257, int(rng.integers(1, 600))])) for _ in range(2))
    length = int(rng.choice([1, 63, 64, 65, 257, int(rng.integers(1, 5000))]))
    rb, cb = (int(rng.choice([0, 0, 7, 1 << 20, (1 << 32) - 700])) for _ in range(2))
    cap = length + int(rng.choice([0, 0, 1, 100]))
    n_dev = rng.choice([None, length, max(length - 1, 0), length // 2, cap + 5])
    a, b, place, what = distance_fuzz.random_sets(rng, n_a, n_b)
    desc = f"config {idx}: {what}, list {length} in {cap}, count {n_dev}, bases {rb}, {cb}"
    if announce is not None:
        announce(desc)
    pairs = contact_fuzz.random_list(rng, n_a, (b.shape if place is None else b[0].shape)[1], length)
    ok, info, wants = plf.run(eng, OVERLAPS, desc, a, b, pairs, cap, n_dev, rb, cb, place)
    LAST.update(plf.hits_and_misses(wants))
    LAST["areas"] = int((wants[0]["area"] > 0).sum())
    return ok, info


if __name__ == "__main__":
    plf.main("overlap_fuzz", one, "records")
