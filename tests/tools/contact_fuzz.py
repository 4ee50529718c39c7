#!/usr/bin/env python3
"""Differential fuzz of c2d_poly_pair_contacts / c2d_rect_pair_contacts against the CPU restatement of their contract
(tests/contact_ref.py, pinned by tests/test_contact_ref_cpu.py): random set sizes, row layouts, vertex-count ranges, densities,
strides and pointer offsets, bases, list lengths and device counts, clockwise polygons, points and segments, outliers, NaN / inf
in real slots, junk in the padded slots, tied shapes; and, one configuration in five, a few hundred near-tied pairs (polygons or
quads whose two best axes are not parallel and 2^-28 .. 2^-10 apart, tests/contact_cases.py) at a power-of-two scale of 2^-52 .. 2^52,
where the kernel's first pass has to tell a decided axis from one too close to call.  This file is the generator; the call and the
judge are pair_list_fuzz.py's.  Prints its seed; a mismatch names its configuration.
usage: contact_fuzz.py [configs] [seed]     (no seed: the commit's, tests/tools/fuzz_seed.py)"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("pair_list_fuzz", os.path.join(HERE, "pair_list_fuzz.py"))
plf = importlib.util.module_from_spec(spec)
spec.loader.exec_module(plf)            # the back half of every list-driven fuzz tool: run(), its judge, main(); it puts tests/ on the path
h, pkg, wl, pbf, fuzz_seed = plf.h, plf.pkg, plf.wl, plf.pbf, plf.fuzz_seed
import contact_cases as cases  # noqa: E402

LAST = {}   # hits / misses of the last configuration, for the exploring leg's "not vacuous" check


def random_list(rng, n_a, n_b, length):
    """row-major, as a list call emits it, with a few entries out of their set"""
    flat = np.sort(rng.integers(0, n_a * n_b, length))
    pairs = np.stack([flat // n_b, flat % n_b], axis=1).astype(np.int64)
    for q in np.flatnonzero(rng.random(length) < 0.01):
        pairs[q, int(rng.integers(0, 2))] = rng.choice([-1, n_a, n_b, max(n_a, n_b) + 5])
    return pairs


def one(eng, rng, idx, announce=None):
    """One configuration; `announce(text)` is called with its description BEFORE any GPU work.  Returns (ok, (description, pairs))."""
    n_a, n_b = (int(rng.choice([1, 2, 63, 64, 65, 257, int(rng.integers(1, 600))])) for _ in range(2))
    length = int(rng.choice([1, 63, 64, 65, 257, int(rng.integers(1, 5000))]))
    near_tie = bool(rng.random() < 0.2)
    if near_tie:
        n_a = n_b = length = int(rng.integers(200, 600))
    rb, cb = (int(rng.choice([0, 0, 7, 1 << 20, (1 << 32) - 700])) for _ in range(2))
    cap = length + int(rng.choice([0, 0, 1, 100]))
    n_dev = rng.choice([None, length, max(length - 1, 0), length // 2, cap + 5])
    rects = bool(rng.random() < (0.5 if near_tie else 0.3))
    place = None
    draw_place = lambda: (int(rng.integers(0, 4)), int(rng.integers(0, 9)))  # noqa: E731   (offset, stride - n) of a polygon set's planes
    if near_tie:
        lo = float(rng.uniform(-28.0, -20.0))
        g_log2, k, seed = (lo, lo + float(rng.uniform(2.0, 10.0))), int(rng.integers(-52, 53)), int(rng.integers(1 << 30))
        what = (f"near-ties, {'quads' if rects else 'polygons'} {n_a} x {n_b} (generator seed {seed}, |g| in 2^{g_log2[0]:.1f} .. 2^{g_log2[1]:.1f}, "
                f"scale 2^{k})")
        if rects:
            a, b = (np.ldexp(x, k).astype(np.float32) for x in cases.near_tie_quad_sets(n_a, seed, g_log2))
        else:
            a, b = (cases.scaled_poly_set(x, k) for x in cases.near_tie_poly_sets(n_a, seed, g_log2))
            place = [draw_place(), draw_place()]
    elif rects:
        a = (rng.uniform(-3, 3, (1, n_a)) + rng.uniform(-2, 2, (8, n_a))).astype(np.float32)
        b = a if (n_a == n_b and rng.random() < 0.3) else (rng.uniform(-3, 3, (1, n_b)) + rng.uniform(-2, 2, (8, n_b))).astype(np.float32)
        if rng.random() < 0.3:
            a = wl.inject_non_finite(a, seed=int(rng.integers(1 << 30)), frac=0.1)
        what = f"rectangles {n_a} x {n_b}"
    else:
        a, da = pbf.random_set(rng, n_a, int(rng.integers(1, 17)))
        same = bool(rng.random() < 0.3)
        b, db = (a, da) if same else pbf.random_set(rng, n_b, int(rng.integers(1, 17)))
        n_b = b[0].shape[1]
        place = [draw_place()] + ([] if same else [draw_place()])
        what = f"polygons {n_a} x {n_b}, A {da}, B {'= A' if same else db}"
    desc = f"config {idx}: {what}, list {length} in {cap}, count {n_dev}, bases {rb}, {cb}"
    if announce is not None:
        announce(desc)
    if near_tie:      # pair (A_i, B_i) is the near-tie: the diagonal in a shuffled order (rows change inside a wave)
        order = rng.permutation(n_a)
        pairs = np.stack([order, order], axis=1).astype(np.int64)
    else:
        pairs = random_list(rng, n_a, n_b, length)
    ok, info, wants = plf.run(eng, h.CONTACTS, desc, a, b, pairs, cap, n_dev, rb, cb, place)
    LAST.update(plf.hits_and_misses(wants))
    return ok, info


if __name__ == "__main__":
    plf.main("contact_fuzz", one, "contacts")
