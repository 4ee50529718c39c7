#!/usr/bin/env python3
"""Differential fuzz of c2d_poly_pair_contacts / c2d_rect_pair_contacts against the CPU restatement of their contract
(tests/contact_ref.py, pinned by tests/test_contact_ref_cpu.py): random set sizes, row layouts, vertex-count ranges, densities,
strides and pointer offsets, bases, list lengths and device counts, clockwise polygons, points and segments, outliers, NaN / inf
in real slots, junk in the padded slots, tied shapes; and, one configuration in five, a few hundred near-tied pairs (polygons or
quads whose two best axes are not parallel and 2^-28 .. 2^-10 apart, tests/contact_cases.py) at a power-of-two scale of 2^-52 .. 2^52,
where the kernel's first pass has to tell a decided axis from one too close to call.  Prints its seed; a mismatch names its
configuration.
usage: contact_fuzz.py [configs] [seed]     (no seed: the commit's, tests/tools/fuzz_seed.py)"""
import importlib
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from __graft_entry__ import load_package  # noqa: E402
import contact_cases as cases  # noqa: E402
import contact_ref as ref  # noqa: E402

pkg = load_package()
wl = importlib.import_module("c2d_amd.workloads")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


pbf = _tool("poly_broad_fuzz")      # its random sets and its upload
fuzz_seed = _tool("fuzz_seed")


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
    if near_tie:
        lo = float(rng.uniform(-28.0, -20.0))
        g_log2, k, seed = (lo, lo + float(rng.uniform(2.0, 10.0))), int(rng.integers(-52, 53)), int(rng.integers(1 << 30))
        desc = (f"config {idx}: near-ties, {'quads' if rects else 'polygons'} {n_a} x {n_b} (generator seed {seed}, |g| in 2^{g_log2[0]:.1f} .. 2^{g_log2[1]:.1f}, "
                f"scale 2^{k}), list {length} in {cap}, count {n_dev}, bases {rb}, {cb}")
        if rects:
            a, b = (np.ldexp(x, k).astype(np.float32) for x in cases.near_tie_quad_sets(n_a, seed, g_log2))
            keep = [eng.to_device(a), eng.to_device(b)]
            pa, pb = [keep[0].row(q) for q in range(8)], [keep[1].row(q) for q in range(8)]
        else:
            a, b = (cases.scaled_poly_set(x, k) for x in cases.near_tie_poly_sets(n_a, seed, g_log2))
            sa, keep = pbf.upload(eng, a, int(rng.integers(0, 4)), n_a + int(rng.integers(0, 9)))
            sb, keep_b = pbf.upload(eng, b, int(rng.integers(0, 4)), n_b + int(rng.integers(0, 9)))
            keep = list(keep) + list(keep_b)
    elif rects:
        a = (rng.uniform(-3, 3, (1, n_a)) + rng.uniform(-2, 2, (8, n_a))).astype(np.float32)
        b = a if (n_a == n_b and rng.random() < 0.3) else (rng.uniform(-3, 3, (1, n_b)) + rng.uniform(-2, 2, (8, n_b))).astype(np.float32)
        if rng.random() < 0.3:
            a = wl.inject_non_finite(a, seed=int(rng.integers(1 << 30)), frac=0.1)
        desc = f"config {idx}: rectangles {n_a} x {n_b}, list {length} in {cap}, count {n_dev}, bases {rb}, {cb}"
        keep = [eng.to_device(a), eng.to_device(b)]
        pa, pb = [keep[0].row(k) for k in range(8)], [keep[1].row(k) for k in range(8)]
    else:
        a, da = pbf.random_set(rng, n_a, int(rng.integers(1, 17)))
        same = bool(rng.random() < 0.3)
        b, db = (a, da) if same else pbf.random_set(rng, n_b, int(rng.integers(1, 17)))
        n_b = b[0].shape[1]
        sa, keep = pbf.upload(eng, a, int(rng.integers(0, 4)), n_a + int(rng.integers(0, 9)))
        sb, keep_b = (sa, ()) if same else pbf.upload(eng, b, int(rng.integers(0, 4)), n_b + int(rng.integers(0, 9)))
        keep = list(keep) + list(keep_b)
        desc = f"config {idx}: polygons {n_a} x {n_b}, A {da}, B {'= A' if same else db}, list {length} in {cap}, count {n_dev}, bases {rb}, {cb}"
    if announce is not None:
        announce(desc)
    if near_tie:      # pair (A_i, B_i) is the near-tie: the diagonal in a shuffled order (rows change inside a wave)
        order = rng.permutation(n_a)
        pairs = np.stack([order, order], axis=1).astype(np.int64)
    else:
        pairs = random_list(rng, n_a, n_b, length)
    listed = np.full((cap, 2), 0xFFFFFFFF, np.uint32)
    listed[:length] = ((pairs + (rb, cb)) & 0xFFFFFFFF).astype(np.uint32)
    # what the call sees is the u32 list minus the bases: an entry that wrapped is judged as the call judges it
    li, lj = listed[:, 0].astype(np.int64) - rb, listed[:, 1].astype(np.int64) - cb
    bound = cap if n_dev is None else min(cap, int(n_dev))
    want = (ref.rect_contacts(a, b, li[:bound], lj[:bound]) if rects else ref.poly_contacts(a, b, li[:bound], lj[:bound]))
    d_pairs = eng.to_device(listed)
    d_out = eng.empty(cap + 2, ref.CONTACT_DT)
    eng.memset(d_out, 0xA5, d_out.nbytes)
    d_n = None if n_dev is None else eng.to_device(np.array([int(n_dev)], np.uint64))
    if rects:
        eng.rect_pair_contacts(pa, n_a, pb, n_b, d_pairs, cap, d_out.ptr + 16, n_pairs_dev=d_n, row_base=rb, col_base=cb)
    else:
        eng.poly_pair_contacts(sa, sb, d_pairs, cap, d_out.ptr + 16, n_pairs_dev=d_n, row_base=rb, col_base=cb)
    try:
        eng.synchronize()
        reported = False
    except pkg.C2DError:
        reported = True
    raw = d_out.get()
    for x in keep + [d_pairs, d_out] + ([d_n] if d_n is not None else []):
        x.free()
    got = raw[1:1 + bound]
    untouched = (np.delete(raw.view(np.uint8).reshape(-1, 16), np.arange(1, 1 + bound), axis=0) == 0xA5).all()
    ok = bool(ref.same(got, want).all()) and bool(untouched) and reported == bool((want["flags"] & ref.BAD_PAIR).any())
    LAST.update(hits=int((want["hit"] != 0).sum()), misses=int((want["hit"] == 0).sum()))
    if not ok:
        print(f"MISMATCH {desc}: {int((~ref.same(got, want)).sum())} contacts differ, untouched {bool(untouched)}, error reported {reported}")
    return ok, (desc, bound)


def main():
    configs = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed, origin = (int(sys.argv[2]), "the command line") if len(sys.argv) > 2 else fuzz_seed.commit_seed()
    print(f"contact_fuzz: {configs} configurations, seed {seed} ({origin})", flush=True)
    rng = np.random.default_rng(seed)
    eng = pkg.Engine(0)
    fails = total = 0
    for i in range(configs):
        ok, info = one(eng, rng, i)
        fails += not ok
        total += info[-1]
        if (i + 1) % 50 == 0:
            print(f"  {i + 1} / {configs} configurations, {fails} failures so far", flush=True)
    print(f"{configs} configurations, {fails} failures; {total} contacts compared")
    eng.close()
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    main()
