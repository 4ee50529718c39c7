#!/usr/bin/env python3
"""Differential fuzz of c2d_poly_pair_manifolds against the CPU restatement of its contract (tests/manifold_ref.py, pinned by
tests/test_manifold_ref_cpu.py) under the equality tests/pair_list_harness.py's MANIFOLDS entry uses, on contact_fuzz.py's polygon
configurations: its random sets (sizes, row layouts, strides and pointer offsets, clockwise polygons, points and segments, outliers,
NaN / inf, junk in the padded slots, the same memory on both sides), its lists (row-major, a few entries out of their set), bases,
capacities and device counts, and one configuration in five its near-tied polygons at a power-of-two scale.  compare() is the judge
(a pure function on host arrays, tests/test_fuzz_compare_cpu.py): both outputs record by record, the guard bands around both
buffers, every record at or beyond min(n_pairs, *d_n_pairs) untouched, a bad entry reported once.  Prints its seed; a mismatch names
its configuration.
usage: manifold_fuzz.py [configs] [seed]     (no seed: the commit's, tests/tools/fuzz_seed.py)"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cfz = _tool("contact_fuzz")         # its generators: random_list, and through it poly_broad_fuzz's sets and contact_cases' near-ties
import contact_ref  # noqa: E402
import manifold_ref as ref  # noqa: E402

pkg, pbf, cases, fuzz_seed = cfz.pkg, cfz.pbf, cfz.cases, cfz.fuzz_seed
GUARD, BAND = 4, 0xA5
DTS = (contact_ref.CONTACT_DT, ref.MANIFOLD_DT)
SAMES = (contact_ref.same, ref.same)
LAST = {}


def compare(contacts, manifolds, reported, clean, want_contacts, want_manifolds, capacity):
    """contacts CONTACT_DT [GUARD + capacity + GUARD], manifolds MANIFOLD_DT likewise, as the call left buffers of BAND bytes;
    reported: the synchronisation raised; clean: check_async afterwards was; want_*: the reference's records of the first
    min(n_pairs, *d_n_pairs) entries -> the list of complaints"""
    out = []
    bound = len(want_contacts)
    for got, want, same, dt, noun in zip((contacts, manifolds), (want_contacts, want_manifolds), SAMES, DTS, ("contacts", "manifolds")):
        if got.dtype != dt or got.shape != (capacity + 2 * GUARD,) or len(want) != bound or bound > capacity:
            out.append(f"{noun}: a buffer of {got.shape} {got.dtype} for a capacity of {capacity} and {len(want)} expected records")
            continue
        raw = got.view(np.uint8).reshape(-1, dt.itemsize)
        if not ((raw[:GUARD] == BAND).all() and (raw[GUARD + capacity:] == BAND).all()):
            out.append(f"{noun}: written outside the output")
        if not (raw[GUARD + bound: GUARD + capacity] == BAND).all():
            out.append(f"{noun}: written at or beyond min(n_pairs, *d_n_pairs)")
        records = got[GUARD: GUARD + bound]
        ok = same(records, want)
        if "reserved" in dt.names:
            ok &= records["reserved"] == 0
        if not ok.all():
            q = int(np.flatnonzero(~ok)[0])
            out.append(f"{int((~ok).sum())} of {bound} {noun} differ; first at {q}: got {records[q]}, want {want[q]}")
    expect = bool((want_contacts["flags"] & contact_ref.BAD_PAIR).any())
    if bool(reported) != expect:
        out.append(f"error reported: {bool(reported)}, the list {'has' if expect else 'has no'} bad entry")
    if not clean:
        out.append("check_async still reports an error after the synchronisation")
    return out


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
    same = False
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
    listed = np.full((cap, 2), 0xFFFFFFFF, np.uint32)
    listed[:length] = ((pairs + (rb, cb)) & 0xFFFFFFFF).astype(np.uint32)
    # what the call sees is the u32 list minus the bases: an entry that wrapped is judged as the call judges it
    li, lj = listed[:, 0].astype(np.int64) - rb, listed[:, 1].astype(np.int64) - cb
    bound = cap if n_dev is None else min(cap, int(n_dev))
    want = ref.poly_manifolds(a, b, li[:bound], lj[:bound])
    sa, keep = pbf.upload(eng, a, place[0][0], n_a + place[0][1])
    sb, keep_b = (sa, ()) if same else pbf.upload(eng, b, place[1][0], n_b + place[1][1])
    keep = list(keep) + list(keep_b) + [eng.to_device(listed)]
    d_pairs = keep[-1]
    d_outs = [eng.empty(cap + 2 * GUARD, dt) for dt in DTS]
    d_n = None if n_dev is None else eng.to_device(np.array([int(n_dev)], np.uint64))
    try:
        for d in d_outs:
            eng.memset(d, BAND, d.nbytes)
        eng.poly_pair_manifolds(sa, sb, d_pairs, cap, *[d.ptr + GUARD * dt.itemsize for d, dt in zip(d_outs, DTS)], n_pairs_dev=d_n,
                                row_base=rb, col_base=cb)
        try:
            eng.synchronize()
            reported = False
        except pkg.C2DError:
            reported = True
        try:
            eng.check_async()
            clean = True
        except pkg.C2DError:
            clean = False
        got = [d.get() for d in d_outs]
    finally:
        for x in keep + d_outs + ([d_n] if d_n is not None else []):
            x.free()
    complaints = compare(got[0], got[1], reported, clean, want[0], want[1], cap)
    LAST.update(hits=int((want[0]["hit"] != 0).sum()), misses=int((want[0]["hit"] == 0).sum()))
    if complaints:
        print(f"MISMATCH {desc}: " + "; ".join(complaints))
    return not complaints, (desc, bound)


def main():
    configs = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed, origin = (int(sys.argv[2]), "the command line") if len(sys.argv) > 2 else fuzz_seed.commit_seed()
    print(f"manifold_fuzz: {configs} configurations, seed {seed} ({origin})", flush=True)
    eng = pkg.Engine(0)
    fails = total = 0
    for i in range(configs):
        ok, info = one(eng, np.random.default_rng([seed, i]), i)
        fails += not ok
        total += info[-1]
        if (i + 1) % 50 == 0:
            print(f"  {i + 1} / {configs} configurations, {fails} failures so far", flush=True)
    print(f"{configs} configurations, {fails} failures; {total} manifolds compared")
    eng.close()
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    main()
