#!/usr/bin/env python3
"""Differential fuzz of c2d_sat_poly_cross_mask / c2d_sat_poly_cross_pairs against the CPU oracle on the materialised, padded pairs
(the non-GPU branch of reference() of tests/test_gpu_sat_poly_cross.py, never another GPU path): poly_broad_fuzz.py's random sets
per side (rows 1 .. 16, stride, pointer offset, clockwise polygons, points and segments, junk in the padded slots, non-finite real
vertices), one configuration in four packed until everything overlaps (a wave's undecided count crosses 16, 32 and 48), d_k == NULL
when every count equals `rows`, one configuration in five with a vertex count out of range (those rows / columns read 0, are not
counted, and each call reports the error once), A and B the same memory, and cross_fuzz.py's call shapes and judge.  Prints its seed;
a mismatch names its configuration.
usage: poly_cross_fuzz.py [configs] [seed]     (no seed: the commit's, tests/tools/fuzz_seed.py)"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cf = _tool("cross_fuzz")            # the call shapes and the judge
pbf = _tool("poly_broad_fuzz")      # its random sets and its upload
compare = cf.compare
LAST = {}
LIMIT = 1 << 18                     # pairs per configuration: the materialised reference stays below about 70 MB


def pack(s):
    """every ordinary polygon moved nine tenths of the way to the origin: everything overlaps"""
    vx, vy, k = s
    rows = vx.shape[0]
    real = np.arange(rows)[:, None] < k[None, :]
    with np.errstate(all="ignore"):
        for v in (vx, vy):
            shift = np.where(np.isfinite(v[0]) & (np.abs(v[0]) < 1e6), v[0] * np.float32(0.9), np.float32(0))
            v[real] = (v - shift[None, :])[real]
    return s


def padded(s, rows):
    vx, vy, _ = s
    ox, oy = np.zeros((rows, vx.shape[1]), np.float32), np.zeros((rows, vx.shape[1]), np.float32)
    ox[:vx.shape[0]], oy[:vx.shape[0]] = vx, vy
    return ox, oy


def reference(oracle, a, b, ka, kb):
    """bool [n_a][n_b]: the oracle on the materialised pairs (A_i, B_j), both sets padded to the larger `rows`; ka, kb: valid counts"""
    rows = max(a[0].shape[0], b[0].shape[0])
    (ax, ay), (bx, by) = padded(a, rows), padded(b, rows)
    n_a, n_b = ax.shape[1], bx.shape[1]
    vx = np.stack([np.repeat(ax, n_b, axis=1), np.tile(bx, n_a)])
    vy = np.stack([np.repeat(ay, n_b, axis=1), np.tile(by, n_a)])
    res, _ = oracle.sat_poly_pairs(vx, vy, np.stack([np.repeat(ka, n_b), np.tile(kb, n_a)]))
    return res.reshape(n_a, n_b).astype(bool)


def one(eng, rng, idx, announce=None, oracle=None):
    """One configuration; `announce(text)` is called with its description BEFORE any GPU work.  Returns (ok, (description, results))."""
    if oracle is None:
        from oracle import cpu as oracle
    n_a, n_b = cf.draw_sizes(rng, LIMIT)
    same = bool(rng.random() < 1 / 3)
    packed = bool(rng.random() < 0.25)
    if same:
        n_a = n_b = min(n_a, 1 << 9)
    a, da = pbf.random_set(rng, n_a, int(rng.integers(1, 17)))
    b, db = (a, "= A (the same memory)") if same else pbf.random_set(rng, n_b, int(rng.integers(1, 17)))
    if packed:
        pack(a)
        if not same:
            pack(b)
    # a vertex count out of range, in A, in B or in both: the reference comes from the valid counts (the oracle refuses others)
    ka, kb = a[2].copy(), b[2].copy()
    bad = str(rng.choice(["A", "B", "both"])) if rng.random() < 0.2 else "none"
    bad_a, bad_b = np.zeros(n_a, bool), np.zeros(n_b, bool)
    if bad in ("A", "both") or (same and bad != "none"):
        q = rng.integers(0, n_a, int(rng.integers(1, 4)))
        bad_a[q] = True
        a[2][q] = rng.choice(np.array([0, a[0].shape[0] + 1, 255], np.uint8), len(q))
    if same:
        bad_b = bad_a
    elif bad in ("B", "both"):
        q = rng.integers(0, n_b, int(rng.integers(1, 4)))
        bad_b[q] = True
        b[2][q] = rng.choice(np.array([0, b[0].shape[0] + 1, 255], np.uint8), len(q))
    no_k = [bool(not bad_x.any() and (s[2] == s[0].shape[0]).all()) for s, bad_x in ((a, bad_a), (b, bad_b))]
    call = cf.draw_call(rng, n_a, n_b)
    place = [(int(rng.integers(0, 4)), n + int(rng.integers(0, 9))) for n in (n_a, n_b)]
    ref = reference(oracle, a, b, ka, kb)
    ref[bad_a] = False
    ref[:, bad_b] = False
    want = cf.expected(ref, call["upper"], call["rb"], call["cb"])
    total = int(want.sum())
    cap = cf.capacity_of(call["cap_kind"], total)
    real = [(np.arange(s[0].shape[0])[:, None] < np.minimum(kk, s[0].shape[0])[None, :]) for s, kk in ((a, ka), (b, kb))]
    finite = all(np.isfinite(s[0][r]).all() and np.isfinite(s[1][r]).all() for s, r in zip((a, b), real))
    desc = (f"config {idx}: {n_a} x {n_b} polygons, A {da}, B {db}, {'packed, ' if packed else ''}{'finite' if finite else 'non-finite real vertices'}, bad count in {bad}, "
            f"d_k {'NULL' if no_k[0] else 'given'} / {'NULL' if no_k[1] else 'given'}, (offset, stride) {place[0]} / {place[0] if same else place[1]}, "
            f"{cf.describe_call(call, n_b, total, cap)}")
    if announce is not None:
        announce(desc)
    sa, keep = pbf.upload(eng, a, *place[0])
    if no_k[0]:
        sa = eng.poly_set(sa.d_vx, sa.d_vy, None, n_a, sa.rows, sa.stride)
    if same:
        sb, keep_b = sa, ()
    else:
        sb, keep_b = pbf.upload(eng, b, *place[1])
        if no_k[1]:
            sb = eng.poly_set(sb.d_vx, sb.d_vy, None, n_b, sb.rows, sb.stride)
    kw = dict(row_base=call["rb"], col_base=call["cb"], upper=call["upper"])
    try:
        got = cf.run_call(eng, lambda m, ld, c: eng.sat_poly_cross_mask(sa, sb, m, ld_words=ld, count=c, **kw),
                          lambda p, capacity, c: eng.sat_poly_cross_pairs(sa, sb, p, capacity, c, **kw), n_a, call, cap)
    finally:
        for x in list(keep) + list(keep_b):
            x.free()
    tested = cf.expected(np.ones((n_a, n_b), bool), call["upper"], call["rb"], call["cb"])
    in_a_tested_pair = bool(tested[bad_a].any() or tested[:, bad_b].any())
    complaints = compare(*got, want, n_b, call["rb"], call["cb"], cap, expect_report=True if in_a_tested_pair else (False if bad == "none" else None))
    LAST.update(hits=total, misses=want.size - total)
    if complaints:
        print(f"MISMATCH {desc}: " + "; ".join(complaints))
    return not complaints, (desc, n_a * n_b)


if __name__ == "__main__":
    cf.main("poly_cross_fuzz", one)
