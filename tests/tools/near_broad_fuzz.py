#!/usr/bin/env python3
"""Differential fuzz of c2d_poly_near_broad_pairs against its reference (tests/near_broad_ref.py: every pair through
tests/distance_ref.py's poly_distances, pinned by tests/test_near_broad_ref_cpu.py): the random sets of poly_broad_fuzz.py (sizes on
both sides of the wave, block and tile edges, row layouts, vertex-count ranges with points and segments, densities, clockwise
polygons, outliers, huge coordinates, NaN / inf in real slots, junk in the padded slots), now and then a vertex count out of range,
strides and pointer offsets, d_k == NULL, two sets, one set against itself (the same memory), C2D_CROSS_UPPER, and a margin per
configuration: 0, -0, the smallest subnormal, a thousandth, a thirtieth, a third of and three times a polygon's size, a hundred
sizes.  draw() makes a configuration and its reference list without a GPU; one() runs it; the judge is pair_search_harness.compare.
Prints its seed; a mismatch names its configuration.
usage: near_broad_fuzz.py [configs] [seed]"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (TESTS, os.path.dirname(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)
import near_broad_ref as ref  # noqa: E402
import pair_search_harness as psh  # noqa: E402


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


poly_broad_fuzz = _tool("poly_broad_fuzz")    # its random sets

LAST = {}   # of the last configuration: "listed" pairs, "apart" = those that are not hit, "misses" = the other pairs
SIZES = [1, 2, 63, 64, 65, 257]
SMALL = 300
MARGINS = [("0", 0.0), ("-0", -0.0), ("denormal", 1e-45), ("size / 1000", 1e-3), ("size / 30", 1 / 30), ("size / 3", 1 / 3), ("3 sizes", 3.0), ("100 sizes", 100.0)]


def _size(s):
    """the median width of the set's polygons over their live, finite vertices"""
    k = np.clip(ref.cref._counts(s), 1, s[0].shape[0])
    live = np.arange(s[0].shape[0])[:, None] < k[None, :]
    with np.errstate(all="ignore"):
        ok = live & np.isfinite(s[0])
        w = np.where(ok, s[0].astype(np.float64), -np.inf).max(0) - np.where(ok, s[0].astype(np.float64), np.inf).min(0)
    w = w[np.isfinite(w) & (w > 0)]
    return float(np.median(w)) if w.size else 1.0


def draw(rng, idx, small=False):
    """One configuration and the reference's list of it, no GPU involved -> a dict of what one() needs (small: no set above SMALL)"""
    sizes = SIZES + [int(rng.integers(1, 1200)), int(rng.integers(1200, 2600))]
    if small:
        sizes = [min(n, SMALL) for n in sizes]
    n_a, n_b = int(rng.choice(sizes)), int(rng.choice(sizes))
    mode = str(rng.choice(["two", "two", "self"]))
    upper = bool(rng.random() < 0.5)
    a, da = poly_broad_fuzz.random_set(rng, n_a, int(rng.integers(1, 17)))
    b, db = poly_broad_fuzz.random_set(rng, n_b, int(rng.integers(1, 17))) if mode == "two" else (a, da)
    name, rel = MARGINS[int(rng.integers(0, len(MARGINS)))]
    with np.errstate(all="ignore"):
        max_dist = float(np.float32(rel if rel in (0.0, 1e-45) else min(rel * _size(a), 2.0 ** 59)))
    # The reference walks every candidate of every pair it cannot drop: where most pairs are listed (a margin of many sizes, the densest
    # scenes) the sets stay small.
    crowded = rel >= 3.0 or "density 16.0" in da + db
    if crowded and max(n_a, n_b) > SMALL:
        cut = lambda s, n: (s[0][:, :n], s[1][:, :n], s[2][:n])   # noqa: E731
        a = cut(a, min(n_a, SMALL))
        b = a if mode != "two" else cut(b, min(n_b, SMALL))
    n_a, n_b = a[0].shape[1], b[0].shape[1]
    no_k = bool(rng.random() < 0.15)
    if no_k:                                                   # d_k == NULL: every polygon has `rows` vertices, and they are all read
        a = (np.nan_to_num(a[0], nan=1.0, posinf=2.0, neginf=-2.0), np.nan_to_num(a[1], nan=1.0, posinf=2.0, neginf=-2.0), None)
    elif rng.random() < 0.3:                                   # a few vertex counts out of range
        k = a[2].copy()
        k[rng.integers(0, n_a, 1 + n_a // 50)] = rng.choice(np.array([0, a[0].shape[0] + 1, 255], np.uint8), 1 + n_a // 50)
        a = (a[0], a[1], k)
    if mode != "two":
        b = a
    what = f"near broad config {idx}: " + (f"{n_a} x {n_b}, A {da}, B {db}" if mode == "two" else f"{mode} n {n_a} {da}")
    what += f", margin {name} = {max_dist!r}, upper {upper}" + (", no count plane" if no_k else "")
    with np.errstate(all="ignore"):
        want = ref.pairs(a, b, max_dist, upper=upper)
        ii, jj = want[:, 0].astype(np.int64), want[:, 1].astype(np.int64)
        hit = int((ref.records(a, b, ii, jj)["hit"] == 1).sum()) if len(want) else 0
    both = ref.present(a)[:, None] & ref.present(b)[None, :]
    considered = int(np.triu(both, 1).sum()) if upper else int(both.sum())
    LAST.update(listed=len(want), apart=len(want) - hit, misses=considered - len(want))
    place = [(int(rng.integers(0, 4)), int(rng.integers(0, 9))) for _ in range(2)]
    return dict(a=a, b=b, max_dist=max_dist, mode=mode, upper=upper, no_k=no_k, what=what, want=want, place=place,
                bad=bool((~ref.present(a)).any() or (~ref.present(b)).any()))


def one(eng, rng, idx, announce=None):
    """One configuration -> (ok, description); a vertex count out of range must be reported by the synchronise.
    `announce(text)` is called with the description before any GPU work."""
    c = draw(rng, idx)
    what = c["what"]
    if announce is not None:
        announce(what)
    a, b, place = c["a"], c["b"], c["place"]
    A = psh.DeviceSet(eng, a, offset=place[0][0], stride=a[0].shape[1] + place[0][1])
    B = psh.DeviceSet(eng, b, offset=place[1][0], stride=b[0].shape[1] + place[1][1]) if c["mode"] == "two" else A
    try:
        got, total = psh.run(eng, psh.near_broad(eng, A, B, c["max_dist"], c["upper"]), absent=c["bad"])     # (a vertex count out of range must be reported, by each call)
    finally:
        A.free()
        if B is not A:
            B.free()
    why = psh.compare(got, total, c["want"])
    if why is not None:
        return False, what + ": " + why
    return True, what + f" [{LAST['listed']} pairs, {LAST['apart']} of them apart, {LAST['misses']} misses]"


def main():
    from __graft_entry__ import load_package

    pkg = load_package()
    configs = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else int.from_bytes(os.urandom(4), "little")
    print(f"near_broad_fuzz: seed {seed}, {configs} configurations", flush=True)
    eng = pkg.Engine(0)
    bad = 0
    for idx in range(configs):
        ok, what = one(eng, np.random.default_rng([seed, idx]), idx)
        print(("ok   " if ok else "FAIL ") + what, flush=True)
        bad += not ok
    eng.close()
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
