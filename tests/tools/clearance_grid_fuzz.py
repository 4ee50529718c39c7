#!/usr/bin/env python3
"""Differential fuzz of c2d_poly_set_clearances_grid against its reference (tests/clearance_grid_ref.py: near_broad_ref's considered
pairs, distance_ref's records of exactly those, a per-row minimum; pinned by tests/test_clearance_grid_ref_cpu.py) on the generators
of near_broad_fuzz.py: the random sets of poly_broad_fuzz.py (sizes on both sides of the wave, block and tile edges, row layouts,
vertex-count ranges with points and segments, densities, clockwise polygons, outliers, huge coordinates, NaN / inf in real slots, junk
in the padded slots), now and then a vertex count out of range, strides and pointer offsets, d_k == NULL, two sets or one set against
itself (the same memory), row and column bases, C2D_CLEARANCE_SKIP_SELF, and a margin per configuration from 0 to several scene
extents.  draw() makes a configuration and the reference's records without a GPU; one() runs it; judge() compares.  Prints its seed; a
mismatch names its configuration.
usage: clearance_grid_fuzz.py [configs] [seed]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (TESTS, os.path.dirname(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)
import best_key_harness as best  # noqa: E402
import clearance_grid_harness as gh  # noqa: E402
import clearance_grid_ref as ref  # noqa: E402
import near_broad_ref as nref  # noqa: E402
import pair_search_harness as psh  # noqa: E402


near_broad_fuzz = best.load_tool("near_broad_fuzz")    # its sizes, its measure of a polygon's size and, through it, poly_broad_fuzz's random sets
poly_broad_fuzz = near_broad_fuzz.poly_broad_fuzz

LAST = {}   # of the last configuration: "winners", "apart" = winners that are not hit, "none" = NONE records, "bad" = BAD_PAIR records
SMALL = 300
NO_POLY = 0xFFFFFFFF
# (name, what it multiplies): sizes of a polygon, or extents of the whole scene
MARGINS = [("0", 0.0, "abs"), ("-0", -0.0, "abs"), ("denormal", 1e-45, "abs"), ("size / 1000", 1e-3, "size"), ("size / 30", 1 / 30, "size"),
           ("size / 3", 1 / 3, "size"), ("1 size", 1.0, "size"), ("3 sizes", 3.0, "size"), ("extent / 10", 0.1, "extent"), ("3 extents", 3.0, "extent")]


def _extent(s):
    """the width of the whole set over its live, finite vertices"""
    with np.errstate(all="ignore"):
        x = s[0][np.isfinite(s[0])].astype(np.float64)
    return float(x.max() - x.min()) if x.size and x.max() > x.min() else 1.0


def draw(rng, idx, small=False):
    """One configuration and the reference's records of it, no GPU involved -> a dict of what one() needs (small: no set above SMALL)"""
    sizes = near_broad_fuzz.SIZES + [int(rng.integers(1, 1200)), int(rng.integers(1200, 2600))]
    if small:
        sizes = [min(n, SMALL) for n in sizes]
    n_a, n_b = int(rng.choice(sizes)), int(rng.choice(sizes + [0]))
    mode = str(rng.choice(["two", "two", "self"]))
    a, da = poly_broad_fuzz.random_set(rng, n_a, int(rng.integers(1, 17)))
    if mode == "two":
        b, db = poly_broad_fuzz.random_set(rng, max(n_b, 1), int(rng.integers(1, 17)))
        b = (b[0][:, :n_b], b[1][:, :n_b], b[2][:n_b])
    else:
        b, db = a, da
    name, rel, unit = MARGINS[int(rng.integers(0, len(MARGINS)))]
    with np.errstate(all="ignore"):
        scale = {"abs": 1.0, "size": near_broad_fuzz._size(a), "extent": _extent(a)}[unit]
        max_dist = float(np.float32(min(rel * scale, 2.0 ** 59))) if unit != "abs" else float(np.float32(rel))
    # The reference walks every candidate of every pair within the margin: where most pairs are (a margin of extents, the densest scenes)
    # the sets stay small.
    crowded = unit == "extent" or rel >= 3.0 or "density 16.0" in da + db
    if crowded and max(n_a, n_b) > SMALL:
        cut = lambda s, n: (s[0][:, :n], s[1][:, :n], s[2][:n])   # noqa: E731
        a = cut(a, min(n_a, SMALL))
        b = a if mode != "two" else cut(b, min(n_b, SMALL))
    n_a, n_b = a[0].shape[1], b[0].shape[1]
    no_k = bool(rng.random() < 0.15)
    if no_k:                                                   # d_k == NULL: every polygon has `rows` vertices, and they are all read
        a = (np.nan_to_num(a[0], nan=1.0, posinf=2.0, neginf=-2.0), np.nan_to_num(a[1], nan=1.0, posinf=2.0, neginf=-2.0), None)
        if mode == "two":
            b = (np.nan_to_num(b[0], nan=1.0, posinf=2.0, neginf=-2.0), np.nan_to_num(b[1], nan=1.0, posinf=2.0, neginf=-2.0), None)
    elif rng.random() < 0.3:                                   # a few vertex counts out of range, in either set
        for s in ("a", "b") if mode == "two" else ("a",):
            x = a if s == "a" else b
            m = x[0].shape[1]
            if m == 0:
                continue
            k = x[2].copy()
            k[rng.integers(0, m, 1 + m // 50)] = rng.choice(np.array([0, x[0].shape[0] + 1, 255], np.uint8), 1 + m // 50)
            if s == "a":
                a = (a[0], a[1], k)
            else:
                b = (b[0], b[1], k)
    if mode != "two":
        b = a
    flags = int(rng.random() < 0.5)
    if mode == "self":
        row_base = col_base = int(rng.choice([0, 0, 7, (1 << 32) - n_a]))
    else:
        row_base, col_base = (int(rng.choice([0, 3, 1000, (1 << 32) - max(n_a, n_b)])) for _ in range(2))
        if flags and rng.random() < 0.7:                       # a shard of B that holds the self pairs: row_base + i == col_base + j somewhere
            col_base = min(row_base + int(rng.integers(-2, 3)) if row_base >= 2 else row_base, (1 << 32) - n_b)
    kw = dict(row_base=row_base, col_base=col_base, flags=flags)
    what = f"clearance grid config {idx}: " + (f"{n_a} x {n_b}, A {da}, B {db}" if mode == "two" else f"{mode} n {n_a} {da}")
    what += f", margin {name} = {max_dist!r}, {kw}" + (", no count plane" if no_k else "")
    with np.errstate(all="ignore"):
        want = ref.clearances(a, b, max_dist, **kw)
    win = want["poly"] != NO_POLY
    LAST.update(winners=int(win.sum()), apart=int((win & (want["hit"] == 0)).sum()), none=int((want["flags"] == ref.NONE_FLAG).sum()),
                bad=int((~win & (want["flags"] != ref.NONE_FLAG)).sum()))
    place = [(int(rng.integers(0, 4)), int(rng.integers(0, 9))) for _ in range(2)]
    return dict(a=a, b=b, max_dist=max_dist, mode=mode, kw=kw, no_k=no_k, what=what, want=want, place=place,
                bad=bool((~nref.present(a)).any() or (n_b and (~nref.present(b)).any())))


def judge(got, want):
    """None when the records `got` equal the reference's, else what differs"""
    if len(got) != len(want):
        return f"{len(got)} records, the reference has {len(want)}"
    ok = ref.same(got, want)
    if ok.all():
        return None
    q = int(np.flatnonzero(~ok)[0])
    fields = [f for f in want.dtype.names if got[f][q].tobytes() != want[f][q].tobytes()]
    return f"{int((~ok).sum())} of {len(want)} records differ; first at query {q} in {fields}: got {got[q]}, want {want[q]}"


def one(eng, rng, idx, announce=None):
    """One configuration -> (ok, description); a vertex count out of range must be reported by the synchronise.
    `announce(text)` is called with the description before any GPU work."""
    c = draw(rng, idx)
    what = c["what"]
    if announce is not None:
        announce(what)
    a, b, place = c["a"], c["b"], c["place"]
    n_a, n_b = a[0].shape[1], b[0].shape[1]
    A = psh.DeviceSet(eng, a, offset=place[0][0], stride=n_a + place[0][1])
    B = psh.DeviceSet(eng, b, offset=place[1][0], stride=n_b + place[1][1]) if c["mode"] == "two" and n_b else A
    b_set = B.set if n_b else eng.poly_set(A.px, A.py, None, 0, b[0].shape[0], 0)      # an empty B: only its `rows` is looked at
    try:
        got = gh.call(eng, A.set, b_set, n_a, c["max_dist"], expect_error=c["bad"], **c["kw"])
    finally:
        A.free()
        if B is not A:
            B.free()
    why = judge(got, c["want"])
    if why is not None:
        return False, what + ": " + why
    return True, what + f" [{LAST['winners']} winners, {LAST['apart']} of them apart, {LAST['none']} none, {LAST['bad']} bad queries]"


if __name__ == "__main__":
    best.fuzz_main("clearance_grid_fuzz", one, needs_wl=False)
