#!/usr/bin/env python3
"""Differential fuzz of c2d_poly_set_clearances against the CPU restatement of its contract (tests/clearance_ref.py, pinned by
tests/test_clearance_ref_cpu.py): random set sizes on both sides of the kernel's tiles, row layouts, vertex-count ranges, densities
from crowded to sparse (where the certified skip fires), repeated polygons (ties between obstacles), scales inside and outside the
bound's domain and in the band where d2 underflows to 0 while the exact test still separates (a hit and a separated pair then tie), NaN / inf in real slots, vertex counts out of range in both sets, strides and pointer offsets, bases, d_k == NULL,
one set against itself under C2D_CLEARANCE_SKIP_SELF, and (about one configuration in seven, two sets only) so many queries that the
launch lies between one strip and one strip per column tile: several tiles per strip, split unevenly, with many row tiles.  The
reference is computed for the distinct polygons and indexed, so a configuration costs a few thousand reference pairs however many
queries it has.  Prints its seed; a mismatch names its configuration.
usage: clearance_fuzz.py [configs] [seed]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (TESTS, os.path.dirname(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)
import best_key_harness as best  # noqa: E402
import clearance_harness as ch  # noqa: E402
import clearance_ref as ref  # noqa: E402
from pair_list_harness import Uploaded  # noqa: E402

F = np.float32


LAST = {}   # of the last configuration: "zero_separated" = winners with hit = 0 and dist = +0 (a separated pair whose d2 underflowed),
            # "hits" / "misses" = winners with hit = 1 / hit = 0
TILE_ROWS, TILE_COLS, BLOCKS_PER_CU, strips_of = best.TILE_ROWS, best.TILE_COLS, best.BLOCKS_PER_CU, best.strips_of


def draw(wl, rng, idx, cus=None):
    """One configuration, drawn and judged by the reference, no GPU involved -> a dict of what run() needs.  cus: the device's
    number of compute units; without it the draw between the strip extremes never fires (its numbers are drawn all the same)."""
    rows_a, rows_b = (int(rng.choice([4, 8, 16])) for _ in range(2))
    da, db = int(rng.integers(1, 120)), int(rng.integers(1, 40))                  # distinct polygons
    n_a = int(rng.choice([1, 63, 64, 65, 255, 256, 257, int(rng.integers(1, 600))]))
    n_b = int(rng.choice([1, 2, 63, 64, 65, 129, 513, int(rng.integers(1, 700))]))
    extent = float(rng.choice([2.0, 8.0, 40.0, 400.0]))
    scale = int(rng.choice([0, 0, 0, 30, -30, 59, 70, -99, -110, -73, -74, -75]))   # 2^-73 .. 2^-75: d2 underflows where the exact test still separates
    no_k = bool(rng.random() < 0.2)
    self_set = bool(rng.random() < 0.2)
    seeds = [int(rng.integers(1 << 30)) for _ in range(2)]

    def make(n, rows, seed):
        s = wl.random_convex_polygon_set(n, seed=seed, kmin=rows if no_k else min(int(rng.integers(1, 4)), rows), kmax=rows, extent=extent, rows=rows)
        vx, vy, k = (x.copy() for x in s)
        if rng.random() < 0.3:                                                    # NaN / inf in real slots
            for q in rng.choice(n, max(1, n // 8), replace=False):
                (vx, vy)[int(rng.integers(2))][int(rng.integers(0, max(1, k[q]))), q] = rng.choice(np.array([np.nan, np.inf, -np.inf, 3e38], F))
        if not no_k and rng.random() < 0.4:                                       # counts out of range
            for q in rng.choice(n, max(1, n // 10), replace=False):
                k[q] = rng.choice([0, rows + 1, 255])
        with np.errstate(over="ignore"):
            return np.ldexp(vx, scale).astype(F), np.ldexp(vy, scale).astype(F), k

    a = make(da, rows_a, seeds[0])
    b = a if self_set else make(db, rows_b, seeds[1])
    ia = rng.integers(0, a[0].shape[1], n_a)
    ib = ia if self_set else rng.integers(0, b[0].shape[1], n_b)
    if not self_set and rng.random() < 0.3:
        ib = np.sort(ib)                                                          # runs of one obstacle
    rb, cb = (int(rng.choice([0, 0, 7, 1 << 20])) for _ in range(2))
    top = False
    if self_set:
        cb = rb
    else:
        top = bool(rng.random() < 0.2)                                            # up to exactly 2^32
    flags = ref.SKIP_SELF if (self_set or rng.random() < 0.2) else 0
    place = [(int(rng.integers(0, 4)), int(rng.integers(0, 9))) for _ in range(2)]
    # the last draws of the stream (every draw above is what it was before they were added): between one strip and one strip per
    # tile.  1 < strips < col_tiles needs three column tiles (a B of fewer is redrawn at 129 .. 700) and 8 * cus / strips row tiles.
    fire, pick, cut, n_b_between = rng.random() < 0.15, rng.random(), int(rng.integers(0, TILE_ROWS)), int(rng.integers(129, 701))
    between = ""
    if fire and cus and not self_set:
        if len(ib) <= 2 * TILE_COLS:
            ib = rng.integers(0, b[0].shape[1], n_b_between)
        col_tiles = -(-len(ib) // TILE_COLS)
        want_strips = 2 + int(pick * (col_tiles - 2))                             # 2 .. col_tiles - 1
        ia = rng.integers(0, a[0].shape[1], TILE_ROWS * (BLOCKS_PER_CU * cus // want_strips) - cut)
        strips = strips_of(cus, len(ia), len(ib))
        between = f", {strips} strips over {col_tiles} column tiles" if 1 < strips < col_tiles else ""
    if top:
        rb, cb = (1 << 32) - len(ia), (1 << 32) - len(ib)
    what = (f"config {idx}: {len(ia)} x {len(ib)} of {a[0].shape[1]} x {b[0].shape[1]} distinct, rows {rows_a} / {rows_b}, extent {extent}, scale 2^{scale}, "
            f"d_k {'NULL' if no_k else 'given'}, {'one set under SKIP_SELF' if self_set else 'two sets'}, bases {rb} / {cb}, flags {flags}, "
            f"planes (offset, stride - n) {place}, generator seeds {seeds}{between}")
    want = ch.indexed_reference(a, ia, b, ib, row_base=rb, col_base=cb, flags=flags)
    LAST["zero_separated"] = int(((want["hit"] == 0) & (want["dist"] == 0) & (want["poly"] != ref.NO_POLY)).sum())
    LAST["hits"], LAST["misses"] = int((want["hit"] == 1).sum()), int(((want["hit"] == 0) & (want["poly"] != ref.NO_POLY)).sum())
    LAST["between"] = bool(between)
    return dict(a=a, b=b, ia=ia, ib=ib, rb=rb, cb=cb, flags=flags, place=place, no_k=no_k, self_set=self_set, what=what, want=want)


def one(eng, wl, rng, idx, announce=None):
    """One configuration -> (ok, description); a vertex count out of range must be reported by the synchronise, once per call.
    `announce(text)` is called with the description before any GPU work."""
    c = draw(wl, rng, idx, eng.info()["compute_units"])
    a, b, ia, ib, place, no_k, self_set, what, want = (c[k] for k in ("a", "b", "ia", "ib", "place", "no_k", "self_set", "what", "want"))
    if announce is not None:
        announce(what)
    sa, sb = ch.take(a, ia), ch.take(b, ib)
    ua = Uploaded(eng, sa, offset=place[0][0], stride=len(ia) + place[0][1], with_k=not no_k)
    ub = ua if self_set else Uploaded(eng, sb, offset=place[1][0], stride=len(ib) + place[1][1], with_k=not no_k)
    bad = bool(ref.bad_counts(sa).any() or ref.bad_counts(sb).any()) and not no_k
    try:
        got = ch.twice(eng, ua.set, ub.set, len(ia), what, row_base=c["rb"], col_base=c["cb"], flags=c["flags"], expect_error=bad)
    finally:
        ua.free()
        if ub is not ua:
            ub.free()
    why = best.mismatch(got, want, ref.same, what)
    if why is not None:
        return False, why
    return True, what + f" [{LAST['zero_separated']} winners separated at dist 0]"


if __name__ == "__main__":
    best.fuzz_main("clearance_fuzz", one, needs_wl=True)
