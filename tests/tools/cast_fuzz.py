#!/usr/bin/env python3
"""Differential fuzz of c2d_poly_set_casts against the CPU restatement of its contract (tests/cast_ref.py, pinned by
tests/test_cast_ref_cpu.py): the geometry of clearance_fuzz.py (set sizes on both sides of the kernel's tiles, row layouts, vertex-count
ranges, densities, repeated polygons, scales, NaN / inf in real slots, counts out of range, strides and pointer offsets, bases,
d_k == NULL, one set against itself under C2D_CAST_SKIP_SELF, launches between one strip and one strip per column tile) plus the
motions of sweep_fuzz.py per set (standing still, all zero, the scale of the scene, a hundredth of it, far larger, mixed scales with
exact zeros and non-finite components).  A motion belongs to a distinct polygon, so the reference is computed for the distinct
polygons and indexed.  Prints its seed; a mismatch names its configuration.
usage: cast_fuzz.py [configs] [seed]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (TESTS, os.path.dirname(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)
import best_key_harness as best  # noqa: E402
import cast_harness as ch  # noqa: E402
import cast_ref as ref  # noqa: E402


clearance_fuzz = best.load_tool("clearance_fuzz")      # its geometry
sweep_fuzz = best.load_tool("sweep_fuzz")              # its motions

LAST = {}   # of the last configuration: "hits" / "misses" = queries with / without a winner, "moving_hits" = winners with toi > 0


def draw(wl, rng, idx, cus=None):
    """One configuration, drawn and judged by the reference, no GPU involved -> a dict of what one() needs"""
    c = clearance_fuzz.draw(wl, rng, idx, cus)
    a, b, ia, ib = c["a"], c["b"], c["ia"], c["ib"]
    coords = np.concatenate([a[0][0], b[0][0]])
    finite = np.abs(coords[np.isfinite(coords)])
    scene = float(np.median(finite)) + float(np.ldexp(1.0, -100)) if finite.size else 1.0
    with np.errstate(all="ignore"):
        ma, name_a = sweep_fuzz.random_motion(rng, a[0].shape[1], scene)
        mb, name_b = (ma, name_a) if c["self_set"] else sweep_fuzz.random_motion(rng, b[0].shape[1], scene)
        want = ch.indexed_reference(a, ia, b, ib, ma, mb, row_base=c["rb"], col_base=c["cb"], flags=c["flags"])
    c.update(ma=ma, mb=mb, want=want, what=c["what"].replace("config", "cast config", 1) + f", motion A {name_a}, B {name_b}")
    LAST["hits"], LAST["misses"] = int((want["hit"] == 1).sum()), int(((want["hit"] == 0) & (want["flags"] == 0)).sum())
    LAST["moving_hits"] = int(((want["hit"] == 1) & (want["toi"] > 0)).sum())
    return c


def one(eng, wl, rng, idx, announce=None):
    """One configuration -> (ok, description); a vertex count out of range must be reported by the synchronise, once per call.
    `announce(text)` is called with the description before any GPU work."""
    c = draw(wl, rng, idx, eng.info()["compute_units"])
    a, b, ia, ib, place, no_k, self_set, what, want = (c[k] for k in ("a", "b", "ia", "ib", "place", "no_k", "self_set", "what", "want"))
    if announce is not None:
        announce(what)
    sa, sb = ch.take(a, ia), ch.take(b, ib)
    sc = ch.Scene(eng, sa, sb, ch.take_motion(c["ma"], ia), ch.take_motion(c["mb"], ib), place[0], place[1], with_k=not no_k, same=self_set)
    bad = bool(ref.bad_counts(sa).any() or ref.bad_counts(sb).any()) and not no_k
    try:
        got = ch.twice(eng, sc.a.set, sc.b_set, len(ia), what, row_base=c["rb"], col_base=c["cb"], flags=c["flags"], expect_error=bad, **sc.motions())
    finally:
        sc.free()
    why = best.mismatch(got, want, ref.same, what)
    if why is not None:
        return False, why
    return True, what + f" [{LAST['hits']} hits, {LAST['moving_hits']} of them later than t = 0, {LAST['misses']} misses]"


if __name__ == "__main__":
    best.fuzz_main("cast_fuzz", one, needs_wl=True)
