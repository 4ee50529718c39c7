#!/usr/bin/env python3
"""Differential fuzz of c2d_poly_set_casts_grid against the CPU restatement of the cast contract (tests/cast_ref.py) and, in the same
run, against c2d_poly_set_casts byte for byte.  The configurations are cast_fuzz.py's (its geometry, its motions, its judge: set
sizes on both sides of the tiles, row layouts, repeated polygons, scales, NaN / inf in real slots, counts out of range, strides and
offsets, bases, d_k == NULL, one set under C2D_CAST_SKIP_SELF) with what a grid can get wrong on top, drawn behind cast_fuzz's own
draws: B's indices dealt in another order (shuffled or reversed, so that the cell order of the walk and the index order disagree),
and a few movers that are fast (their swept boxes span many cells: wild in the pipeline) or wild by the motion itself (non-finite,
2^60 and more).  draw() makes a configuration and the reference's records without a GPU; one() runs it; judge() compares.  Prints its
seed; a mismatch names its configuration.
usage: cast_grid_fuzz.py [configs] [seed]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (TESTS, os.path.dirname(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)
import best_key_harness as best  # noqa: E402
import cast_grid_harness as cg  # noqa: E402
import cast_harness as ch  # noqa: E402
import cast_ref as ref  # noqa: E402


cast_fuzz = best.load_tool("cast_fuzz")      # its generators: clearance_fuzz's geometry with sweep_fuzz's motions

LAST = {}   # of the last configuration: "hits" / "misses" = queries with / without a winner, "moving_hits" = winners with toi > 0
ODD = np.array([np.nan, np.inf, -np.inf, 3e38, 2.0 ** 60, -2.0 ** 61], np.float32)


def _movers(rng, motion, n, scene):
    """a few of the n distinct polygons made fast (3 .. 300 scenes per step) or wild by their motion -> (motion, how many)"""
    if n == 0 or rng.random() < 0.4:
        return motion, 0
    m = [np.zeros(n, np.float32), np.zeros(n, np.float32)] if motion is None else [motion[0].copy(), motion[1].copy()]
    who = rng.choice(n, max(1, n // int(rng.choice([3, 10, 30]))), replace=False)
    for q in who:
        if rng.random() < 0.7:
            ang, far = rng.uniform(0, 2 * np.pi), scene * float(np.exp(rng.uniform(np.log(3.0), np.log(300.0))))
            with np.errstate(over="ignore"):
                m[0][q], m[1][q] = np.float32(far * np.cos(ang)), np.float32(far * np.sin(ang))
        else:
            m[int(rng.integers(2))][q] = rng.choice(ODD)
    return (m[0], m[1]), len(who)


def draw(wl, rng, idx, cus=None):
    """One configuration, drawn and judged by the reference, no GPU involved -> a dict of what one() needs"""
    c = cast_fuzz.draw(wl, rng, idx, cus)
    a, b, ia, ib, ma, mb = (c[k] for k in ("a", "b", "ia", "ib", "ma", "mb"))
    coords = np.concatenate([a[0][0], b[0][0]])
    finite = np.abs(coords[np.isfinite(coords)])
    scene = float(np.median(finite)) + float(np.ldexp(1.0, -100)) if finite.size else 1.0
    ma, fast_a = _movers(rng, ma, a[0].shape[1], scene)
    if c["self_set"]:
        mb, fast_b = ma, fast_a
    else:
        mb, fast_b = _movers(rng, mb, b[0].shape[1], scene)
    order = str(rng.choice(["as drawn", "shuffled", "shuffled", "reversed"]))
    if order != "as drawn":
        perm = rng.permutation(len(ib)) if order == "shuffled" else np.arange(len(ib))[::-1]
        ib = ib[perm]
        if c["self_set"]:
            ia = ib                                                   # one set: the queries are the same memory
    with np.errstate(all="ignore"):
        want = ch.indexed_reference(a, ia, b, ib, ma, mb, row_base=c["rb"], col_base=c["cb"], flags=c["flags"])
    c.update(ia=ia, ib=ib, ma=ma, mb=mb, want=want,
             what=c["what"].replace("cast config", "cast grid config", 1) + f", B {order}, fast or wild movers {fast_a} / {fast_b}")
    LAST["hits"], LAST["misses"] = int((want["hit"] == 1).sum()), int(((want["hit"] == 0) & (want["flags"] == 0)).sum())
    LAST["moving_hits"] = int(((want["hit"] == 1) & (want["toi"] > 0)).sum())
    return c


def judge(got, want):
    """None when the records `got` equal the reference's, else what differs"""
    if len(got) != len(want):
        return f"{len(got)} records, the reference has {len(want)}"
    ok = ref.same(got, want)
    if ok.all():
        return None
    q = int(np.flatnonzero(~ok)[0])
    fields = [f for f in want.dtype.names if not ref.same(_only(got, q, f, want), want[q:q + 1])[0]]
    return f"{int((~ok).sum())} of {len(want)} records differ; first at query {q} in {fields}: got {got[q]}, want {want[q]}"


def _only(got, q, f, want):
    """the reference's record q with field f taken from `got`"""
    rec = want[q:q + 1].copy()
    rec[f] = got[f][q]
    return rec


def one(eng, wl, rng, idx, announce=None):
    """One configuration -> (ok, description): the grid call twice (the same bytes), the reference, and c2d_poly_set_casts in the same
    run (the same bytes); a vertex count out of range must be reported by the synchronise, once per call.
    `announce(text)` is called with the description before any GPU work."""
    c = draw(wl, rng, idx, eng.info()["compute_units"])
    a, b, ia, ib, place, no_k, self_set, what, want = (c[k] for k in ("a", "b", "ia", "ib", "place", "no_k", "self_set", "what", "want"))
    if announce is not None:
        announce(what)
    sa, sb = ch.take(a, ia), ch.take(b, ib)
    sc = ch.Scene(eng, sa, sb, ch.take_motion(c["ma"], ia), ch.take_motion(c["mb"], ib), place[0], place[1], with_k=not no_k, same=self_set)
    bad = bool(ref.bad_counts(sa).any() or ref.bad_counts(sb).any()) and not no_k
    try:
        got = cg.check(eng, sc.a.set, sc.b_set, len(ia), None, what, row_base=c["rb"], col_base=c["cb"], flags=c["flags"], expect_error=bad, **sc.motions())
    except AssertionError as e:
        return False, what + f": {e}"
    finally:
        sc.free()
    why = judge(got, want)
    if why is not None:
        return False, what + ": " + why
    return True, what + f" [{LAST['hits']} hits, {LAST['moving_hits']} of them later than t = 0, {LAST['misses']} misses]"


if __name__ == "__main__":
    best.fuzz_main("cast_grid_fuzz", one, needs_wl=True)
