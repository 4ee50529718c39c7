#!/usr/bin/env python3
"""Differential fuzz of c2d_poly_pair_sweeps / c2d_rect_pair_sweeps against the CPU restatement of their contract
(tests/sweep_ref.py, pinned by tests/test_sweep_ref_cpu.py), after distance_fuzz.py: the same random sets, layouts, lists, bases and
device counts, plus a random motion per set — a set standing still (no planes), all zero, the scale of the scene, a hundredth of it,
far larger than it, a mix of scales per object with exact zeros among them, and now and then a non-finite component.  This file is
the generator; the call and the judge are pair_list_fuzz.py's.  Prints its seed; a mismatch names its configuration.
usage: sweep_fuzz.py [configs] [seed]     (no seed: the commit's, tests/tools/fuzz_seed.py)"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location("pair_list_fuzz", os.path.join(HERE, "pair_list_fuzz.py"))
plf = importlib.util.module_from_spec(spec)
spec.loader.exec_module(plf)            # the back half of every list-driven fuzz tool: run(), its judge, main(); it puts tests/ on the path
h = plf.h
contact_fuzz = plf.tool("contact_fuzz")      # its random list
distance_fuzz = plf.tool("distance_fuzz")      # its random sets

LAST = {}   # hits / misses of the last configuration, for an exploring leg's "not vacuous" check
MOTIONS = ("still", "zero", "scene", "small", "huge", "mixed")


def random_motion(rng, n, scene):
    """-> (the motion of a set of n objects whose coordinates span about `scene`: None or (dx, dy) f32[n]), its name"""
    kind = str(rng.choice(MOTIONS))
    if kind == "still":
        return None, kind
    if kind == "zero":
        return (np.zeros(n, np.float32), np.zeros(n, np.float32)), kind
    scale = {"scene": scene, "small": scene / 100, "huge": scene * float(rng.choice([1e3, 1e6, 1e30]))}.get(kind)
    if scale is None:       # per object: 2^-20 .. 2^20 of the scene, exact zeros, and a few non-finite components
        scale = scene * np.exp2(rng.uniform(-20, 20, n))
    m = [(rng.uniform(-1, 1, n) * scale).astype(np.float32) for _ in range(2)]
    if kind == "mixed":
        for plane in m:
            plane[rng.random(n) < 0.15] = 0.0
            odd = rng.random(n) < 0.02
            plane[odd] = rng.choice(np.array([np.nan, np.inf, -np.inf, 3e38], np.float32), int(odd.sum()))
    return (m[0], m[1]), kind


def _scene(coords):
    finite = np.abs(coords[np.isfinite(coords)])
    return float(np.median(finite)) + 1.0 if finite.size else 1.0


def one(eng, rng, idx, announce=None):
    """One configuration; `announce(text)` is called with its description BEFORE any GPU work.  Returns (ok, (description, records))."""
    n_a, n_b = (int(rng.choice([1, 2, 63, 64, 65, 257, int(rng.integers(1, 600))])) for _ in range(2))
    length = int(rng.choice([1, 63, 64, 65, 257, int(rng.integers(1, 5000))]))
    rb, cb = (int(rng.choice([0, 0, 7, 1 << 20, (1 << 32) - 700])) for _ in range(2))
    cap = length + int(rng.choice([0, 0, 1, 100]))
    n_dev = rng.choice([None, length, max(length - 1, 0), length // 2, cap + 5])
    a, b, place, what = distance_fuzz.random_sets(rng, n_a, n_b)
    n_b = (b.shape if place is None else b[0].shape)[1]
    scene = _scene(np.concatenate([a.ravel(), b.ravel()] if place is None else [a[0][0], b[0][0]]))
    (ma, name_a), (mb, name_b) = random_motion(rng, n_a, scene), random_motion(rng, n_b, scene)
    desc = f"config {idx}: {what}, motion A {name_a}, B {name_b}, list {length} in {cap}, count {n_dev}, bases {rb}, {cb}"
    if announce is not None:
        announce(desc)
    pairs = contact_fuzz.random_list(rng, n_a, n_b, length)
    ok, info, (want,) = plf.run(eng, h.SWEEPS, desc, a, b, pairs, cap, n_dev, rb, cb, place, extras=(ma, mb))
    LAST.update(plf.hits_and_misses([want]), moving_hits=int(h.sweep_classes(want)[1].sum()))
    return ok, info


if __name__ == "__main__":
    plf.main("sweep_fuzz", one, "records")
