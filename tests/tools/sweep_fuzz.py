#!/usr/bin/env python3
"""Differential fuzz of c2d_poly_pair_sweeps / c2d_rect_pair_sweeps against the CPU restatement of their contract
(tests/sweep_ref.py, pinned by tests/test_sweep_ref_cpu.py), after distance_fuzz.py: the same random sets, layouts, lists, bases and
device counts, plus a random motion per set — a set standing still (no planes), all zero, the scale of the scene, a hundredth of it,
far larger than it, a mix of scales per object with exact zeros among them, and now and then a non-finite component.  Prints its
seed; a mismatch names its configuration.
usage: sweep_fuzz.py [configs] [seed]     (no seed: the commit's, tests/tools/fuzz_seed.py)"""
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
import sweep_ref as ref  # noqa: E402

pkg = load_package()
wl = importlib.import_module("c2d_amd.workloads")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


pbf = _tool("poly_broad_fuzz")      # its random sets and its upload
contact_fuzz = _tool("contact_fuzz")      # its random list
distance_fuzz = _tool("distance_fuzz")      # its random quads
fuzz_seed = _tool("fuzz_seed")


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
    rects = bool(rng.random() < 0.3)
    if rects:
        a = distance_fuzz.random_quads(rng, n_a)
        b = a if (n_a == n_b and rng.random() < 0.3) else distance_fuzz.random_quads(rng, n_b)
        if rng.random() < 0.3:
            a = wl.inject_non_finite(a, seed=int(rng.integers(1 << 30)), frac=0.1)
        desc = f"config {idx}: rectangles {n_a} x {n_b}"
        keep = [eng.to_device(a), eng.to_device(b)]
        pa, pb = [keep[0].row(k) for k in range(8)], [keep[1].row(k) for k in range(8)]
        scene = _scene(np.concatenate([a.ravel(), b.ravel()]))
    else:
        a, da = pbf.random_set(rng, n_a, int(rng.integers(1, 17)))
        same = bool(rng.random() < 0.3)
        b, db = (a, da) if same else pbf.random_set(rng, n_b, int(rng.integers(1, 17)))
        n_b = b[0].shape[1]
        sa, keep = pbf.upload(eng, a, int(rng.integers(0, 4)), n_a + int(rng.integers(0, 9)))
        sb, keep_b = (sa, ()) if same else pbf.upload(eng, b, int(rng.integers(0, 4)), n_b + int(rng.integers(0, 9)))
        keep = list(keep) + list(keep_b)
        desc = f"config {idx}: polygons {n_a} x {n_b}, A {da}, B {'= A' if same else db}"
        scene = _scene(np.concatenate([a[0][0], b[0][0]]))
    (ma, name_a), (mb, name_b) = random_motion(rng, n_a, scene), random_motion(rng, n_b, scene)
    desc += f", motion A {name_a}, B {name_b}, list {length} in {cap}, count {n_dev}, bases {rb}, {cb}"
    if announce is not None:
        announce(desc)
    pairs = contact_fuzz.random_list(rng, n_a, n_b, length)
    listed = np.full((cap, 2), 0xFFFFFFFF, np.uint32)
    listed[:length] = ((pairs + (rb, cb)) & 0xFFFFFFFF).astype(np.uint32)
    # what the call sees is the u32 list minus the bases: an entry that wrapped is judged as the call judges it
    li, lj = listed[:, 0].astype(np.int64) - rb, listed[:, 1].astype(np.int64) - cb
    bound = cap if n_dev is None else min(cap, int(n_dev))
    want = (ref.rect_sweeps if rects else ref.poly_sweeps)(a, b, li[:bound], lj[:bound], ma, mb)
    d_pairs = eng.to_device(listed)
    d_out = eng.empty(cap + 2, ref.SWEEP_DT)
    eng.memset(d_out, 0xA5, d_out.nbytes)
    d_n = None if n_dev is None else eng.to_device(np.array([int(n_dev)], np.uint64))
    d_m = [None if m is None else eng.to_device(np.stack(m)) for m in (ma, mb)]
    dev_a, dev_b = (None if d is None else (d.row(0), d.row(1)) for d in d_m)
    if rects:
        eng.rect_pair_sweeps(pa, n_a, pb, n_b, d_pairs, cap, d_out.ptr + 16, a_motion=dev_a, b_motion=dev_b, n_pairs_dev=d_n, row_base=rb, col_base=cb)
    else:
        eng.poly_pair_sweeps(sa, sb, d_pairs, cap, d_out.ptr + 16, a_motion=dev_a, b_motion=dev_b, n_pairs_dev=d_n, row_base=rb, col_base=cb)
    try:
        eng.synchronize()
        reported = False
    except pkg.C2DError:
        reported = True
    raw = d_out.get()
    for x in keep + [d_pairs, d_out] + [d for d in d_m + [d_n] if d is not None]:
        x.free()
    got = raw[1:1 + bound]
    untouched = (np.delete(raw.view(np.uint8).reshape(-1, 16), np.arange(1, 1 + bound), axis=0) == 0xA5).all()
    ok = bool(ref.same(got, want).all()) and bool(untouched) and reported == bool((want["flags"] & ref.BAD_PAIR).any())
    start = (want["flags"] & ref.START_OVERLAP) != 0
    LAST.update(hits=int((want["hit"] != 0).sum()), misses=int((want["hit"] == 0).sum()), moving_hits=int(((want["hit"] != 0) & ~start).sum()))
    if not ok:
        print(f"MISMATCH {desc}: {int((~ref.same(got, want)).sum())} records differ, untouched {bool(untouched)}, error reported {reported}")
    return ok, (desc, bound)


def main():
    configs = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed, origin = (int(sys.argv[2]), "the command line") if len(sys.argv) > 2 else fuzz_seed.commit_seed()
    print(f"sweep_fuzz: {configs} configurations, seed {seed} ({origin})", flush=True)
    rng = np.random.default_rng(seed)
    eng = pkg.Engine(0)
    fails = total = 0
    for i in range(configs):
        ok, info = one(eng, rng, i)
        fails += not ok
        total += info[-1]
        if (i + 1) % 50 == 0:
            print(f"  {i + 1} / {configs} configurations, {fails} failures so far", flush=True)
    print(f"{configs} configurations, {fails} failures; {total} records compared")
    eng.close()
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    main()
