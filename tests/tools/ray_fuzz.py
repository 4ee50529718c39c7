#!/usr/bin/env python3
"""Differential fuzz of c2d_poly_ray_casts against the CPU restatement of its contract (tests/ray_ref.py, pinned by
tests/test_ray_ref_cpu.py), after distance_fuzz.py: random numbers of rays and polygons on both sides of the kernel's tiles, row
layouts, vertex-count ranges, densities, strides and pointer offsets, col_base, ray planes at odd offsets; clockwise polygons, points
and segments, outliers, NaN / inf in real slots, junk in the padded slots (poly_broad_fuzz.py's random sets), duplicated polygons,
now and then a vertex count out of range; rays that start on a vertex or on an edge, point queries, rays of mixed scales and
non-finite rays.  Prints its seed; a mismatch names its configuration.
usage: ray_fuzz.py [configs] [seed]     (no seed: the commit's, tests/tools/fuzz_seed.py)"""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from __graft_entry__ import load_package  # noqa: E402
import best_key_harness as best  # noqa: E402
import ray_ref as ref  # noqa: E402

pkg = load_package()
wl = importlib.import_module("c2d_amd.workloads")
F = np.float32


pbf = best.load_tool("poly_broad_fuzz")      # its random sets and its upload
fuzz_seed = best.load_tool("fuzz_seed")


LAST = {}   # hits / misses of the last configuration, for the exploring leg's "not vacuous" check


def random_rays(rng, n, b):
    """n rays around the set b: a third start anywhere, the others on a vertex, on the middle of an edge or at a vertex mean"""
    vx, vy, k = b
    n_b = vx.shape[1]
    finite = np.isfinite(vx[0]) & np.isfinite(vy[0]) & (np.abs(vx[0]) < 1e6) & (np.abs(vy[0]) < 1e6) if n_b else np.zeros(0, bool)
    lo, hi = (float(min(vx[0][finite].min(), vy[0][finite].min())) - 2, float(max(vx[0][finite].max(), vy[0][finite].max())) + 2) if finite.any() else (-4.0, 4.0)
    ox, oy = rng.uniform(lo, hi, n).astype(F), rng.uniform(lo, hi, n).astype(F)
    if n_b:
        j = rng.integers(0, n_b, n)
        kk = np.clip(k[j].astype(np.int64), 1, vx.shape[0])
        e = rng.integers(0, 1 << 30, n) % kk
        e1 = (e + 1) % kk
        how = rng.integers(0, 6, n)
        with np.errstate(all="ignore"):
            mx, my = (vx[e, j] + vx[e1, j]) * F(0.5), (vy[e, j] + vy[e1, j]) * F(0.5)
            cx, cy = (vx[0, j] + vx[e, j] + vx[e1, j]) / F(3), (vy[0, j] + vy[e, j] + vy[e1, j]) / F(3)
        ox = np.where(how == 0, vx[e, j], np.where(how == 1, mx, np.where(how == 2, cx, ox))).astype(F)
        oy = np.where(how == 0, vy[e, j], np.where(how == 1, my, np.where(how == 2, cy, oy))).astype(F)
    ang = rng.uniform(0, 2 * np.pi, n)
    length = rng.uniform(0, (hi - lo) * float(rng.choice([0.05, 0.3, 1.5])), n)
    length = np.where(rng.random(n) < 0.1, 0.0, length)                       # point queries
    dx, dy = (length * np.cos(ang)).astype(F), (length * np.sin(ang)).astype(F)
    if rng.random() < 0.5:                                                    # axis-parallel and grid-aligned rays: exact ties
        grid = rng.random(n) < 0.3
        dx, dy = np.where(grid, np.round(dx), dx).astype(F), np.where(grid, 0, dy).astype(F)
        with np.errstate(all="ignore"):                                       # (an origin on a vertex of an outlier polygon can be huge)
            ox, oy = np.where(grid, np.round(ox * 4) / 4, ox).astype(F), np.where(grid, np.round(oy * 4) / 4, oy).astype(F)
    odd = np.flatnonzero(rng.random(n) < 0.03)
    junk = np.array([np.nan, np.inf, -np.inf, 3e38, 1e30, -1e30, 1e-30, 1e-42], F)
    for q in odd:
        (ox, oy, dx, dy)[int(rng.integers(0, 4))][q] = rng.choice(junk)
    return ox, oy, dx, dy


def one(eng, rng, idx, announce=None):
    """One configuration; `announce(text)` is called with its description BEFORE any GPU work.  Returns (ok, (description, records))."""
    n_b = int(rng.choice([0, 1, 2, 63, 64, 65, 129, 257, int(rng.integers(1, 1500))]))
    n_rays = int(rng.choice([1, 63, 64, 65, 257, int(rng.integers(1, 3000))]))
    n_rays = max(1, min(n_rays, (3 << 19) // max(n_b, 1)))
    rows = int(rng.integers(1, 17))
    cb = int(rng.choice([0, 0, 7, 1 << 20, (1 << 32) - n_b]))
    cap = n_rays + int(rng.choice([0, 1, 100]))
    offs = tuple(int(x) for x in rng.integers(0, 4, 4))
    b, db = pbf.random_set(rng, max(n_b, 1), rows)
    b = tuple(x[..., :n_b].copy() for x in b)
    if n_b > 3 and rng.random() < 0.5:                                       # duplicated polygons: the smaller index must win
        src, dst = rng.integers(0, n_b, n_b // 3), rng.integers(0, n_b, n_b // 3)
        for x in b:
            x[..., dst] = x[..., src]
    bad = n_b > 0 and rng.random() < 0.2
    if bad:
        b[2][int(rng.integers(0, n_b))] = rng.choice(np.array([0, rows + 1, 255], np.uint8))
    no_k = bool(n_b > 0 and not bad and (b[2] == rows).all())
    rays = random_rays(rng, n_rays, b)
    desc = f"config {idx}: {n_rays} rays in {cap} (plane offsets {offs}) x {n_b} polygons, {db}, col_base {cb}, bad count {bad}, d_k {'NULL' if no_k else 'given'}"
    if announce is not None:
        announce(desc)
    want = ref.ray_casts(rays, b, col_base=cb)
    keep = []
    if n_b:
        sb, keep = pbf.upload(eng, b, int(rng.integers(0, 4)), n_b + int(rng.integers(0, 9)))
        if no_k:
            sb = eng.poly_set(sb.d_vx, sb.d_vy, None, n_b, rows, sb.stride)
    else:
        sb = eng.poly_set(0, 0, None, 0, rows)
    host = np.full((4, n_rays + 4), np.nan, F)
    for p in range(4):
        host[p, offs[p]: offs[p] + n_rays] = rays[p]
    d_rays = eng.to_device(host)
    d_out = eng.empty(cap + 2, ref.RAY_HIT_DT)
    eng.memset(d_out, 0xA5, d_out.nbytes)
    eng.poly_ray_casts([d_rays.row(p) + 4 * offs[p] for p in range(4)], n_rays, sb, d_out.ptr + 16, col_base=cb)
    try:
        eng.synchronize()
        reported = False
    except pkg.C2DError:
        reported = True
    raw = d_out.get()
    for x in list(keep) + [d_rays, d_out]:
        x.free()
    got = raw[1:1 + n_rays]
    untouched = (np.delete(raw.view(np.uint8).reshape(-1, 16), np.arange(1, 1 + n_rays), axis=0) == 0xA5).all()
    ok = bool(ref.same(got, want).all()) and bool(untouched) and reported == bool(bad)
    LAST.update(hits=int((want["hit"] != 0).sum()), misses=int((want["hit"] == 0).sum()))
    if not ok:
        print(f"MISMATCH {desc}: {int((~ref.same(got, want)).sum())} records differ, untouched {bool(untouched)}, error reported {reported}")
    return ok, (desc, n_rays)


def main():
    configs = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed, origin = (int(sys.argv[2]), "the command line") if len(sys.argv) > 2 else fuzz_seed.commit_seed()
    print(f"ray_fuzz: {configs} configurations, seed {seed} ({origin})", flush=True)
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
