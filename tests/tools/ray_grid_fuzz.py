#!/usr/bin/env python3
"""Differential fuzz of c2d_poly_ray_casts_grid against the CPU restatement of its contract (tests/ray_grid_ref.py, pinned by
tests/test_ray_grid_ref_cpu.py): ray_fuzz.py's inputs (random numbers of rays and polygons, row layouts, strides, pointer offsets,
col_base, ray planes at odd offsets, clockwise polygons, points and segments, outliers, NaN / inf, junk in the padded slots, bad
counts, rays on vertices and edges, point queries, non-finite rays) plus what bears on a grid: polygons clustered in a few cells (long
walks, listed rays), polygons duplicated many times, and outsized polygons that span many cells or reach far outside the others'
bounds.  Every configuration runs twice (the same bytes) and is compared with the reference.  Prints its seed; a mismatch names its
configuration.
usage: ray_grid_fuzz.py [configs] [seed]     (no seed: the commit's, tests/tools/fuzz_seed.py)"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import best_key_harness as best  # noqa: E402
import ray_grid_ref as gref  # noqa: E402


rf = best.load_tool("ray_fuzz")              # its rays, its random sets (poly_broad_fuzz.py's) and its package
pkg, pbf, fuzz_seed = rf.pkg, rf.pbf, rf.fuzz_seed
F = np.float32

LAST = {}   # hits / misses / listed rays of the last configuration


def reshape_for_a_grid(rng, b):
    """clusters, duplicates and outsized polygons, in place; -> what was done"""
    vx, vy, k = b
    rows, n = vx.shape
    done = []
    live = np.arange(rows)[:, None] < np.clip(k.astype(np.int64), 0, rows)[None, :]
    if n > 8 and rng.random() < 0.5:            # a cluster: a share of the polygons moved into one small spot
        who = np.flatnonzero(rng.random(n) < rng.choice([0.2, 0.6, 1.0]))
        with np.errstate(all="ignore"):
            cx, cy = np.where(live, vx, 0).sum(0) / np.maximum(live.sum(0), 1), np.where(live, vy, 0).sum(0) / np.maximum(live.sum(0), 1)
            spot = rng.uniform(-3, 3, 2)
            vx[:, who] = (vx[:, who] - cx[who] + spot[0] + rng.uniform(-1, 1, len(who))).astype(F)
            vy[:, who] = (vy[:, who] - cy[who] + spot[1] + rng.uniform(-1, 1, len(who))).astype(F)
        done.append(f"cluster of {len(who)}")
    if n > 3 and rng.random() < 0.5:            # duplicates: the smaller index must win
        m = int(rng.choice([n // 3, min(n - 1, 1100)]))
        src = int(rng.integers(0, n))
        dst = rng.choice(n, m, replace=False)
        for x in (vx, vy, k):
            x[..., dst] = x[..., [src]]
        done.append(f"{m} copies of one polygon")
    if n > 1 and rng.random() < 0.6:            # outsized: many cells wide, or far outside the others' bounds
        for q in rng.choice(n, min(n, int(rng.integers(1, 8))), replace=False):
            with np.errstate(all="ignore"):
                if rng.random() < 0.5:
                    f = F(rng.choice([8.0, 100.0, 1e4]))
                    vx[:, q], vy[:, q] = vx[:, q] * f, vy[:, q] * f
                else:
                    vx[:, q] += F(rng.choice([1e3, -1e5, 1e9]))
        done.append("outsized")
    return ", ".join(done) or "as drawn"


def one(eng, rng, idx, announce=None):
    """One configuration; `announce(text)` is called with its description BEFORE any GPU work.  Returns (ok, (description, records))."""
    n_b = int(rng.choice([0, 1, 2, 63, 64, 65, 513, 1100, int(rng.integers(1, 1500)), int(rng.integers(1500, 5000))]))
    n_rays = int(rng.choice([1, 63, 64, 65, 257, int(rng.integers(1, 3000))]))
    n_rays = max(1, min(n_rays, (3 << 19) // max(n_b, 1)))
    rows = int(rng.integers(1, 17))
    cb = int(rng.choice([0, 0, 7, 1 << 20, (1 << 32) - n_b]))
    cap = n_rays + int(rng.choice([0, 1, 100]))
    offs = tuple(int(x) for x in rng.integers(0, 4, 4))
    b, db = pbf.random_set(rng, max(n_b, 1), rows)
    b = tuple(x[..., :n_b].copy() for x in b)
    shaped = reshape_for_a_grid(rng, b) if n_b else "empty"
    bad = n_b > 0 and rng.random() < 0.2
    if bad:
        b[2][int(rng.integers(0, n_b))] = rng.choice(np.array([0, rows + 1, 255], np.uint8))
    no_k = bool(n_b > 0 and not bad and (b[2] == rows).all())
    rays = rf.random_rays(rng, n_rays, b)
    desc = (f"config {idx}: {n_rays} rays in {cap} (plane offsets {offs}) x {n_b} polygons, {db}, {shaped}, col_base {cb}, bad count {bad}, "
            f"d_k {'NULL' if no_k else 'given'}")
    if announce is not None:
        announce(desc)
    want = gref.ray_casts(rays, b, col_base=cb)
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
    d_out = eng.empty(cap + 2, gref.RAY_HIT_DT)
    raws, reported = [], []
    for _ in range(2):
        eng.memset(d_out, 0xA5, d_out.nbytes)
        eng.poly_ray_casts_grid([d_rays.row(p) + 4 * offs[p] for p in range(4)], n_rays, sb, d_out.ptr + 16, col_base=cb)
        try:
            eng.synchronize()
            reported.append(False)
        except pkg.C2DError:
            reported.append(True)
        raws.append(d_out.get())
    listed = eng.poly_ray_casts_grid_stats()["listed"] if n_b else 0
    for x in list(keep) + [d_rays, d_out]:
        x.free()
    raw = raws[0]
    got = raw[1:1 + n_rays]
    untouched = (np.delete(raw.view(np.uint8).reshape(-1, 16), np.arange(1, 1 + n_rays), axis=0) == 0xA5).all()
    ok = bool(gref.same(got, want).all()) and bool(untouched) and reported == [bool(bad)] * 2 and raws[0].tobytes() == raws[1].tobytes()
    LAST.update(hits=int((want["hit"] != 0).sum()), misses=int((want["hit"] == 0).sum()), listed=int(listed))
    if not ok:
        print(f"MISMATCH {desc}: {int((~gref.same(got, want)).sum())} records differ, untouched {bool(untouched)}, error reported {reported}, "
              f"two runs equal {raws[0].tobytes() == raws[1].tobytes()}")
    return ok, (desc, n_rays)


def main():
    configs = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed, origin = (int(sys.argv[2]), "the command line") if len(sys.argv) > 2 else fuzz_seed.commit_seed()
    print(f"ray_grid_fuzz: {configs} configurations, seed {seed} ({origin})", flush=True)
    rng = np.random.default_rng(seed)
    eng = pkg.Engine(0)
    fails = total = listed = 0
    for i in range(configs):
        ok, info = one(eng, rng, i)
        fails += not ok
        total += info[-1]
        listed += LAST["listed"]
        if (i + 1) % 50 == 0:
            print(f"  {i + 1} / {configs} configurations, {fails} failures so far", flush=True)
    print(f"{configs} configurations, {fails} failures; {total} records compared, {listed} rays took the one-ray-per-wave route")
    eng.close()
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    main()
