#!/usr/bin/env python3
"""Developer tool: the shape casts (c2d_poly_set_casts) against the engine's way to answer the question before they existed,
c2d_poly_pair_sweeps on the materialised all-pairs list of the same sets (its reduction by the caller not counted), one JSON line per
configuration.  GPU only, no oracle (tests/test_gpu_casts.py checks the records).

Scene: the sparse generator (workloads.random_convex_polygon_set: K ~ U{3..16}, radii 0.3 .. 2.5) with extent 200 * sqrt(N / 32768),
N the number of obstacles, queries and obstacles in the same box, every polygon of both sets moving by up to +-4 per component (a few
polygon radii).  Shapes n_a x n_b: 4096 x 4096, 131072 x 4096 and 4096 x 131072, each with the queries as generated (unsorted) and
sorted along a Morton curve over their first vertices.  Per configuration:
  cast_ms          the call (three launches), HIP events, median of --reps after a warm-up
  pairs_per_s      n_a * n_b / cast time
  yardstick_ns_per_pair   c2d_poly_pair_sweeps over the all-pairs list of the first --yard-rows queries against all obstacles (2^25
                   listed pairs at most), median of --reps, per pair; ratio = yardstick time scaled to n_a * n_b / cast time
  past_first_axis  the share of (lane, j) that the exact abandon does not end after the first axis, modelled on the host for the
                   first --model-rows queries: the first axis chosen as the kernel chooses it (in float64: a statistic, not a
                   result), its lo / hi by numpy, the lane's best walked in the kernel's strips over the yardstick's own records;
                   past_first_axis_wave: the same per wave of 64 consecutive queries (a wave goes on when a lane does)
usage: cast_bench.py [--shapes 4096x4096,131072x4096,4096x131072] [--reps 7] [--yard-rows 4096] [--model-rows 256]"""
import argparse
import importlib
import json
import os
import sys

import torch  # before libc2d.so
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
wl = importlib.import_module("c2d_amd.workloads")
F = np.float32
TILE_ROWS, TILE_COLS = 256, 64


def morton_order(s):
    x, y = s[0][0].astype(np.float64), s[1][0].astype(np.float64)
    q = lambda v: np.clip(((v - v.min()) / max(v.max() - v.min(), 1e-30) * 65535).astype(np.uint64), 0, 65535)  # noqa: E731

    def spread(v):
        v = (v | (v << np.uint64(8))) & np.uint64(0x00FF00FF)
        v = (v | (v << np.uint64(4))) & np.uint64(0x0F0F0F0F)
        v = (v | (v << np.uint64(2))) & np.uint64(0x33333333)
        return (v | (v << np.uint64(1))) & np.uint64(0x55555555)
    return np.argsort(spread(q(x)) | (spread(q(y)) << np.uint64(1)), kind="stable")


def first_axis(a, ma, b, mb):
    """per pair of a x b (finite polygons) what the first axis of csrc/c2d_cast.hip leaves: sep, never, t_in, t_out [n_a][n_b]"""
    n_a, n_b = a[0].shape[1], b[0].shape[1]
    ax, ay, ka = a[0].astype(np.float64), a[1].astype(np.float64), a[2].astype(np.int64)
    bx, by, kb = b[0].astype(np.float64), b[1].astype(np.float64), b[2].astype(np.int64)
    rows = np.arange(16)[:, None]
    live_a, live_b = rows < ka[None, :], rows < kb[None, :]
    cx = 0.5 * np.where(live_a, ax, np.inf).min(0) + 0.5 * np.where(live_a, ax, -np.inf).max(0)
    cy = 0.5 * np.where(live_a, ay, np.inf).min(0) + 0.5 * np.where(live_a, ay, -np.inf).max(0)
    nxt = np.where(rows + 1 < kb[None, :], rows + 1, 0)
    cols = np.arange(n_b)[None, :]
    nx, ny = -(by[nxt, cols] - by), bx[nxt, cols] - bx                          # [16][n_b]: the true normals of B's edges
    proj = nx[:, None, :] * bx[None, :, :] + ny[:, None, :] * by[None, :, :]      # [edge][vertex][n_b]
    mnb = np.where(live_b[None, :, :], proj, np.inf).min(1)
    mxb = np.where(live_b[None, :, :], proj, -np.inf).max(1)
    pa = nx * bx + ny * by
    sg = np.where((mxb - pa) > (pa - mnb), -1.0, 1.0)
    with np.errstate(all="ignore"):
        inv = sg / np.sqrt(nx * nx + ny * ny)
    ux, uy, off = nx * inv, ny * inv, pa * inv
    score = ux[:, None, :] * cx[None, :, None] + uy[:, None, :] * cy[None, :, None] - off[:, None, :]     # [edge][n_a][n_b]
    score = np.where(live_b[:, None, :] & ~np.isnan(score), score, -np.inf)
    fe = score.argmax(0)                                                          # [n_a][n_b]
    jj = np.broadcast_to(np.arange(n_b)[None, :], (n_a, n_b))
    fx, fy, fmn, fmx = nx[fe, jj], ny[fe, jj], mnb[fe, jj], mxb[fe, jj]
    mna, mxa = np.full((n_a, n_b), np.inf), np.full((n_a, n_b), -np.inf)
    for r in range(16):
        p = np.where(live_a[r][:, None], fx * ax[r][:, None] + fy * ay[r][:, None], np.nan)
        mna, mxa = np.fmin(mna, p), np.fmax(mxa, p)
    sep = (mxa < fmn) | (fmx < mna)
    o1, o2 = mxa - fmn, fmx - mna
    v = fx * (mb[0].astype(np.float64)[None, :] - ma[0].astype(np.float64)[:, None]) + fy * (mb[1].astype(np.float64)[None, :] - ma[1].astype(np.float64)[:, None])
    with np.errstate(all="ignore"):
        lo, hi = np.where(v > 0, -o2 / v, o1 / v), np.where(v > 0, o1 / v, -o2 / v)
    never = (v == 0) & ((o1 < 0) | (o2 < 0))
    return sep, never, np.where((v != 0) & (lo > 0), lo, 0.0), np.where((v != 0) & (hi < 1), hi, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x4096,131072x4096,4096x131072")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--yard-rows", type=int, default=4096)
    ap.add_argument("--model-rows", type=int, default=256)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    sh = stream.cuda_stream
    cus = eng.info()["compute_units"]

    def timed(fn, reps):
        fn()
        stream.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            stream.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    def upload(s, m):
        t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in tuple(s) + tuple(m)]
        return t, eng.poly_set(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), s[0].shape[1], wl.KMAX), (t[3].data_ptr(), t[4].data_ptr())

    size = pkg.CAST_DT.itemsize
    for shape in args.shapes.split(","):
        n_a, n_b = (int(v) for v in shape.split("x"))
        extent = 200.0 * np.sqrt(n_b / 32768)
        a0 = wl.random_convex_polygon_set(n_a, seed=0xCA57, extent=extent)
        b = wl.random_convex_polygon_set(n_b, seed=0xCA58, extent=extent)
        rng = np.random.default_rng(0xCA59)
        ma0, mb = (tuple((rng.uniform(-4, 4, n)).astype(F) for _ in range(2)) for n in (n_a, n_b))
        tb, sb, pb = upload(b, mb)
        for order in ("unsorted", "sorted"):
            perm = np.arange(n_a) if order == "unsorted" else morton_order(a0)
            a, ma = tuple(np.ascontiguousarray(x[..., perm]) for x in a0), tuple(np.ascontiguousarray(m[perm]) for m in ma0)
            ta, sa, pa = upload(a, ma)
            out_t = torch.empty((n_a, size), dtype=torch.uint8, device=dev)
            ms = timed(lambda: eng.poly_set_casts(sa, sb, pa, pb, 0, 0, 0, out_t.data_ptr(), sh), args.reps)
            rec = out_t.cpu().numpy().view(pkg.CAST_DT).reshape(-1)
            row_tiles, col_tiles = -(-n_a // TILE_ROWS), -(-n_b // TILE_COLS)
            strips = min(col_tiles, max(1, 8 * cus // row_tiles))
            res = {"config": f"{n_a}x{n_b}_{order}", "n_a": n_a, "n_b": n_b, "extent": round(float(extent), 2), "strips": strips, "cast_ms": round(ms, 4),
                   "pairs_per_s": round(n_a * n_b / (ms * 1e-3), 1), "hit_share": round(float((rec["hit"] == 1).mean()), 4),
                   "start_overlap_share": round(float((rec["flags"] == pkg.SWEEP_START_OVERLAP).mean()), 4)}
            # the yardstick: the all-pairs list of the first rows against all of B through the sweep kernel (unchanged code)
            rows = max(64, min(args.yard_rows, n_a, (1 << 25) // n_b))     # (at most 2^25 listed pairs: 512 MiB of records, 256 MiB of list)
            pairs = torch.stack([torch.arange(rows, device=dev, dtype=torch.int32).repeat_interleave(n_b),
                                 torch.arange(n_b, device=dev, dtype=torch.int32).repeat(rows)], dim=1).contiguous()
            sw_t = torch.empty((rows * n_b, 16), dtype=torch.uint8, device=dev)
            yard_ms = timed(lambda: eng.poly_pair_sweeps(sa, sb, pairs.data_ptr(), rows * n_b, sw_t.data_ptr(), a_motion=pa, b_motion=pb, stream=sh), args.reps)
            per_pair = yard_ms * 1e-3 / (rows * n_b)
            res["yardstick_ns_per_pair"] = round(per_pair * 1e9, 4)
            res["yardstick_pairs_per_s"] = round(1.0 / per_pair, 1)
            res["ratio"] = round(per_pair * n_a * n_b / (ms * 1e-3), 2)
            # the caller's reduction of the yardstick's rows names the same winners
            S = sw_t.cpu().numpy().view(pkg.SWEEP_DT).reshape(rows, n_b)
            key = np.where(S["hit"] == 1, S["toi"], np.inf)
            win = key.argmin(axis=1)
            hit = np.isfinite(key[np.arange(rows), win])
            assert np.array_equal(rec["hit"][:rows] == 1, hit) and np.array_equal(rec["poly"][:rows][hit], win[hit].astype(np.uint32)), res["config"]
            # what the abandon leaves after the first axis, on the host: the strips' walk in order of j over the yardstick's records
            m = min(args.model_rows, rows)
            parts = [first_axis(tuple(x[..., :m] for x in a), tuple(x[:m] for x in ma), tuple(x[..., c:c + 4096] for x in b), tuple(x[c:c + 4096] for x in mb))
                     for c in range(0, n_b, 4096)]      # (in chunks of obstacles: the scores are 16 x m x 4096 doubles at a time)
            sep, never, t_in, t_out = (np.concatenate([p[q] for p in parts], axis=1) for q in range(4))
            past = np.zeros((m, n_b), bool)
            per = [col_tiles // strips + (1 if s < col_tiles % strips else 0) for s in range(strips)]
            first = 0
            for tiles in per:
                j0, j1 = first * TILE_COLS, min((first + tiles) * TILE_COLS, n_b)
                first += tiles
                best = np.full(m, np.inf)
                for j in range(j0, j1):
                    live = best != 0
                    past[:, j] = live & ~(sep[:, j] & (never[:, j] | (t_in[:, j] > t_out[:, j]) | (t_in[:, j] >= best)))
                    best = np.where(live & (key[:m, j] < best), key[:m, j], best)
            res["past_first_axis"] = round(float(past.mean()), 5)
            res["past_first_axis_wave"] = round(float(past[: m - m % 64].reshape(-1, 64, n_b).any(axis=1).mean()), 5)
            print(json.dumps(res), flush=True)
            del ta, out_t, pairs, sw_t
        del tb
        torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
