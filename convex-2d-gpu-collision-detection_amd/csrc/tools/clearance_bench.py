#!/usr/bin/env python3
"""Developer tool: the clearance query (c2d_poly_set_clearances) against the engine's way to answer the question before it existed,
c2d_poly_pair_distances on the materialised all-pairs list of the same sets (its reduction by the caller not counted), one JSON line
per configuration.  GPU only, no oracle (tests/test_gpu_clearances.py checks the records).

Scene: the sparse generator (workloads.random_convex_polygon_set: K ~ U{3..16}, radii 0.3 .. 2.5) with extent 200 * sqrt(N / 32768),
N the number of obstacles, queries and obstacles in the same box.  Shapes n_a x n_b: 4096 x 4096, 131072 x 4096 and 4096 x 131072,
each with the queries as generated (unsorted) and sorted along a Morton curve over their first vertices (the lanes of a wave share
their skips only if neighbouring queries are neighbours in space).  Per configuration:
  clearance_ms     the call (three launches), HIP events, median of --reps after a warm-up
  noskip_ms        the same from lib/libc2d_clr_noskip.so (`make lib-ab-clearance`: the kernel without its certified skip), when built;
                   its records must be the same bytes (asserted)
  pairs_per_s      n_a * n_b / clearance time
  yardstick_ns_per_pair   c2d_poly_pair_distances over the all-pairs list of the first --yard-rows queries against all obstacles
                   (2^26 listed pairs at most: 2.5 GiB of list and records; 4096 x 4096 is listed whole), median of --reps, per pair; ratio = yardstick time scaled to n_a * n_b / clearance time (ratio_noskip likewise)
  entered_share    the share of (lane, j) that enter the candidate loops, counted on the host for the first --yard-rows queries with
                   the numpy statement of the bound below over the yardstick's own distances (dist * dist stands for d2) walked in
                   the kernel's strips; entered_share_wave: the same per wave of 64 consecutive queries (a wave enters when a lane does)
usage: clearance_bench.py [--shapes 4096x4096,131072x4096,4096x131072] [--reps 7] [--yard-rows 4096]"""
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


def boxes(s):
    """xlo, xhi, ylo, yhi, largest |coordinate| of every polygon's live vertices (finite input)"""
    vx, vy, k = s
    live = np.arange(vx.shape[0])[:, None] < k[None, :].astype(np.int64)
    x, y = np.where(live, vx, np.nan), np.where(live, vy, np.nan)
    return np.stack([np.nanmin(x, 0), np.nanmax(x, 0), np.nanmin(y, 0), np.nanmax(y, 0), np.fmax(np.nanmax(np.abs(x), 0), np.nanmax(np.abs(y), 0))]).astype(F)


def lb2(a, b):
    """the numpy statement of clearance_lb2 (csrc/c2d_clearance_bound.hpp), a f32[5][n_a] against b f32[5][n_b] -> f32[n_a][n_b]
    (tests/test_clearance_bound_cpu.py holds the statement of tests/clearance_cases.py to the header bit for bit; this is the same
    arithmetic on finite boxes)"""
    C = np.maximum(a[4][:, None], b[4][None, :])
    ok = (C >= F(2.0 ** -100)) & (C <= F(2.0 ** 60))
    g = np.maximum(np.maximum(b[0][None, :] - a[1][:, None], a[0][:, None] - b[1][None, :]), np.maximum(b[2][None, :] - a[3][:, None], a[2][:, None] - b[3][None, :]))
    L = (g - F(2.0 ** -21) * C).astype(F)
    return np.where(ok & (L > 0), L * L, F(0)).astype(F)


def morton_order(s):
    x, y = s[0][0].astype(np.float64), s[1][0].astype(np.float64)
    q = lambda v: np.clip(((v - v.min()) / max(v.max() - v.min(), 1e-30) * 65535).astype(np.uint64), 0, 65535)  # noqa: E731

    def spread(v):
        v = (v | (v << np.uint64(8))) & np.uint64(0x00FF00FF)
        v = (v | (v << np.uint64(4))) & np.uint64(0x0F0F0F0F)
        v = (v | (v << np.uint64(2))) & np.uint64(0x33333333)
        return (v | (v << np.uint64(1))) & np.uint64(0x55555555)
    return np.argsort(spread(q(x)) | (spread(q(y)) << np.uint64(1)), kind="stable")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x4096,131072x4096,4096x131072")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--yard-rows", type=int, default=4096)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    noskip_path = os.path.join(os.path.dirname(pkg.library_path()), "libc2d_clr_noskip.so")
    eng_noskip = pkg.Engine(0, lib_path=noskip_path) if os.path.exists(noskip_path) else None
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

    def upload(e, s):
        t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in s]
        return t, e.poly_set(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), s[0].shape[1], wl.KMAX)

    for shape in args.shapes.split(","):
        n_a, n_b = (int(v) for v in shape.split("x"))
        extent = 200.0 * np.sqrt(n_b / 32768)
        a0 = wl.random_convex_polygon_set(n_a, seed=0xC1EA, extent=extent)
        b = wl.random_convex_polygon_set(n_b, seed=0xC1EB, extent=extent)
        tb, sb = upload(eng, b)
        for order in ("unsorted", "sorted"):
            a = a0 if order == "unsorted" else tuple(np.ascontiguousarray(x[..., morton_order(a0)]) for x in a0)
            ta, sa = upload(eng, a)
            out_t = torch.empty((n_a, 32), dtype=torch.uint8, device=dev)
            ms = timed(lambda: eng.poly_set_clearances(sa, sb, out_t.data_ptr(), stream=sh), args.reps)
            rec = out_t.cpu().numpy().view(pkg.CLEARANCE_DT).reshape(-1)
            row_tiles, col_tiles = -(-n_a // TILE_ROWS), -(-n_b // TILE_COLS)
            strips = min(col_tiles, max(1, 8 * cus // row_tiles))
            res = {"config": f"{n_a}x{n_b}_{order}", "n_a": n_a, "n_b": n_b, "extent": round(float(extent), 2), "strips": strips,
                   "clearance_ms": round(ms, 4), "pairs_per_s": round(n_a * n_b / (ms * 1e-3), 1), "hit_share": round(float((rec["hit"] == 1).mean()), 4)}
            if eng_noskip is not None:
                res["noskip_ms"] = round(timed(lambda: eng_noskip.poly_set_clearances(sa, sb, out_t.data_ptr(), stream=sh), args.reps), 4)
                same = out_t.cpu().numpy().view(pkg.CLEARANCE_DT).reshape(-1)
                assert same.tobytes() == rec.tobytes(), f"{res['config']}: the build without the skip writes other records"
            # the yardstick: the all-pairs list of the first rows against all of B through the distance kernel (unchanged code)
            rows = max(64, min(args.yard_rows, n_a, (1 << 26) // n_b))     # (at most 2^26 listed pairs: 2 GiB of records, 512 MiB of list)
            pairs = torch.stack([torch.arange(rows, device=dev, dtype=torch.int32).repeat_interleave(n_b),
                                 torch.arange(n_b, device=dev, dtype=torch.int32).repeat(rows)], dim=1).contiguous()
            dist_t = torch.empty((rows * n_b, 32), dtype=torch.uint8, device=dev)
            yard_ms = timed(lambda: eng.poly_pair_distances(sa, sb, pairs.data_ptr(), rows * n_b, dist_t.data_ptr(), stream=sh), args.reps)
            per_pair = yard_ms * 1e-3 / (rows * n_b)
            res["yardstick_ns_per_pair"] = round(per_pair * 1e9, 4)
            res["yardstick_pairs_per_s"] = round(1.0 / per_pair, 1)
            res["ratio"] = round(per_pair * n_a * n_b / (ms * 1e-3), 2)
            if "noskip_ms" in res:
                res["ratio_noskip"] = round(per_pair * n_a * n_b / (res["noskip_ms"] * 1e-3), 2)
            # what the skip leaves, on the host: the strips' walk in order of j over the yardstick's distances
            D = dist_t.cpu().numpy().view(pkg.DISTANCE_DT).reshape(rows, n_b)
            d2 = D["dist"].astype(F) * D["dist"].astype(F)
            hit = D["hit"] == 1
            bound = lb2(boxes(tuple(x[..., :rows] for x in a)), boxes(b))
            entered = np.zeros((rows, n_b), bool)
            per = [col_tiles // strips + (1 if s < col_tiles % strips else 0) for s in range(strips)]
            first = 0
            for tiles in per:
                j0, j1 = first * TILE_COLS, min((first + tiles) * TILE_COLS, n_b)
                first += tiles
                best = np.full(rows, np.inf, F)
                done = np.zeros(rows, bool)
                for j in range(j0, j1):
                    live = ~done
                    enter = live & ~hit[:, j] & ~(bound[:, j] > best)
                    entered[:, j] = enter
                    best = np.where(enter & (d2[:, j] < best), d2[:, j], best)
                    best = np.where(live & hit[:, j], F(0), best)
                    done |= live & (hit[:, j] | (enter & (d2[:, j] == 0)))
            res["entered_share"] = round(float(entered.mean()), 5)
            waves = entered[: rows - rows % 64].reshape(-1, 64, n_b).any(axis=1)
            res["entered_share_wave"] = round(float(waves.mean()), 5)
            print(json.dumps(res), flush=True)
            del ta, out_t, pairs, dist_t
        del tb
        torch.cuda.empty_cache()
    eng.close()
    if eng_noskip is not None:
        eng_noskip.close()


if __name__ == "__main__":
    main()
