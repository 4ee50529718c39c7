#!/usr/bin/env python3
"""Developer tool: the grid shape cast (c2d_poly_set_casts_grid) next to the two ways the library had to answer "which obstacle does
each moving footprint touch first" before it, both on unchanged code and timed in the same process:
  nxm     c2d_poly_set_casts on the same sets and motions (all n_a x n_b pairs; where n_a * n_b <= --nxm-max-pairs).  Wherever it
          runs, the grid call's bytes must equal its bytes: the tool asserts it;
  chain   c2d_poly_sweep_broad_pairs (count, then the list at its exact capacity) followed by c2d_poly_pair_sweeps on the device
          count: every pair that touches with its record, the per-row minimum left to the caller and not counted.
One JSON line per configuration, then the same as a markdown table.  GPU only, no reference (tests/test_gpu_casts_grid.py checks the
records).

Scene: csrc/tools/cast_bench.py's generator (workloads.random_convex_polygon_set: K ~ U{3..16}, half axes 0.3 .. 2.5, extent
200 * sqrt(N / 32768), N the number of obstacles, queries and obstacles in the same box), every polygon of both sets moving by up to
+- m per component, m = --motions polygon sizes (a size is 3).  Shapes n_a x n_b: 131072 x 4096, 4096 x 131072, 131072 x 131072 and
131072 x 1048576, the queries as generated (unsorted) and sorted along a Morton curve over their first vertices.  Per configuration:
  grid_ms, nxm_ms, chain_ms     HIP events around the call(s), median of --reps (>= 7) after a warm-up
  miss_share, start_share, moving_share   the shares of queries that touch nothing, start in overlap, are first touched at t > 0
  listed, walked, candidates, walks       c2d_poly_set_casts_grid_stats, the last three per query: sorted grid entries a walk looked
                                at; candidates (swept boxes meet, or wild); pairs that ran the axis walk
  chain_pairs                   pairs per query in the chain's list
usage: cast_grid_bench.py [--shapes 131072x4096,...] [--reps 7] [--motions 0.1,1,3] [--nxm-max-pairs 34359738368]"""
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
POLYGON_SIZE = 3.0
COLUMNS = ["config", "motion_sizes", "grid_ms", "nxm_ms", "chain_ms", "miss_share", "start_share", "moving_share", "listed", "walked", "candidates", "walks",
           "chain_pairs"]


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
    ap.add_argument("--shapes", default="131072x4096,4096x131072,131072x131072,131072x1048576")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--motions", default="0.1,1,3", help="the largest motion per component, in polygon sizes")
    ap.add_argument("--nxm-max-pairs", type=int, default=1 << 35)
    args = ap.parse_args()
    reps = max(7, args.reps)
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    sh = stream.cuda_stream
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    size = pkg.CAST_DT.itemsize
    rows = []

    def timed(fn):
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

    def upload(s):
        t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in s]
        return t, eng.poly_set(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), s[0].shape[1], wl.KMAX)

    def upload_motion(unit, reach):
        t = [torch.from_numpy(np.ascontiguousarray((u * F(reach)).astype(F))).to(dev) for u in unit]
        return t, (t[0].data_ptr(), t[1].data_ptr())

    for shape in args.shapes.split(","):
        n_a, n_b = (int(v) for v in shape.split("x"))
        extent = 200.0 * np.sqrt(n_b / 32768)
        a0 = wl.random_convex_polygon_set(n_a, seed=0xCA57, extent=extent)
        b = wl.random_convex_polygon_set(n_b, seed=0xCA58, extent=extent)
        rng = np.random.default_rng(0xCA59)
        ua0, ub = (tuple(rng.uniform(-1, 1, n).astype(F) for _ in range(2)) for n in (n_a, n_b))      # the motions in units of the reach
        tb, sb = upload(b)
        for order in ("unsorted", "sorted"):
            perm = np.arange(n_a) if order == "unsorted" else morton_order(a0)
            a, ua = tuple(np.ascontiguousarray(x[..., perm]) for x in a0), tuple(np.ascontiguousarray(u[perm]) for u in ua0)
            ta, sa = upload(a)
            out_t = torch.empty((n_a, size), dtype=torch.uint8, device=dev)
            full_t = torch.empty((n_a, size), dtype=torch.uint8, device=dev)
            for rel in [float(x) for x in args.motions.split(",")]:
                reach = rel * POLYGON_SIZE
                tma, pa = upload_motion(ua, reach)
                tmb, pb = upload_motion(ub, reach)
                res = {"config": f"{n_a}x{n_b}_{order}", "n_a": n_a, "n_b": n_b, "extent": round(float(extent), 2), "motion_sizes": rel, "reps": reps}
                res["grid_ms"] = round(timed(lambda: eng.poly_set_casts_grid(sa, sb, pa, pb, 0, 0, 0, out_t.data_ptr(), sh)), 4)
                st = eng.poly_set_casts_grid_stats()
                rec = out_t.cpu().numpy().view(pkg.CAST_DT).reshape(-1)
                hit = rec["hit"] == 1
                res["nxm_ms"] = None
                if n_a * n_b <= args.nxm_max_pairs:
                    res["nxm_ms"] = round(timed(lambda: eng.poly_set_casts(sa, sb, pa, pb, 0, 0, 0, full_t.data_ptr(), sh)), 4)
                    assert full_t.cpu().numpy().tobytes() == rec.tobytes(), f"{res['config']}, motion {rel}: the bytes differ from c2d_poly_set_casts'"
                    res["equals_nxm"] = True
                res["miss_share"] = round(float((~hit).mean()), 4)
                res["start_share"] = round(float((hit & (rec["toi"] == 0)).mean()), 4)
                res["moving_share"] = round(float((hit & (rec["toi"] > 0)).mean()), 4)
                res["listed"] = st["listed"]
                for key in ("walked", "candidates", "walks"):
                    res[key] = round(st[key] / n_a, 2)
                # the chain: count, then the list at its exact capacity and the records on the device count
                cnt.zero_()
                eng.poly_sweep_broad_pairs(sa, sb, None, 0, cnt.data_ptr(), pa, pb, stream=sh)
                stream.synchronize()
                total = int(cnt.item())
                pairs = torch.empty((max(total, 1), 2), dtype=torch.int32, device=dev)
                sweep_t = torch.empty((max(total, 1), pkg.SWEEP_DT.itemsize), dtype=torch.uint8, device=dev)

                def chain():
                    cnt.zero_()
                    eng.poly_sweep_broad_pairs(sa, sb, pairs.data_ptr(), total, cnt.data_ptr(), pa, pb, stream=sh)
                    eng.poly_pair_sweeps(sa, sb, pairs.data_ptr(), total, sweep_t.data_ptr(), a_motion=pa, b_motion=pb, n_pairs_dev=cnt.data_ptr(), stream=sh)

                res["chain_ms"] = round(timed(chain), 4)
                res["chain_pairs"] = round(total / n_a, 2)
                print(json.dumps(res), flush=True)
                rows.append(res)
                del pairs, sweep_t, tma, tmb
            del ta, out_t, full_t
            torch.cuda.empty_cache()
        del tb
        torch.cuda.empty_cache()
    eng.check_async()
    eng.close()
    print("\n| " + " | ".join(COLUMNS) + " |\n|" + "---|" * len(COLUMNS))
    for r in rows:
        print("| " + " | ".join("–" if r.get(c) is None else str(r[c]) for c in COLUMNS) + " |")


if __name__ == "__main__":
    main()
