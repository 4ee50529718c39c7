#!/usr/bin/env python3
"""Developer tool: the proximity pair search (c2d_poly_near_broad_pairs) next to the static broad phase (c2d_sat_poly_broad_pairs: the
same pipeline on boxes without a margin, with the pairwise test alone) and to the only route a caller had before it,
c2d_poly_pair_distances over the materialised N x M list; one JSON line per configuration, all timed in the same run.  GPU only, no
reference (tests/test_gpu_near_broad.py checks the lists).

Scene: poly_broad_bench.py's sparse set (K ~ U{3..16}, half axes U(0.3, 2.5), extent 200 sqrt(N / 32768)).  Sizes 32 768 (where the
N x M list fits), 131 072 and 10^6, each in self (C2D_CROSS_UPPER, B = A) and two-set mode, at margins of --margins polygon sizes (a
size is 3).  Per configuration:
  count_ms, list_ms        the count-only call and the full list with an exact capacity: HIP events, median of --reps (>= 7)
  static_count_ms, static_list_ms, static_hits   c2d_sat_poly_broad_pairs on the same sets; list_ratio = list_ms / static_list_ms
  pairs, pairs_per_object, separated_share       the count; the share of the list that is not hit (that the static list lacks)
  candidates_per_object    pairs whose boxes under the margin overlap (tests/tools/poly_near_box.py), per polygon, on a sample of rows
  wild_share               polygons without a regular box (the pipeline's span test is not modelled)
  all_pairs_distances_ms   c2d_poly_pair_distances over all n_a x n_b pairs (n <= --all-pairs-max), pairs_equal: its hit | dist <= margin
                           entries are the list; speedup_over_all_pairs = all_pairs_distances_ms / list_ms
usage: near_broad_bench.py [--sizes 32768,131072,1000000] [--reps 7] [--margins 0,0.1,1] [--all-pairs-max 32768] [--once]"""
import argparse
import importlib
import importlib.util
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
_spec = importlib.util.spec_from_file_location("poly_near_box", os.path.join(ROOT, "tests", "tools", "poly_near_box.py"))
pnb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pnb)
POLYGON_SIZE = 3.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32768,131072,1000000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--margins", default="0,0.1,1", help="margins in polygon sizes")
    ap.add_argument("--all-pairs-max", type=int, default=32768)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    reps = max(7, args.reps)
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    sh = stream.cuda_stream
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)

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

    def counted(call):
        cnt.zero_()
        call(None, 0)
        stream.synchronize()
        return int(cnt.item())

    for n in [int(x) for x in args.sizes.split(",")]:
        extent = 200.0 * np.sqrt(n / 32768)
        host = [wl.random_convex_polygon_set(n, seed=seed, extent=extent) for seed in (0xC505, 0xC506)]
        devs = [[torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in s] for s in host]
        sets = [eng.poly_set(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), n, wl.KMAX) for t in devs]
        for upper in (True, False):
            q = 0 if upper else 1
            a, b = sets[0], sets[q]

            def static(pairs, cap):
                eng.sat_poly_broad_pairs(a, b, pairs, cap, cnt.data_ptr(), upper=upper, stream=sh)

            static_total = counted(static)
            static_pairs = torch.empty((max(static_total, 1), 2), dtype=torch.int32, device=dev)
            static_ms = None
            allp = rec = None
            for rel in [float(x) for x in args.margins.split(",")]:
                margin = float(np.float32(rel * POLYGON_SIZE))

                def near(pairs, cap):
                    eng.poly_near_broad_pairs(a, b, margin, pairs, cap, cnt.data_ptr(), upper=upper, stream=sh)

                total = counted(near)
                pairs = torch.empty((max(total, 1), 2), dtype=torch.int32, device=dev)
                if args.once:
                    near(pairs.data_ptr(), total)
                    stream.synchronize()
                    continue
                if static_ms is None:
                    static_ms = (round(timed(lambda: static(None, 0), reps), 4), round(timed(lambda: static(static_pairs.data_ptr(), static_total), reps), 4))
                out = {"config": f"sparse_{'self_upper' if upper else 'two_set'}", "n_a": n, "n_b": n, "extent": round(extent, 2), "margin_sizes": rel,
                       "count_ms": round(timed(lambda: near(None, 0), reps), 4), "list_ms": round(timed(lambda: near(pairs.data_ptr(), total), reps), 4),
                       "static_count_ms": static_ms[0], "static_list_ms": static_ms[1],
                       "pairs": total, "static_hits": static_total, "pairs_per_object": round(total / n, 4),
                       "separated_share": round(1.0 - static_total / max(total, 1), 4), "reps": reps}
                out["list_ratio"] = round(out["list_ms"] / out["static_list_ms"], 2)
                if n <= args.all_pairs_max:
                    # the route without a front end: every pair listed, every pair measured (the list and the records: 40 bytes per pair)
                    if allp is None:
                        rows = torch.arange(n, device=dev, dtype=torch.int32)
                        allp = torch.stack([rows.repeat_interleave(n), rows.repeat(n)], dim=1).contiguous()
                        rec = torch.empty((n * n, 8), dtype=torch.int32, device=dev)
                        out["all_pairs_distances_ms"] = all_ms = round(timed(lambda: eng.poly_pair_distances(a, b, allp.data_ptr(), n * n, rec.data_ptr(), stream=sh), reps), 4)
                    else:
                        out["all_pairs_distances_ms"] = all_ms
                    keep = ((rec[:, 6] & 0xFF) == 1) | (rec[:, 0].view(torch.float32) <= margin)
                    if upper:
                        keep &= allp[:, 1] > allp[:, 0]
                    out["pairs_equal"] = bool(torch.equal(allp[keep], pairs[:total]))
                    assert out["pairs_equal"], "the list differs from hit | dist <= margin of c2d_poly_pair_distances over all pairs"
                    out["speedup_over_all_pairs"] = round(all_ms / out["list_ms"], 1)
                    del keep
                boxed = [pnb.poly_near_boxes(*host[0], margin), pnb.poly_near_boxes(*host[q], margin)]
                k = max(16, min(n, 2048, 200_000_000 // n))
                ba = torch.from_numpy(boxed[0][0][:, :k]).to(dev).double()
                bb = torch.from_numpy(boxed[1][0]).to(dev).double()
                meet = (ba[0][:, None] <= bb[2][None]) & (bb[0][None] <= ba[2][:, None]) & (ba[1][:, None] <= bb[3][None]) & (bb[1][None] <= ba[3][:, None])
                if upper:
                    meet &= torch.arange(n, device=dev)[None] > torch.arange(k, device=dev)[:, None]
                out["candidates_per_object"] = round(float(meet.sum().item()) / k, 3)
                out["wild_share"] = round(float(1.0 - np.concatenate([boxed[0][1], boxed[1][1]]).mean()), 6)
                print(json.dumps(out), flush=True)
                del pairs, meet
            del static_pairs, allp, rec
            torch.cuda.empty_cache()
        del devs, sets
        torch.cuda.empty_cache()
    eng.check_async()
    eng.close()


if __name__ == "__main__":
    main()
