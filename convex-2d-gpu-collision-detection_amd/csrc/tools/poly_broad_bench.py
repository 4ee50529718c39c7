#!/usr/bin/env python3
"""Developer tool: the broad-phase polygon pair search (c2d_sat_poly_broad_pairs) against the N x M list
(c2d_sat_poly_cross_pairs) on the polygon cross bench's sparse scene, one JSON line per configuration.  GPU only, no oracle
(tests/test_gpu_sat_poly_broad.py checks the lists).

Scene: poly_cross_bench.py's sparse set (K ~ U{3..16}, half axes U(0.3, 2.5)) with its extent 200 scaled by sqrt(N / 32768), so that
the hits per polygon stay constant.  Sizes 32 768, 131 072 and 10^6, each in self (C2D_CROSS_UPPER, B = A) and two-set mode.  Per
configuration:
  count_ms        the count-only call (capacity 0), HIP events, median of --reps (>= 7) after a warm-up
  list_ms         the full list with an exact capacity
  hits            the count; hits_per_object = hits / n_a
  candidates_per_object   pairs whose conservative boxes overlap (the rule of DESIGN.md §5.10, restated in numpy by
                  tests/tools/poly_broad_box.py), per polygon, on a sample of rows: the exact tests of the short path
  cross_ms        c2d_sat_poly_cross_pairs on the same input (exact capacity), where it runs in reasonable time (n <= --cross-max)
  speedup         cross_ms / list_ms; lists_equal: the two lists compared on the device
The share of each phase comes from a separate run under `rocprofv3 --kernel-trace --stats -- python3 poly_broad_bench.py --once`.
usage: poly_broad_bench.py [--sizes 32768,131072,1000000] [--reps 7] [--cross-max 131072] [--once] [--density D]"""
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
_spec = importlib.util.spec_from_file_location("poly_broad_box", os.path.join(ROOT, "tests", "tools", "poly_broad_box.py"))
pbb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pbb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32768,131072,1000000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cross-max", type=int, default=131072)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--density", type=float, default=1.0, help="divide the extent by this (hits per object grow with its square)")
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

    for n in [int(x) for x in args.sizes.split(",")]:
        extent = 200.0 * np.sqrt(n / 32768) / args.density
        host = [wl.random_convex_polygon_set(n, seed=seed, extent=extent) for seed in (0xC505, 0xC506)]
        devs = [[torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in s] for s in host]
        sets = [eng.poly_set(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), n, wl.KMAX) for t in devs]
        boxes = [pbb.poly_broad_boxes(*s)[0] for s in host]
        for upper in (True, False):
            a, b = sets[0], sets[0 if upper else 1]
            cnt.zero_()
            eng.sat_poly_broad_pairs(a, b, None, 0, cnt.data_ptr(), upper=upper, stream=sh)
            stream.synchronize()
            total = int(cnt.item())
            pairs = torch.empty((max(total, 1), 2), dtype=torch.int32, device=dev)

            def count_call():
                eng.sat_poly_broad_pairs(a, b, None, 0, cnt.data_ptr(), upper=upper, stream=sh)

            def list_call():
                eng.sat_poly_broad_pairs(a, b, pairs.data_ptr(), total, cnt.data_ptr(), upper=upper, stream=sh)

            if args.once:
                list_call()
                stream.synchronize()
                continue
            scene = "sparse" if args.density == 1.0 else f"density{args.density:g}"
            out = {"config": f"{scene}_{'self_upper' if upper else 'two_set'}", "n_a": n, "n_b": n, "extent": round(extent, 2),
                   "count_ms": round(timed(count_call, reps), 4), "list_ms": round(timed(list_call, reps), 4),
                   "hits": total, "hits_per_object": round(total / n, 4), "reps": reps}
            if n <= args.cross_max:
                cross_pairs = torch.empty((max(total, 1), 2), dtype=torch.int32, device=dev)

                def cross_call():
                    eng.sat_poly_cross_pairs(a, b, cross_pairs.data_ptr(), total, cnt.data_ptr(), upper=upper, stream=sh)

                out["cross_ms"] = round(timed(cross_call, reps), 4)
                out["speedup"] = round(out["cross_ms"] / out["list_ms"], 1)
                out["lists_equal"] = bool(torch.equal(cross_pairs[:total], pairs[:total]))
                assert out["lists_equal"], "the broad list differs from the cross list"
                del cross_pairs
            # candidates: the conservative boxes of a sample of rows against all of B's (wild polygons have NaN boxes: left out)
            k = max(16, min(n, 2048, 200_000_000 // n))
            ba = torch.from_numpy(boxes[0][:, :k]).to(dev).double()
            bb = torch.from_numpy(boxes[0 if upper else 1]).to(dev).double()
            meet = (ba[0][:, None] <= bb[2][None]) & (bb[0][None] <= ba[2][:, None]) & (ba[1][:, None] <= bb[3][None]) & (bb[1][None] <= ba[3][:, None])
            if upper:
                meet &= torch.arange(n, device=dev)[None] > torch.arange(k, device=dev)[:, None]
            out["candidates_per_object"] = round(float(meet.sum().item()) / k, 3)
            print(json.dumps(out), flush=True)
            del pairs, meet
        del devs, sets
        torch.cuda.empty_cache()
    eng.check_async()
    eng.close()


if __name__ == "__main__":
    main()
