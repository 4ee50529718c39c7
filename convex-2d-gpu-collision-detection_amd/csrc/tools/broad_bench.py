#!/usr/bin/env python3
"""Developer tool: the broad-phase pair search (c2d_sat_rect_broad_pairs) against the N x M list (c2d_sat_rect_cross_pairs) on
the cross bench's sparse scene, one JSON line per configuration.  GPU only, no oracle (tests/test_gpu_sat_broad.py checks the
lists).

Scene: cross_bench.py's sparse set (sizes U(0.1, 5), any angle) with its extent 400 scaled by sqrt(N / 32768), so that the hits per
object stay constant.  Sizes 32 768, 131 072, 10^6 and 10^7, each in self (C2D_CROSS_UPPER, B = A) and two-set mode.  Per
configuration:
  count_ms        the count-only call (capacity 0), HIP events, median of --reps after a warm-up
  list_ms         the full list with an exact capacity
  hits            the count; hits_per_object = hits / n_a
  candidates_per_object   pairs whose vertex boxes overlap, per object, on a sample of rows: about the exact tests the short
                  path makes (its conservative boxes are a few ulps wider)
  cross_ms        c2d_sat_rect_cross_pairs on the same input (exact capacity), where it runs in seconds (n <= --cross-max)
  speedup         cross_ms / list_ms
The share of each phase comes from a separate run under `rocprofv3 --kernel-trace --stats -- python3 broad_bench.py --once`:
each configuration's list call once, so the trace's per-kernel totals split one call of every configuration.
--density D divides the extent by D: hits per object grow by D^2 (D = 4: about 12 per object in self mode, 24 in two-set mode).
usage: broad_bench.py [--sizes 32768,131072,1000000,10000000] [--reps 10] [--cross-max 131072] [--once] [--density D]"""
import argparse
import json
import os
import sys

import torch  # before libc2d.so
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32768,131072,1000000,10000000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cross-max", type=int, default=131072)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--density", type=float, default=1.0, help="divide the extent by this (hits per object grow with its square)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    sh = stream.cuda_stream
    row = lambda t, k: t.data_ptr() + k * t.stride(0) * t.element_size()  # noqa: E731
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)

    def rects(n, extent, seed):
        gen = torch.Generator(device=dev)
        gen.manual_seed(seed)
        pose = torch.empty((5, n), dtype=torch.float32, device=dev)
        pose[0].uniform_(-extent, extent, generator=gen)
        pose[1].uniform_(-extent, extent, generator=gen)
        pose[2].uniform_(0.1, 5.0, generator=gen)
        pose[3].uniform_(0.1, 5.0, generator=gen)
        pose[4].uniform_(0.0, 2.0 * np.pi, generator=gen)
        planes = torch.empty((8, n), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        eng.rects_from_poses(*[row(pose, k) for k in range(5)], n, [row(planes, k) for k in range(8)], stream=sh)
        stream.synchronize()
        return planes

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
        extent = 400.0 * np.sqrt(n / 32768) / args.density
        a, b = rects(n, extent, 0xB0A1), rects(n, extent, 0xB0A2)
        for upper in (True, False):
            pa = [row(a, q) for q in range(8)]
            pb = pa if upper else [row(b, q) for q in range(8)]
            cnt.zero_()
            eng.sat_rect_broad_pairs(pa, n, pb, n, None, 0, cnt.data_ptr(), upper=upper, stream=sh)
            stream.synchronize()
            total = int(cnt.item())
            pairs = torch.empty((max(total, 1), 2), dtype=torch.int32, device=dev)

            def count_call():
                eng.sat_rect_broad_pairs(pa, n, pb, n, None, 0, cnt.data_ptr(), upper=upper, stream=sh)

            def list_call():
                eng.sat_rect_broad_pairs(pa, n, pb, n, pairs.data_ptr(), total, cnt.data_ptr(), upper=upper, stream=sh)

            if args.once:
                list_call()
                stream.synchronize()
                continue
            scene = "sparse" if args.density == 1.0 else f"density{args.density:g}"
            out = {"config": f"{scene}_{'self_upper' if upper else 'two_set'}", "n_a": n, "n_b": n, "extent": round(extent, 2),
                   "count_ms": round(timed(count_call, args.reps), 4), "list_ms": round(timed(list_call, args.reps), 4),
                   "hits": total, "hits_per_object": round(total / n, 4)}
            if n <= args.cross_max:
                cross_pairs = torch.empty((max(total, 1), 2), dtype=torch.int32, device=dev)

                def cross_call():
                    eng.sat_rect_cross_pairs(pa, n, pb, n, cross_pairs.data_ptr(), total, cnt.data_ptr(), upper=upper, stream=sh)

                out["cross_ms"] = round(timed(cross_call, max(2, args.reps // 4)), 4)
                out["speedup"] = round(out["cross_ms"] / out["list_ms"], 1)
                out["lists_equal"] = bool(torch.equal(cross_pairs[:total], pairs[:total]))
                del cross_pairs
            # candidates: boxes of the sample rows against all of B (the device's grid adds none: it only narrows the search)
            k = max(16, min(n, 2048, 200_000_000 // n))
            aa = a[:, :k].double()
            bb = (a if upper else b).double()

            def boxes(r):
                x, y = r[0::2], r[1::2]
                return x.min(0).values, y.min(0).values, x.max(0).values, y.max(0).values

            ax0, ay0, ax1, ay1 = boxes(aa)
            bx0, by0, bx1, by1 = boxes(bb)
            meet = (ax0[:, None] <= bx1[None]) & (bx0[None] <= ax1[:, None]) & (ay0[:, None] <= by1[None]) & (by0[None] <= ay1[:, None])
            if upper:
                meet &= torch.arange(n, device=dev)[None] > torch.arange(k, device=dev)[:, None]
            out["candidates_per_object"] = round(float(meet.sum().item()) / k, 3)
            print(json.dumps(out), flush=True)
            del pairs, meet
        del a, b
        torch.cuda.empty_cache()
    eng.close()


if __name__ == "__main__":
    main()
