#!/usr/bin/env python3
"""Developer tool: the all-pairs rectangle entry points (c2d_sat_rect_cross_mask / _pairs) at N = M, one JSON line per
configuration.  GPU only, no oracle (tests/test_gpu_sat_cross.py checks the booleans).

Configurations: a sparse set (centres over +-extent_sparse: a broad-phase-like rate, well below 1 %) and a dense one
(the bench workload's extent 8: about 13 %), each in full and upper (self) mode.  Per configuration:
  mask_ms                 c2d_sat_rect_cross_mask, HIP events around each call, median of --reps after a warm-up
  pair_tests_per_s        tested pairs / mask_ms (upper mode: n (n - 1) / 2 tested pairs)
  list_ms, list_over_mask c2d_sat_rect_cross_pairs with an exact capacity (count from the mask form), and its ratio to mask_ms
  pairwise_*              the same pairs materialised on the device in chunks of rows and run through c2d_sat_rect_pairs_verts_mask
                          (kernel time only, summed over the chunks); upper mode: the full rate applied to the tested pairs
  valu_*                  with --counters DIR (a rocprofv3 --pmc SQ_INSTS_VALU ... pass of `--once`): VALU instructions per tested
                          pair and the achieved VALU lane-instr/s as a fraction of bench.py's VALU_PEAK_TLANE
usage: cross_bench.py [--n 32768] [--reps 20] [--once] [--counters DIR]
       --once: each configuration's mask call once and nothing else of this library's N x M kernel (the PMC pass: the i-th
       cross_mask_kernel dispatch is configuration i)"""
import argparse
import collections
import csv
import glob
import json
import os
import sys

import torch  # before libc2d.so
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
VALU_PEAK_TLANE = 157.3 / 2   # bench.py: 10^12 VALU lane-instructions/s (FP32 peak, FMA counted as 2)
CONFIGS = [("sparse", 400.0, False), ("sparse", 400.0, True), ("dense", 8.0, False), ("dense", 8.0, True)]


def counters(d):
    """{dispatch order among cross_mask_kernel dispatches: {counter: value}} from a rocprofv3 counter_collection.csv"""
    per = collections.defaultdict(dict)
    for f in glob.glob(os.path.join(d, "**", "*_counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "cross_mask_kernel" in r["Kernel_Name"]:
                did = int(r["Dispatch_Id"])
                per[did][r["Counter_Name"]] = per[did].get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
    return [per[k] for k in sorted(per)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--counters", default=None)
    args = ap.parse_args()
    n = args.n
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    sh = stream.cuda_stream
    row = lambda t, k: t.data_ptr() + k * t.stride(0) * t.element_size()  # noqa: E731
    pmc = counters(args.counters) if args.counters else None
    words = (n + 63) // 64
    mask = torch.empty((n, words), dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)

    def rects(extent, seed):
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
        for _ in range(3):
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

    sets = {}
    pairwise_rate = {}
    for k, (name, extent, upper) in enumerate(CONFIGS):
        if name not in sets:
            sets[name] = (rects(extent, 0xC505), rects(extent, 0xC506))
        a, b = sets[name]
        pa, pb = [row(a, q) for q in range(8)], [row(b if not upper else a, q) for q in range(8)]

        def mask_call():
            eng.sat_rect_cross_mask(pa, n, pb, n, mask.data_ptr(), upper=upper, count=cnt.data_ptr(), stream=sh)

        if args.once:
            mask_call()
            stream.synchronize()
            continue
        tested = n * (n - 1) // 2 if upper else n * n
        mask_ms = timed(mask_call, args.reps)
        cnt.zero_()
        mask_call()
        stream.synchronize()
        total = int(cnt.item())
        pairs = torch.empty((max(total, 1), 2), dtype=torch.int32, device=dev)

        def list_call():
            eng.sat_rect_cross_pairs(pa, n, pb, n, pairs.data_ptr(), total, cnt.data_ptr(), upper=upper, stream=sh)

        list_ms = timed(list_call, max(3, args.reps // 4))
        if name not in pairwise_rate:   # materialise-then-pairwise on the full N x M of this set
            rows_per = max(1, (1 << 25) // n)
            p16 = torch.empty((16, rows_per * n), dtype=torch.float32, device=dev)
            m16 = torch.empty(((rows_per * n + 63) // 64,), dtype=torch.int64, device=dev)
            kern_ms = 0.0
            for r0 in range(-rows_per, n, rows_per):   # (the first chunk is a warm-up)
                rr = range(max(r0, 0), min(n, max(r0, 0) + rows_per))
                m = len(rr) * n
                p16[:8, :m] = a[:, rr.start:rr.stop].repeat_interleave(n, dim=1)
                p16[8:, :m] = (b if not upper else a).repeat(1, len(rr))
                torch.cuda.current_stream(dev).synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                eng.sat_rect_pairs_verts_mask([row(p16, q) for q in range(16)], m, m16.data_ptr(), None, stream=sh)
                e1.record(stream)
                stream.synchronize()
                if r0 >= 0:
                    kern_ms += e0.elapsed_time(e1)
            pairwise_rate[name] = n * n / (kern_ms * 1e-3)
            del p16, m16
        out = {"config": f"{name}_{'upper' if upper else 'full'}", "n_a": n, "n_b": n, "extent": extent, "tested_pairs": tested,
               "colliding": total, "collide_frac": round(total / tested, 6), "mask_ms": round(mask_ms, 4),
               "pair_tests_per_s": float(f"{tested / (mask_ms * 1e-3):.4g}"), "list_ms": round(list_ms, 4),
               "list_over_mask": round(list_ms / mask_ms, 3), "pairwise_pair_tests_per_s": float(f"{pairwise_rate[name]:.4g}"),
               "pairwise_ms": round(tested / pairwise_rate[name] * 1e3, 4),
               "speedup_vs_pairwise": round(tested / pairwise_rate[name] * 1e3 / mask_ms, 2)}
        if pmc is not None and k < len(pmc):
            c = pmc[k]
            valu = c.get("SQ_INSTS_VALU")
            if valu:
                lane = valu * 64 / (mask_ms * 1e-3) / 1e12
                out.update({"valu_instr_per_pair": round(valu * 64 / tested, 1), "valu_tlane_per_s": round(lane, 2),
                            "valu_frac": round(lane / VALU_PEAK_TLANE, 4), "valu_peak_tlane": VALU_PEAK_TLANE})
            for key in ("SQ_INSTS_LDS", "SQ_LDS_BANK_CONFLICT", "SQ_WAVES"):
                if key in c:
                    out[key] = c[key]
        print(json.dumps(out), flush=True)
        del pairs
    eng.close()


if __name__ == "__main__":
    main()
