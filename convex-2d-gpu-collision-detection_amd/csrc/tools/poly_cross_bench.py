#!/usr/bin/env python3
"""Developer tool: the all-pairs convex polygon entry points (c2d_sat_poly_cross_mask / _pairs) at N = M, K ~ U{3..16}, one JSON
line per configuration.  GPU only, no oracle (tests/test_gpu_sat_poly_cross.py checks the booleans).

Configurations: a sparse scene (centres over +-extent_sparse: below 1 % colliding) and a dense one (above 50 %), each in full
and upper (self) mode.  Per configuration:
  mask_ms                 c2d_sat_poly_cross_mask, HIP events around each call, median of --reps (>= 5) after a warm-up
  pair_tests_per_s        tested pairs / mask_ms (upper mode: n (n - 1) / 2 tested pairs)
  list_ms, list_over_mask c2d_sat_poly_cross_pairs with an exact capacity (count from the mask form), and its ratio to mask_ms
  pairwise_*              a tile of the same pairs (--tile-rows rows of A against all of B) materialised on the device in the padded
                          layout and run through c2d_sat_poly_pairs_rows: kernel time only, median of --reps after a warm-up
  speedup_vs_pairwise     pair tests/s of the mask form over those of the pairwise kernel (the condition of DESIGN.md §5.9: >= 1.0)
  valu_*                  with --counters DIR (a rocprofv3 --pmc SQ_INSTS_VALU pass of `--once`): VALU instructions per tested pair
                          and the achieved VALU lane-instr/s as a fraction of bench.py's VALU peak
usage: poly_cross_bench.py [--n 32768] [--reps 7] [--tile-rows 256] [--once] [--counters DIR]"""
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
import importlib  # noqa: E402

wl = importlib.import_module("c2d_amd.workloads")
VALU_PEAK_TLANE = 157.3 / 2   # bench.py: 10^12 VALU lane-instructions/s (FP32 peak, FMA counted as 2)
CONFIGS = [("sparse", 200.0, False), ("sparse", 200.0, True), ("dense", 0.8, False), ("dense", 0.8, True)]


def counters(d):
    """[{counter: value}] of the poly_cross_mask_kernel dispatches of a rocprofv3 counter_collection.csv, in dispatch order"""
    per = collections.defaultdict(dict)
    for f in glob.glob(os.path.join(d, "**", "*_counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "poly_cross_mask_kernel" in r["Kernel_Name"]:
                did = int(r["Dispatch_Id"])
                per[did][r["Counter_Name"]] = per[did].get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
    return [per[k] for k in sorted(per)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tile-rows", type=int, default=256)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--counters", default=None)
    args = ap.parse_args()
    n, reps = args.n, max(5, args.reps)
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    sh = stream.cuda_stream
    pmc = counters(args.counters) if args.counters else None
    words = (n + 63) // 64
    mask = torch.empty((n, words), dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)

    def timed(fn, reps):
        for _ in range(2):
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

    def device_set(extent, seed):
        return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in wl.random_convex_polygon_set(n, seed=seed, extent=extent)]

    sets, pairwise_rate = {}, {}
    for q, (name, extent, upper) in enumerate(CONFIGS):
        if name not in sets:
            sets[name] = (device_set(extent, 0xC505), device_set(extent, 0xC506))
        ta, tb = sets[name][0], sets[name][0 if upper else 1]
        a = eng.poly_set(ta[0].data_ptr(), ta[1].data_ptr(), ta[2].data_ptr(), n, wl.KMAX)
        b = eng.poly_set(tb[0].data_ptr(), tb[1].data_ptr(), tb[2].data_ptr(), n, wl.KMAX)

        def mask_call():
            eng.sat_poly_cross_mask(a, b, mask.data_ptr(), upper=upper, count=cnt.data_ptr(), stream=sh)

        if args.once:
            mask_call()
            stream.synchronize()
            continue
        tested = n * (n - 1) // 2 if upper else n * n
        mask_ms = timed(mask_call, reps)
        cnt.zero_()
        mask_call()
        stream.synchronize()
        total = int(cnt.item())
        pairs = torch.empty((max(total, 1), 2), dtype=torch.int32, device=dev)

        def list_call():
            eng.sat_poly_cross_pairs(a, b, pairs.data_ptr(), total, cnt.data_ptr(), upper=upper, stream=sh)

        list_ms = timed(list_call, 5)
        del pairs
        if name not in pairwise_rate:   # the pairwise padded kernel on a materialised tile: rows [0, tile_rows) of A x all of B
            tr = min(args.tile_rows, n)
            m = tr * n
            sa, sb = sets[name]
            vx = torch.stack([sa[0][:, :tr].repeat_interleave(n, dim=1), sb[0].repeat(1, tr)]).contiguous()
            vy = torch.stack([sa[1][:, :tr].repeat_interleave(n, dim=1), sb[1].repeat(1, tr)]).contiguous()
            kk = torch.stack([sa[2][:tr].repeat_interleave(n), sb[2].repeat(tr)]).contiguous()
            out = torch.empty(m, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            ms = timed(lambda: eng.sat_poly_pairs_rows(vx.data_ptr(), vy.data_ptr(), kk.data_ptr(), m, wl.KMAX, out.data_ptr(), None, stream=sh), reps)
            pairwise_rate[name] = (m / (ms * 1e-3), float(out.float().mean().item()), m)
            del vx, vy, kk, out
        rate, tile_frac, tile_pairs = pairwise_rate[name]
        rec = {"config": f"{name}_{'upper' if upper else 'full'}", "n_a": n, "n_b": n, "extent": extent, "tested_pairs": tested,
               "colliding": total, "collide_frac": round(total / tested, 6), "mask_ms": round(mask_ms, 4),
               "pair_tests_per_s": float(f"{tested / (mask_ms * 1e-3):.4g}"), "list_ms": round(list_ms, 4),
               "list_over_mask": round(list_ms / mask_ms, 3), "pairwise_tile_pairs": tile_pairs, "pairwise_tile_collide_frac": round(tile_frac, 6),
               "pairwise_pair_tests_per_s": float(f"{rate:.4g}"), "speedup_vs_pairwise": round(tested / (mask_ms * 1e-3) / rate, 2), "reps": reps}
        if pmc is not None and q < len(pmc):
            valu = pmc[q].get("SQ_INSTS_VALU")
            if valu:
                lane = valu * 64 / (mask_ms * 1e-3) / 1e12
                rec.update({"valu_instr_per_pair": round(valu * 64 / tested, 1), "valu_tlane_per_s": round(lane, 2),
                            "valu_frac": round(lane / VALU_PEAK_TLANE, 4), "valu_peak_tlane": VALU_PEAK_TLANE})
            for key in ("SQ_INSTS_LDS", "SQ_LDS_BANK_CONFLICT", "SQ_WAVES"):
                if key in pmc[q]:
                    rec[key] = pmc[q][key]
        print(json.dumps(rec), flush=True)
    eng.check_async()
    eng.close()


if __name__ == "__main__":
    main()
