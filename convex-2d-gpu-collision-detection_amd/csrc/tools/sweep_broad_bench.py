#!/usr/bin/env python3
"""Developer tool: the swept broad-phase polygon pair search (c2d_poly_sweep_broad_pairs) next to the static one
(c2d_sat_poly_broad_pairs: the same pipeline on boxes at rest with the pairwise test) and to the only route a caller had before it,
c2d_poly_pair_sweeps over the materialised N x M list; one JSON line per configuration, all timed in the same run.  GPU only, no
reference (tests/test_gpu_sweep_broad.py checks the lists).

Scene: poly_broad_bench.py's sparse set (K ~ U{3..16}, half axes U(0.3, 2.5), extent 200 sqrt(N / 32768)), every polygon moving by
--motion polygon sizes (a size is 3) in a random direction.  Sizes 131 072 and 10^6 (and 32 768, where the N x M list fits), each in
self (C2D_CROSS_UPPER, B = A with the same motion planes) and two-set mode.  Per configuration:
  count_ms, list_ms        the count-only call and the full list with an exact capacity: HIP events, median of --reps (>= 7)
  static_count_ms, static_list_ms, static_hits   c2d_sat_poly_broad_pairs on the same sets; list_ratio = list_ms / static_list_ms
  hits, hits_per_object, moving_share            the count; the share of the list that the static list lacks
  candidates_per_object    pairs whose SWEPT boxes overlap (tests/tools/poly_sweep_box.py), per polygon, on a sample of rows
  wild_share               polygons without a regular swept box (the pipeline's span test is not modelled)
  all_pairs_sweeps_ms      c2d_poly_pair_sweeps over all n_a x n_b pairs (n <= --all-pairs-max), hits_equal: its hits are the list
usage: sweep_broad_bench.py [--sizes 32768,131072,1000000] [--reps 7] [--motion 1.0] [--all-pairs-max 32768] [--once]"""
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
_spec = importlib.util.spec_from_file_location("poly_sweep_box", os.path.join(ROOT, "tests", "tools", "poly_sweep_box.py"))
psb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(psb)
POLYGON_SIZE = 3.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32768,131072,1000000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--motion", type=float, default=1.0, help="displacement per step in polygon sizes")
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
        motions = []
        for seed in (0x5EED1, 0x5EED2):
            ang = np.random.default_rng(seed).uniform(0, 2 * np.pi, n)
            motions.append(((args.motion * POLYGON_SIZE * np.cos(ang)).astype(np.float32), (args.motion * POLYGON_SIZE * np.sin(ang)).astype(np.float32)))
        devs = [[torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in s] for s in host]
        dmot = [[torch.from_numpy(x).to(dev) for x in m] for m in motions]
        sets = [eng.poly_set(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), n, wl.KMAX) for t in devs]
        mots = [(m[0].data_ptr(), m[1].data_ptr()) for m in dmot]
        boxed = [psb.poly_sweep_boxes(*s, m) for s, m in zip(host, motions)]
        for upper in (True, False):
            q = 0 if upper else 1
            a, b, ma, mb = sets[0], sets[q], mots[0], mots[q]

            def swept(pairs, cap):
                eng.poly_sweep_broad_pairs(a, b, pairs, cap, cnt.data_ptr(), ma, mb, upper=upper, stream=sh)

            def static(pairs, cap):
                eng.sat_poly_broad_pairs(a, b, pairs, cap, cnt.data_ptr(), upper=upper, stream=sh)

            total, static_total = counted(swept), counted(static)
            pairs = torch.empty((max(total, 1), 2), dtype=torch.int32, device=dev)
            static_pairs = torch.empty((max(static_total, 1), 2), dtype=torch.int32, device=dev)
            if args.once:
                swept(pairs.data_ptr(), total)
                stream.synchronize()
                continue
            out = {"config": f"sparse_{'self_upper' if upper else 'two_set'}", "n_a": n, "n_b": n, "extent": round(extent, 2), "motion_sizes": args.motion,
                   "count_ms": round(timed(lambda: swept(None, 0), reps), 4), "list_ms": round(timed(lambda: swept(pairs.data_ptr(), total), reps), 4),
                   "static_count_ms": round(timed(lambda: static(None, 0), reps), 4),
                   "static_list_ms": round(timed(lambda: static(static_pairs.data_ptr(), static_total), reps), 4),
                   "hits": total, "static_hits": static_total, "hits_per_object": round(total / n, 4),
                   "moving_share": round(1.0 - static_total / max(total, 1), 4), "reps": reps}
            out["list_ratio"] = round(out["list_ms"] / out["static_list_ms"], 2)
            if n <= args.all_pairs_max:
                # the route without a front end: every pair listed, every pair swept (the list and the records: 24 bytes per pair)
                rows = torch.arange(n, device=dev, dtype=torch.int32)
                allp = torch.stack([rows.repeat_interleave(n), rows.repeat(n)], dim=1).contiguous()
                rec = torch.empty((n * n, 4), dtype=torch.int32, device=dev)
                out["all_pairs_sweeps_ms"] = round(timed(lambda: eng.poly_pair_sweeps(a, b, allp.data_ptr(), n * n, rec.data_ptr(), a_motion=ma, b_motion=mb,
                                                                                      stream=sh), reps), 4)
                hit = ((rec[:, 3] >> 16) & 0xFF) == 1
                if upper:
                    hit &= allp[:, 1] > allp[:, 0]
                out["hits_equal"] = bool(torch.equal(allp[hit], pairs[:total]))
                assert out["hits_equal"], "the list differs from the hits of c2d_poly_pair_sweeps over all pairs"
                out["speedup_over_all_pairs"] = round(out["all_pairs_sweeps_ms"] / out["list_ms"], 1)
                del allp, rec, hit
            k = max(16, min(n, 2048, 200_000_000 // n))
            ba = torch.from_numpy(boxed[0][0][:, :k]).to(dev).double()
            bb = torch.from_numpy(boxed[q][0]).to(dev).double()
            meet = (ba[0][:, None] <= bb[2][None]) & (bb[0][None] <= ba[2][:, None]) & (ba[1][:, None] <= bb[3][None]) & (bb[1][None] <= ba[3][:, None])
            if upper:
                meet &= torch.arange(n, device=dev)[None] > torch.arange(k, device=dev)[:, None]
            out["candidates_per_object"] = round(float(meet.sum().item()) / k, 3)
            out["wild_share"] = round(float(1.0 - np.concatenate([boxed[0][1], boxed[q][1]]).mean()), 6)
            print(json.dumps(out), flush=True)
            del pairs, static_pairs, meet
        del devs, sets, dmot
        torch.cuda.empty_cache()
    eng.check_async()
    eng.close()


if __name__ == "__main__":
    main()
