#!/usr/bin/env python3
"""Developer tool: the grid clearance query (c2d_poly_set_clearances_grid) next to the two ways the library had to answer "the nearest
obstacle within a margin" before it, both on unchanged code and timed in the same process:
  nxm     c2d_poly_set_clearances on the same sets (all n_a x n_b pairs; where n_a * n_b <= --nxm-max-pairs), which needs no margin and
          finds the nearest obstacle however far it is;
  chain   c2d_poly_near_broad_pairs at the same margin (count, then the list at its exact capacity) followed by
          c2d_poly_pair_distances on the device count: every pair within the margin with its record, the per-row minimum left to the
          caller and not counted.
One JSON line per configuration, then the same as a markdown table.  GPU only, no reference (tests/test_gpu_clearances_grid.py checks
the records); where every query has a winner the records are compared with c2d_poly_set_clearances' bytes.

Scene: the sparse generator (workloads.random_convex_polygon_set: K ~ U{3..16}, half axes 0.3 .. 2.5) with extent
200 * sqrt(N / 32768), N the number of obstacles, queries and obstacles in the same box (csrc/tools/clearance_bench.py's).  Shapes
n_a x n_b: 131072 x 4096, 4096 x 131072, 131072 x 131072 and 131072 x 1048576, the queries as generated (unsorted) and sorted along
a Morton curve over their first vertices; margins of --margins polygon sizes (a size is 3).  Per configuration:
  grid_ms, nxm_ms, chain_ms     HIP events around the call(s), median of --reps (>= 7) after a warm-up
  none_share                    the share of queries that get the NONE record; hit_share: of queries whose winner is hit
  listed, walked, candidates, tested, walks   c2d_poly_set_clearances_grid_stats, the last four per query: sorted grid entries a walk
                                looked at; candidates (boxes meet, or wild); pairs that ran the pairwise test; pairs that ran the
                                candidate walk of the distance rule
  chain_pairs                   pairs per query in the chain's list
usage: clearance_grid_bench.py [--shapes 131072x4096,...] [--reps 7] [--margins 0.1,1,3] [--nxm-max-pairs 34359738368]"""
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
POLYGON_SIZE = 3.0
COLUMNS = ["config", "margin_sizes", "grid_ms", "nxm_ms", "chain_ms", "none_share", "hit_share", "listed", "walked", "candidates", "tested", "walks", "chain_pairs"]


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
    ap.add_argument("--margins", default="0.1,1,3", help="margins in polygon sizes")
    ap.add_argument("--nxm-max-pairs", type=int, default=1 << 35)
    args = ap.parse_args()
    reps = max(7, args.reps)
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    sh = stream.cuda_stream
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
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

    for shape in args.shapes.split(","):
        n_a, n_b = (int(v) for v in shape.split("x"))
        extent = 200.0 * np.sqrt(n_b / 32768)
        a0 = wl.random_convex_polygon_set(n_a, seed=0xC1EA, extent=extent)
        b = wl.random_convex_polygon_set(n_b, seed=0xC1EB, extent=extent)
        tb, sb = upload(b)
        for order in ("unsorted", "sorted"):
            a = a0 if order == "unsorted" else tuple(np.ascontiguousarray(x[..., morton_order(a0)]) for x in a0)
            ta, sa = upload(a)
            out_t = torch.empty((n_a, 32), dtype=torch.uint8, device=dev)
            full_t = torch.empty((n_a, 32), dtype=torch.uint8, device=dev)
            nxm_ms = None
            if n_a * n_b <= args.nxm_max_pairs:
                nxm_ms = round(timed(lambda: eng.poly_set_clearances(sa, sb, full_t.data_ptr(), stream=sh)), 4)
            for rel in [float(x) for x in args.margins.split(",")]:
                margin = float(np.float32(rel * POLYGON_SIZE))
                res = {"config": f"{n_a}x{n_b}_{order}", "n_a": n_a, "n_b": n_b, "extent": round(float(extent), 2), "margin_sizes": rel, "reps": reps}
                res["grid_ms"] = round(timed(lambda: eng.poly_set_clearances_grid(sa, sb, margin, out_t.data_ptr(), stream=sh)), 4)
                st = eng.poly_set_clearances_grid_stats()
                rec = out_t.cpu().numpy().view(pkg.CLEARANCE_DT).reshape(-1)
                win = rec["poly"] != 0xFFFFFFFF
                res["nxm_ms"] = nxm_ms
                res["none_share"] = round(float((~win).mean()), 4)
                res["hit_share"] = round(float((rec["hit"] == 1).mean()), 4)
                res["listed"] = st["listed"]
                for key in ("walked", "candidates", "tested", "walks"):
                    res[key] = round(st[key] / n_a, 2)
                if nxm_ms is not None and win.all():
                    assert full_t.cpu().numpy().tobytes() == rec.tobytes(), f"{res['config']}: every query has a winner, and the bytes differ from c2d_poly_set_clearances'"
                    res["equals_nxm"] = True
                # the chain: count, then the list at its exact capacity and the records on the device count
                cnt.zero_()
                eng.poly_near_broad_pairs(sa, sb, margin, None, 0, cnt.data_ptr(), stream=sh)
                stream.synchronize()
                total = int(cnt.item())
                pairs = torch.empty((max(total, 1), 2), dtype=torch.int32, device=dev)
                dist_t = torch.empty((max(total, 1), 32), dtype=torch.uint8, device=dev)

                def chain():
                    cnt.zero_()
                    eng.poly_near_broad_pairs(sa, sb, margin, pairs.data_ptr(), total, cnt.data_ptr(), stream=sh)
                    eng.poly_pair_distances(sa, sb, pairs.data_ptr(), total, dist_t.data_ptr(), n_pairs_dev=cnt.data_ptr(), stream=sh)

                res["chain_ms"] = round(timed(chain), 4)
                res["chain_pairs"] = round(total / n_a, 2)
                print(json.dumps(res), flush=True)
                rows.append(res)
                del pairs, dist_t
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
