#!/usr/bin/env python3
"""Developer tool: the ray query (c2d_poly_ray_casts) next to the way the engine answers the boolean half of the same question without it,
one JSON line per shape.  GPU only, no oracle (tests/test_gpu_ray_casts.py checks the values).

Scenes: the sparse polygon scene of poly_broad_bench.py (K ~ U{3..16}, extent 200 * sqrt(N / 32768)) as B, and segments that start
anywhere in B's box, with a uniform direction and a length uniform in [0, 24).  Two shapes: 2^20 segments x 4096 polygons (many row
tiles, one strip) and 4096 segments x 2^20 polygons (few row tiles: B is cut into strips that meet in the atomic minimum).  Per shape,
HIP events on one stream, median of --reps (>= 7) after a warm-up:
  rays_ms           c2d_poly_ray_casts alone
  mask_ms           the yardstick, in the same run: c2d_sat_poly_cross_mask with the same segments as 2-gons (o, o + d) against the
                    same B — an R x M bit matrix that says whether, never where or which first, and leaves every row to be reduced
  rays_over_mask    rays_ms / mask_ms
  edge_tests        segments x the sum of B's vertex counts;  edge_tests_per_s = edge_tests / rays_ms
  hit_share         the share of segments with a hit;  mask_row_share the share of mask rows with a set bit (the same number)
The grid leg (--grid; c2d_poly_ray_casts_grid), in the same run with the same inputs, c2d_poly_ray_casts being the yardstick:
  grid_ms, rays_ms, rays_over_grid           on the two shapes above
  2^20 segments x 2^20 polygons              rays_ms is timed on the first --few segments and scaled by n_rays / --few ("rays_ms_scaled")
  candidates / visited per ray, listed_share from c2d_poly_ray_casts_grid_stats
  equal                                      the grid call's records are the brute-force call's bytes (asserted)
  on the sparse 2^20 x 4096 shape the tool asserts  visited <= 16 * (candidates + n_rays): a walk that visits a multiple of M fails
  break_even                                 for n_rays = --many and n_rays = --few, both calls over n_b = 64 .. 262144
The kernels' own times come from a separate run under `rocprofv3 --kernel-trace --stats -- python3 ray_bench.py --once`.
usage: ray_bench.py [--many 1048576] [--few 4096] [--reps 7] [--once] [--grid]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--many", type=int, default=1 << 20)
    ap.add_argument("--few", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--grid", action="store_true", help="the grid leg instead of the mask leg")
    args = ap.parse_args()
    reps = max(7, args.reps)
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    sh = stream.cuda_stream

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

    def scene(n_rays, n_b, extent=None):
        extent = 200.0 * np.sqrt(n_b / 32768) if extent is None else extent
        host = wl.random_convex_polygon_set(n_b, seed=0xC505, extent=extent)
        rng = np.random.default_rng(0x5E6)
        ox, oy = rng.uniform(-extent, extent, n_rays), rng.uniform(-extent, extent, n_rays)
        ang, length = rng.uniform(0.0, 2.0 * np.pi, n_rays), rng.uniform(0.0, 24.0, n_rays)
        rays = np.stack([ox, oy, length * np.cos(ang), length * np.sin(ang)]).astype(np.float32)
        tb = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in host]
        return extent, tb, torch.from_numpy(rays).to(dev), eng.poly_set(tb[0].data_ptr(), tb[1].data_ptr(), tb[2].data_ptr(), n_b, wl.KMAX)

    def grid_leg(config, n_rays, n_b, sample=None, check_walk=False):
        """both calls on one scene; sample: the brute-force call runs on the first `sample` rays only and its time is scaled"""
        extent, tb, t_rays, b = scene(n_rays, n_b)
        n_brute = n_rays if sample is None else min(sample, n_rays)
        planes = [t_rays[p].data_ptr() for p in range(4)]
        out_g = torch.empty((n_rays, 4), dtype=torch.int32, device=dev)
        out_b = torch.empty((n_brute, 4), dtype=torch.int32, device=dev)
        grid_call = lambda: eng.poly_ray_casts_grid(planes, n_rays, b, out_g.data_ptr(), stream=sh)      # noqa: E731
        brute_call = lambda: eng.poly_ray_casts(planes, n_brute, b, out_b.data_ptr(), stream=sh)         # noqa: E731
        if args.once:
            grid_call()
            brute_call()
            stream.synchronize()
            return None
        res = {"config": config, "n_rays": n_rays, "n_b": n_b, "reps": reps, "extent": round(float(extent), 2)}
        res["grid_ms"] = round(timed(grid_call), 4)
        st = eng.poly_ray_casts_grid_stats()
        brute_ms = timed(brute_call)
        if sample is None:
            res["rays_ms"] = round(brute_ms, 4)
        else:
            res["rays_ms_sample"], res["sample"] = round(brute_ms, 4), n_brute
            brute_ms *= n_rays / n_brute
            res["rays_ms_scaled"] = round(brute_ms, 2)
        res["rays_over_grid"] = round(brute_ms / res["grid_ms"], 2)
        res["equal"] = bool(torch.equal(out_g[:n_brute], out_b))
        res["candidates_per_ray"] = round(st["candidates"] / n_rays, 2)
        res["visited_per_ray"] = round(st["visited"] / n_rays, 2)
        res["listed_share"] = round(st["listed"] / n_rays, 6)
        res["outliers"] = st["outliers"]
        res["hit_share"] = round(float(((out_g[:, 3] >> 16) & 1).float().mean().item()), 4)
        print(json.dumps(res), flush=True)
        assert res["equal"], "the grid call's records differ from the brute-force call's"
        if check_walk:
            assert st["visited"] <= 16 * (st["candidates"] + n_rays), "the walk visits far more entries than it has candidates"
        return res

    if args.grid:
        grid_leg("many_segments", args.many, args.few, check_walk=True)
        grid_leg("many_polygons", args.few, args.many)
        grid_leg("many_both", args.many, args.many, sample=args.few)
        if not args.once:
            for n_rays in (args.many, args.few):
                pts, even = [], None
                for n_b in (64, 256, 1024, 4096, 16384, 65536, 262144):
                    if n_rays * n_b > 1 << 36:
                        break
                    extent, tb, t_rays, b = scene(n_rays, n_b)
                    planes = [t_rays[p].data_ptr() for p in range(4)]
                    out = torch.empty((n_rays, 4), dtype=torch.int32, device=dev)
                    g = timed(lambda: eng.poly_ray_casts_grid(planes, n_rays, b, out.data_ptr(), stream=sh))
                    r = timed(lambda: eng.poly_ray_casts(planes, n_rays, b, out.data_ptr(), stream=sh))
                    pts.append({"n_b": n_b, "grid_ms": round(g, 4), "rays_ms": round(r, 4)})
                    if even is None and g < r:
                        even = n_b
                print(json.dumps({"config": "break_even", "n_rays": n_rays, "first_n_b_where_the_grid_wins": even, "points": pts}), flush=True)
        eng.check_async()
        eng.close()
        return

    for config, n_rays, n_b in (("many_segments", args.many, args.few), ("many_polygons", args.few, args.many)):
        extent = 200.0 * np.sqrt(n_b / 32768)
        host = wl.random_convex_polygon_set(n_b, seed=0xC505, extent=extent)
        rng = np.random.default_rng(0x5E6)
        ox, oy = rng.uniform(-extent, extent, n_rays), rng.uniform(-extent, extent, n_rays)
        ang, length = rng.uniform(0.0, 2.0 * np.pi, n_rays), rng.uniform(0.0, 24.0, n_rays)
        rays = np.stack([ox, oy, length * np.cos(ang), length * np.sin(ang)]).astype(np.float32)
        segs = np.stack([rays[0], rays[0] + rays[2], rays[1], rays[1] + rays[3]]).astype(np.float32)      # vx[2][n] | vy[2][n]
        tb = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in host]
        t_rays, t_segs = torch.from_numpy(rays).to(dev), torch.from_numpy(segs).to(dev)
        b = eng.poly_set(tb[0].data_ptr(), tb[1].data_ptr(), tb[2].data_ptr(), n_b, wl.KMAX)
        a = eng.poly_set(t_segs[0].data_ptr(), t_segs[2].data_ptr(), None, n_rays, 2)
        out = torch.empty((n_rays, 4), dtype=torch.int32, device=dev)
        words = (n_b + 63) // 64
        mask = torch.empty((n_rays, words), dtype=torch.int64, device=dev)

        def rays_call():
            eng.poly_ray_casts([t_rays[p].data_ptr() for p in range(4)], n_rays, b, out.data_ptr(), stream=sh)

        def mask_call():
            eng.sat_poly_cross_mask(a, b, mask.data_ptr(), stream=sh)

        if args.once:
            rays_call()
            mask_call()
            stream.synchronize()
            continue
        edge_tests = n_rays * int(host[2].astype(np.int64).sum())
        res = {"config": config, "n_rays": n_rays, "n_b": n_b, "reps": reps, "extent": round(float(extent), 2)}
        res["rays_ms"] = round(timed(rays_call), 4)
        res["mask_ms"] = round(timed(mask_call), 4)
        res["rays_over_mask"] = round(res["rays_ms"] / res["mask_ms"], 3)
        res["edge_tests"] = edge_tests
        res["edge_tests_per_s"] = round(edge_tests / (res["rays_ms"] * 1e-3), 0)
        res["hit_share"] = round(float(((out[:, 3] >> 16) & 1).float().mean().item()), 4)      # byte 14 of a record is `hit`
        res["mask_row_share"] = round(float((mask != 0).any(dim=1).float().mean().item()), 4)
        assert res["hit_share"] == res["mask_row_share"], "the ray query and the mask disagree on which segments touch anything"
        print(json.dumps(res), flush=True)
        del mask, out, t_rays, t_segs, tb
    eng.check_async()
    eng.close()


if __name__ == "__main__":
    main()
