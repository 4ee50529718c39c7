#!/usr/bin/env python3
"""Developer tool: the overlap queries (c2d_poly_pair_overlaps / c2d_rect_pair_overlaps) next to the distances and contacts calls on
the same lists in the same process, after contact_bench.py, one JSON line per configuration.  GPU only, no oracle
(tests/test_gpu_overlaps.py checks the values).

Scenes: one dense polygon list of about 1e7 pairs (every pair of two sets of --dense-n polygons, enumerated on the device; mostly
misses: a wave without a hit skips the clip), the all-hit broad list of the sparse self-collision scene of poly_broad_bench.py
(K ~ U{3..16}, extent 200 * sqrt(N / 32768), C2D_CROSS_UPPER with B = A), and the broad list of the rectangle scene of broad_bench.py
at the same density.  Per configuration, HIP events on one stream, median of --reps (>= 7) after a warm-up:
  overlaps_ms / distances_ms / contacts_ms   each call alone on the list (the broad lists bounded by the list's device count)
  overlaps_over_distances / overlaps_over_contacts   the ratios within this run
  overlaps_per_s   listed pairs / overlaps_ms;  hit_share / area_share: the shares of the list with hit == 1 / area > 0
The kernels' own times come from a separate run under `rocprofv3 --kernel-trace --stats -- python3 overlap_bench.py --once`.
usage: overlap_bench.py [--n 131072] [--dense-n 3163] [--reps 7] [--once]"""
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
    ap.add_argument("--n", type=int, default=131072)
    ap.add_argument("--dense-n", type=int, default=3163)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    reps = max(7, args.reps)
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    stream = torch.cuda.Stream(device=dev)
    sh = stream.cuda_stream
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)

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

    def report(config, n, total, overlaps_call, distances_call, contacts_call, overlaps_out, extra=None):
        if args.once:
            for call in (overlaps_call, distances_call, contacts_call):
                call()
            stream.synchronize()
            return
        out = {"config": config, "n": n, "pairs": total, "reps": reps}
        for name, call in (("overlaps", overlaps_call), ("distances", distances_call), ("contacts", contacts_call)):
            out[name + "_ms"] = round(timed(call), 4)
        out["overlaps_over_distances"] = round(out["overlaps_ms"] / out["distances_ms"], 3)
        out["overlaps_over_contacts"] = round(out["overlaps_ms"] / out["contacts_ms"], 3)
        out["overlaps_per_s"] = round(total / (out["overlaps_ms"] * 1e-3), 0)
        if total:     # byte 24 of a record is `hit`, the first float its area
            out["hit_share"] = round(float(overlaps_out[:total, 24].float().mean().item()), 4)
            out["area_share"] = round(float((overlaps_out.view(torch.float32)[:total, 0] > 0).float().mean().item()), 4)
        out.update(extra or {})
        print(json.dumps(out), flush=True)

    # -- one dense polygon list: every pair of two sets ------------------------------------------------------------------
    m = args.dense_n
    da = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in wl.random_convex_polygon_set(m, seed=0xC507, extent=8.0)]
    db = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in wl.random_convex_polygon_set(m, seed=0xC508, extent=8.0)]
    sa = eng.poly_set(da[0].data_ptr(), da[1].data_ptr(), da[2].data_ptr(), m, wl.KMAX)
    sb = eng.poly_set(db[0].data_ptr(), db[1].data_ptr(), db[2].data_ptr(), m, wl.KMAX)
    idx = torch.arange(m, dtype=torch.int32, device=dev)
    dense = torch.stack([idx.repeat_interleave(m), idx.repeat(m)], dim=1).contiguous()
    dovl = torch.empty((m * m, 32), dtype=torch.uint8, device=dev)
    ddist = torch.empty((m * m, 32), dtype=torch.uint8, device=dev)
    dcon = torch.empty((m * m, 16), dtype=torch.uint8, device=dev)
    report("dense_polygon_list", m, m * m,
           lambda: eng.poly_pair_overlaps(sa, sb, dense.data_ptr(), m * m, dovl.data_ptr(), stream=sh),
           lambda: eng.poly_pair_distances(sa, sb, dense.data_ptr(), m * m, ddist.data_ptr(), stream=sh),
           lambda: eng.poly_pair_contacts(sa, sb, dense.data_ptr(), m * m, dcon.data_ptr(), stream=sh), dovl)
    del dense, dovl, ddist, dcon

    # -- sparse polygons, self-collision: the broad list, all hit ----------------------------------------------------------
    n = args.n
    extent = 200.0 * np.sqrt(n / 32768)
    host = wl.random_convex_polygon_set(n, seed=0xC505, extent=extent)
    t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in host]
    s = eng.poly_set(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), n, wl.KMAX)
    cnt.zero_()
    eng.sat_poly_broad_pairs(s, s, None, 0, cnt.data_ptr(), upper=True, stream=sh)
    stream.synchronize()
    total = int(cnt.item())
    pairs = torch.empty((max(total, 1), 2), dtype=torch.int32, device=dev)
    cnt.zero_()
    eng.sat_poly_broad_pairs(s, s, pairs.data_ptr(), total, cnt.data_ptr(), upper=True, stream=sh)
    ovl = torch.empty((max(total, 1), 32), dtype=torch.uint8, device=dev)
    dist = torch.empty((max(total, 1), 32), dtype=torch.uint8, device=dev)
    con = torch.empty((max(total, 1), 16), dtype=torch.uint8, device=dev)
    report("sparse_polygons_self_upper", n, total,
           lambda: eng.poly_pair_overlaps(s, s, pairs.data_ptr(), total, ovl.data_ptr(), n_pairs_dev=cnt.data_ptr(), stream=sh),
           lambda: eng.poly_pair_distances(s, s, pairs.data_ptr(), total, dist.data_ptr(), n_pairs_dev=cnt.data_ptr(), stream=sh),
           lambda: eng.poly_pair_contacts(s, s, pairs.data_ptr(), total, con.data_ptr(), n_pairs_dev=cnt.data_ptr(), stream=sh), ovl,
           {"extent": round(float(extent), 2)})
    del pairs, ovl, dist, con

    # -- sparse rectangles, self-collision: the broad list -------------------------------------------------------------------
    poses = wl.random_obb_pose_planes(n, seed=0xB0AD, extent=extent)
    d_pose = torch.from_numpy(np.ascontiguousarray(poses[:5])).to(dev)
    planes = torch.empty((8, n), dtype=torch.float32, device=dev)
    eng.rects_from_poses(*[d_pose[k].data_ptr() for k in range(5)], n, [planes[k].data_ptr() for k in range(8)], stream=sh)
    pp = [planes[k].data_ptr() for k in range(8)]
    cnt.zero_()
    eng.sat_rect_broad_pairs(pp, n, pp, n, None, 0, cnt.data_ptr(), upper=True, stream=sh)
    stream.synchronize()
    rtotal = int(cnt.item())
    rpairs = torch.empty((max(rtotal, 1), 2), dtype=torch.int32, device=dev)
    cnt.zero_()
    eng.sat_rect_broad_pairs(pp, n, pp, n, rpairs.data_ptr(), rtotal, cnt.data_ptr(), upper=True, stream=sh)
    rovl = torch.empty((max(rtotal, 1), 32), dtype=torch.uint8, device=dev)
    rdist = torch.empty((max(rtotal, 1), 32), dtype=torch.uint8, device=dev)
    rcon = torch.empty((max(rtotal, 1), 16), dtype=torch.uint8, device=dev)
    report("sparse_rectangles_self_upper", n, rtotal,
           lambda: eng.rect_pair_overlaps(pp, n, pp, n, rpairs.data_ptr(), rtotal, rovl.data_ptr(), n_pairs_dev=cnt.data_ptr(), stream=sh),
           lambda: eng.rect_pair_distances(pp, n, pp, n, rpairs.data_ptr(), rtotal, rdist.data_ptr(), n_pairs_dev=cnt.data_ptr(), stream=sh),
           lambda: eng.rect_pair_contacts(pp, n, pp, n, rpairs.data_ptr(), rtotal, rcon.data_ptr(), n_pairs_dev=cnt.data_ptr(), stream=sh), rovl,
           {"extent": round(float(extent), 2)})
    eng.check_async()
    eng.close()


if __name__ == "__main__":
    main()
