#!/usr/bin/env python3
"""Developer tool: the contact queries (c2d_poly_pair_contacts / c2d_rect_pair_contacts, and c2d_poly_pair_manifolds), the distance queries
(c2d_poly_pair_distances / c2d_rect_pair_distances) and the swept queries (c2d_poly_pair_sweeps / c2d_rect_pair_sweeps) next to the list calls that feed them, one JSON line per configuration.  GPU only, no oracle (tests/test_gpu_contacts.py checks the values).

Scenes: the sparse self-collision scenes of poly_broad_bench.py (K ~ U{3..16}, extent 200 * sqrt(N / 32768)) and broad_bench.py
(rectangles of random_obb_pose_planes at the same density), C2D_CROSS_UPPER with B = A; and one dense polygon list of about 1e7
pairs (every pair of two sets of --dense-n polygons, enumerated on the device).  Per configuration, HIP events on one stream,
median of --reps (>= 7) after a warm-up:
  list_ms         the broad-phase list call alone (exact capacity)
  contacts_ms     the contacts call alone on that list, bounded by the list's device count
  both_ms         the two back to back on the stream, no host synchronisation between them
  contacts_per_s  listed pairs / contacts_ms;   hits: the list's length
  manifolds_ms    (polygon scenes) c2d_poly_pair_manifolds alone on the same list in the same run; manifolds_over_contacts is its
                  ratio to contacts_ms — the contacts call is the yardstick
  distances_ms    the distances call alone on the same list in the same run; distances_over_contacts its ratio to contacts_ms,
                  distances_per_s listed pairs / distances_ms, separated_share the share of the list that is not hit (a wave of
                  hit pairs skips the candidate loops: the broad lists are all hit, the dense list is mostly separated)
  sweeps_ms       the sweeps call alone on the same list in the same run, both sets moving by up to +---motion per component (seeded);
                  sweeps_over_contacts its ratio to contacts_ms, sweeps_per_s listed pairs / sweeps_ms, start_share / moving_hit_share
                  the shares of the list that start in overlap / first touch during the step (a wave of start-overlap pairs skips
                  the axis walk: the broad lists are all start overlap); sweeps_still_ms the same call with no motion planes (every
                  wave skips the walk: the pairwise test, the gather and the store alone)
The kernels' own times come from a separate run under `rocprofv3 --kernel-trace --stats -- python3 contact_bench.py --once`.
usage: contact_bench.py [--n 131072] [--dense-n 3163] [--reps 7] [--motion 2.0] [--once]"""
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
    ap.add_argument("--motion", type=float, default=2.0)
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

    def motion_planes(count, seed):
        """dx, dy f32[count] of one set, uniform in +-args.motion -> the two tensors (kept alive by the caller) and their pointers"""
        rng = np.random.default_rng(seed)
        m = [torch.from_numpy(rng.uniform(-args.motion, args.motion, count).astype(np.float32)).to(dev) for _ in range(2)]
        return m, (m[0].data_ptr(), m[1].data_ptr())

    def report(config, n, list_call, contacts_call, total, extra=None, manifolds_call=None, distances_call=None, distances_out=None, sweeps_call=None,
               sweeps_still_call=None, sweeps_out=None):
        def both():
            if list_call is not None:
                list_call()
            contacts_call()

        if args.once:
            both()
            if manifolds_call is not None:
                manifolds_call()
            if distances_call is not None:
                distances_call()
            if sweeps_call is not None:
                sweeps_call()
                sweeps_still_call()
            stream.synchronize()
            return
        out = {"config": config, "n": n, "hits": total, "reps": reps}
        if list_call is not None:
            out["list_ms"] = round(timed(list_call), 4)
        out["contacts_ms"] = round(timed(contacts_call), 4)
        if list_call is not None:
            out["both_ms"] = round(timed(both), 4)
        out["contacts_per_s"] = round(total / (out["contacts_ms"] * 1e-3), 0)
        if manifolds_call is not None:
            out["manifolds_ms"] = round(timed(manifolds_call), 4)
            out["manifolds_over_contacts"] = round(out["manifolds_ms"] / out["contacts_ms"], 3)
        if distances_call is not None:
            out["distances_ms"] = round(timed(distances_call), 4)
            out["distances_over_contacts"] = round(out["distances_ms"] / out["contacts_ms"], 3)
            out["distances_per_s"] = round(total / (out["distances_ms"] * 1e-3), 0)
            if total:     # byte 24 of a record is `hit`
                out["separated_share"] = round(1.0 - float(distances_out[:total, 24].float().mean().item()), 4)
        if sweeps_call is not None:
            out["sweeps_ms"] = round(timed(sweeps_call), 4)
            out["sweeps_over_contacts"] = round(out["sweeps_ms"] / out["contacts_ms"], 3)
            out["sweeps_per_s"] = round(total / (out["sweeps_ms"] * 1e-3), 0)
            if total:     # byte 14 of a record is `hit`, byte 15 `flags` (1: START_OVERLAP)
                start = sweeps_out[:total, 15] == 1
                out["start_share"] = round(float(start.float().mean().item()), 4)
                out["moving_hit_share"] = round(float(((sweeps_out[:total, 14] == 1) & ~start).float().mean().item()), 4)
            out["sweeps_still_ms"] = round(timed(sweeps_still_call), 4)
            out["motion"] = args.motion
        out.update(extra or {})
        print(json.dumps(out), flush=True)

    n = args.n
    extent = 200.0 * np.sqrt(n / 32768)
    # -- sparse polygons, self-collision ---------------------------------------------------------------------------------
    host = wl.random_convex_polygon_set(n, seed=0xC505, extent=extent)
    t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in host]
    s = eng.poly_set(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), n, wl.KMAX)
    cnt.zero_()
    eng.sat_poly_broad_pairs(s, s, None, 0, cnt.data_ptr(), upper=True, stream=sh)
    stream.synchronize()
    total = int(cnt.item())
    pairs = torch.empty((max(total, 1), 2), dtype=torch.int32, device=dev)
    out = torch.empty((max(total, 1), 16), dtype=torch.uint8, device=dev)

    def poly_list():
        cnt.zero_()
        eng.sat_poly_broad_pairs(s, s, pairs.data_ptr(), total, cnt.data_ptr(), upper=True, stream=sh)

    def poly_contacts():
        eng.poly_pair_contacts(s, s, pairs.data_ptr(), total, out.data_ptr(), n_pairs_dev=cnt.data_ptr(), stream=sh)

    man = torch.empty((max(total, 1), 32), dtype=torch.uint8, device=dev)

    def poly_manifolds():
        eng.poly_pair_manifolds(s, s, pairs.data_ptr(), total, out.data_ptr(), man.data_ptr(), n_pairs_dev=cnt.data_ptr(), stream=sh)

    dist = torch.empty((max(total, 1), 32), dtype=torch.uint8, device=dev)

    def poly_distances():
        eng.poly_pair_distances(s, s, pairs.data_ptr(), total, dist.data_ptr(), n_pairs_dev=cnt.data_ptr(), stream=sh)

    swp = torch.empty((max(total, 1), 16), dtype=torch.uint8, device=dev)
    keep_m, mot = motion_planes(n, 0xC50A)

    def poly_sweeps():
        eng.poly_pair_sweeps(s, s, pairs.data_ptr(), total, swp.data_ptr(), a_motion=mot, b_motion=mot, n_pairs_dev=cnt.data_ptr(), stream=sh)

    def poly_sweeps_still():
        eng.poly_pair_sweeps(s, s, pairs.data_ptr(), total, swp.data_ptr(), n_pairs_dev=cnt.data_ptr(), stream=sh)

    poly_list()
    report("sparse_polygons_self_upper", n, poly_list, poly_contacts, total, {"extent": round(float(extent), 2)}, poly_manifolds, poly_distances, dist,
           poly_sweeps, poly_sweeps_still, swp)
    hit_share = float((out.view(torch.int32)[:total, 3] >> 16 & 1).float().mean().item()) if total and not args.once else None
    assert hit_share in (None, 1.0), "a listed pair without `hit`"
    del pairs, out, man, dist, swp

    # -- sparse rectangles, self-collision -------------------------------------------------------------------------------
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
    rout = torch.empty((max(rtotal, 1), 16), dtype=torch.uint8, device=dev)

    def rect_list():
        cnt.zero_()
        eng.sat_rect_broad_pairs(pp, n, pp, n, rpairs.data_ptr(), rtotal, cnt.data_ptr(), upper=True, stream=sh)

    def rect_contacts():
        eng.rect_pair_contacts(pp, n, pp, n, rpairs.data_ptr(), rtotal, rout.data_ptr(), n_pairs_dev=cnt.data_ptr(), stream=sh)

    rdist = torch.empty((max(rtotal, 1), 32), dtype=torch.uint8, device=dev)

    def rect_distances():
        eng.rect_pair_distances(pp, n, pp, n, rpairs.data_ptr(), rtotal, rdist.data_ptr(), n_pairs_dev=cnt.data_ptr(), stream=sh)

    rswp = torch.empty((max(rtotal, 1), 16), dtype=torch.uint8, device=dev)

    def rect_sweeps():
        eng.rect_pair_sweeps(pp, n, pp, n, rpairs.data_ptr(), rtotal, rswp.data_ptr(), a_motion=mot, b_motion=mot, n_pairs_dev=cnt.data_ptr(), stream=sh)

    def rect_sweeps_still():
        eng.rect_pair_sweeps(pp, n, pp, n, rpairs.data_ptr(), rtotal, rswp.data_ptr(), n_pairs_dev=cnt.data_ptr(), stream=sh)

    rect_list()
    report("sparse_rectangles_self_upper", n, rect_list, rect_contacts, rtotal, {"extent": round(float(extent), 2)}, None, rect_distances, rdist,
           rect_sweeps, rect_sweeps_still, rswp)
    del rpairs, rout, rdist, rswp

    # -- one dense polygon list: every pair of two sets ------------------------------------------------------------------
    m = args.dense_n
    da = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in wl.random_convex_polygon_set(m, seed=0xC507, extent=8.0)]
    db = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in wl.random_convex_polygon_set(m, seed=0xC508, extent=8.0)]
    sa = eng.poly_set(da[0].data_ptr(), da[1].data_ptr(), da[2].data_ptr(), m, wl.KMAX)
    sb = eng.poly_set(db[0].data_ptr(), db[1].data_ptr(), db[2].data_ptr(), m, wl.KMAX)
    idx = torch.arange(m, dtype=torch.int32, device=dev)
    dense = torch.stack([idx.repeat_interleave(m), idx.repeat(m)], dim=1).contiguous()
    dout = torch.empty((m * m, 16), dtype=torch.uint8, device=dev)

    def dense_contacts():
        eng.poly_pair_contacts(sa, sb, dense.data_ptr(), m * m, dout.data_ptr(), stream=sh)

    dman = torch.empty((m * m, 32), dtype=torch.uint8, device=dev)

    def dense_manifolds():
        eng.poly_pair_manifolds(sa, sb, dense.data_ptr(), m * m, dout.data_ptr(), dman.data_ptr(), stream=sh)

    def dense_distances():      # (into the manifolds' buffer: the same 32 bytes per entry, and the manifolds leg is over by then)
        eng.poly_pair_distances(sa, sb, dense.data_ptr(), m * m, dman.data_ptr(), stream=sh)

    dswp = torch.empty((m * m, 16), dtype=torch.uint8, device=dev)
    keep_a, mot_a = motion_planes(m, 0xC50B)
    keep_b, mot_b = motion_planes(m, 0xC50C)

    def dense_sweeps():
        eng.poly_pair_sweeps(sa, sb, dense.data_ptr(), m * m, dswp.data_ptr(), a_motion=mot_a, b_motion=mot_b, stream=sh)

    def dense_sweeps_still():
        eng.poly_pair_sweeps(sa, sb, dense.data_ptr(), m * m, dswp.data_ptr(), stream=sh)

    report("dense_polygon_list", m, None, dense_contacts, m * m, None, dense_manifolds, dense_distances, dman, dense_sweeps, dense_sweeps_still, dswp)
    eng.check_async()
    eng.close()


if __name__ == "__main__":
    main()
