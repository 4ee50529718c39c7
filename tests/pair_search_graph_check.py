"""Graph-capture check of the broad-phase pair searches, run as a separate process by the test_graph_capture of
tests/test_gpu_sat_broad.py, test_gpu_sat_poly_broad.py, test_gpu_sweep_broad.py and test_gpu_near_broad.py:
    pair_search_graph_check.py rect_broad | poly_broad | sweep_broad | near_broad

torch must be imported before libc2d.so in a process that uses both (tests/graph_capture_check.py says why).  A capture on a
fresh ctx must be refused before it enqueues anything (the ctx scratch would have to grow).  After one eager call of the same
size, one capture of the list with its count on a single stream, replayed three times, must give the eager call's list and count,
in two-set and in self (upper) mode.  Each stage is printed as it starts, so that a failure names its stage.  The searches differ
in SEARCHES alone: how a set is made of torch tensors, the call, and the least total the eager call must find.
TEST INFRASTRUCTURE: uses the oracle to build the rectangles."""
import os
import sys

import torch  # noqa: F401  (first: see above)
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
import importlib  # noqa: E402

wl = importlib.import_module("c2d_amd.workloads")
MARGIN = 0.5


def stage(msg):
    print(msg, flush=True)


def rectangles(eng, dev, n, seed):
    """(tensors to keep, the call's arguments of the set): eight planes of one tensor"""
    from oracle import cpu as oracle

    t = torch.from_numpy(oracle.rects_from_poses(*wl.random_obb_pose_planes(n, seed=seed, extent=120.0)[:5])).to(dev)
    return t, ([t.data_ptr() + 4 * k * t.stride(0) for k in range(8)], n)


def polygons(extent, moving=False):
    def build(eng, dev, n, seed):
        """(tensors to keep, (the c2d_poly_set,) or (the c2d_poly_set, its motion planes))"""
        t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in wl.random_convex_polygon_set(n, seed=seed, extent=extent)]
        args = (eng.poly_set(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), n, wl.KMAX),)
        if moving:
            rng = np.random.default_rng(seed)
            ang, mag = rng.uniform(0, 2 * np.pi, n), rng.uniform(1.0, 4.0, n)
            t += [torch.from_numpy((mag * f(ang)).astype(np.float32)).to(dev) for f in (np.cos, np.sin)]
            args += ((t[3].data_ptr(), t[4].data_ptr()),)
        return t, args
    return build


# search -> (the word of its last line, how a set is built, call(eng, a, b, pairs, cap, cnt, **upper / stream), the eager total exceeds)
SEARCHES = {
    "rect_broad": ("broad", rectangles, lambda eng, a, b, *out, **kw: eng.sat_rect_broad_pairs(*a, *b, *out, **kw), 0),
    "poly_broad": ("poly broad", polygons(80.0), lambda eng, a, b, *out, **kw: eng.sat_poly_broad_pairs(*a, *b, *out, **kw), 10_000),
    "sweep_broad": ("sweep broad", polygons(120.0, moving=True),
                    lambda eng, a, b, *out, **kw: eng.poly_sweep_broad_pairs(a[0], b[0], *out, a[1], b[1], **kw), 10_000),
    "near_broad": ("near broad", polygons(120.0), lambda eng, a, b, *out, **kw: eng.poly_near_broad_pairs(*a, *b, MARGIN, *out, **kw), 10_000),
}


def main(search):
    label, build, call, least = SEARCHES[search]
    dev = torch.device("cuda", 0)
    n_a, n_b = 30_000, 20_001
    eng = pkg.Engine(0)
    ta, sa = build(eng, dev, n_a, 201)
    tb, sb = build(eng, dev, n_b, 202)
    cap = 1_000_000
    side = torch.cuda.Stream(device=dev)

    stage("capture on a fresh ctx")
    pairs = torch.full((cap, 2), -1, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    g = torch.cuda.CUDAGraph()
    status = None
    with torch.cuda.graph(g, stream=side):
        try:
            call(eng, sa, sb, pairs.data_ptr(), cap, cnt.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
        except pkg.C2DError as e:
            status = e.status
    del g
    torch.cuda.synchronize()
    assert status == -1, f"a capture that has to grow the scratch was not refused (status {status})"
    assert int(cnt.item()) == 0 and bool((pairs == -1).all()), "the refused call wrote something"

    for upper, sb_ in ((False, sb), (True, sa)):
        stage(f"eager call (upper={upper})")
        eager = torch.full((cap, 2), -1, dtype=torch.int32, device=dev)
        eager_cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        call(eng, sa, sb_, eager.data_ptr(), cap, eager_cnt.data_ptr(), upper=upper)
        torch.cuda.synchronize()
        total = int(eager_cnt.item())
        assert least < total <= cap, total
        stage(f"capture (upper={upper}, {total} pairs)")
        pairs = torch.zeros((cap, 2), dtype=torch.int32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            sh = torch.cuda.current_stream(dev).cuda_stream
            call(eng, sa, sb_, pairs.data_ptr(), cap, cnt.data_ptr(), upper=upper, stream=sh)
        for rep in range(3):
            stage(f"replay {rep} (upper={upper})")
            pairs.fill_(-1)
            cnt.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(pairs, eager), f"replay {rep} (upper={upper}): list differs from the eager call"
            assert int(cnt.item()) == total, f"replay {rep} (upper={upper}): count differs"
        del g
        torch.cuda.synchronize()
    eng.check_async()
    print(f"{label} graph ok: {n_a} x {n_b}, two-set and self upper, 3 replays each equal the eager call; fresh-ctx capture refused",
          flush=True)
    eng.close()


if __name__ == "__main__":
    main(sys.argv[1])
