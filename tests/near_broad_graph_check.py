"""Graph-capture check of c2d_poly_near_broad_pairs, run as a separate process by tests/test_gpu_near_broad.py.

torch must be imported before libc2d.so in a process that uses both (tests/graph_capture_check.py says why).  A capture on a
fresh ctx must be refused before it enqueues anything (the ctx scratch would have to grow).  After one eager call of the same
size, one capture of the list with its count on a single stream, replayed three times, must give the eager call's list and count,
in two-set and in self (upper) mode.  Each stage is printed as it starts, so that a failure names its stage."""
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


def stage(msg):
    print(msg, flush=True)


def main():
    dev = torch.device("cuda", 0)
    n_a, n_b = 30_000, 20_001
    eng = pkg.Engine(0)

    def device_set(n, seed):
        t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in wl.random_convex_polygon_set(n, seed=seed, extent=120.0)]
        return t, eng.poly_set(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), n, wl.KMAX)

    ta, sa = device_set(n_a, 201)
    tb, sb = device_set(n_b, 202)
    margin = 0.5
    cap = 1_000_000
    side = torch.cuda.Stream(device=dev)

    stage("capture on a fresh ctx")
    pairs = torch.full((cap, 2), -1, dtype=torch.int32, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    g = torch.cuda.CUDAGraph()
    status = None
    with torch.cuda.graph(g, stream=side):
        try:
            eng.poly_near_broad_pairs(sa, sb, margin, pairs.data_ptr(), cap, cnt.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
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
        eng.poly_near_broad_pairs(sa, sb_, margin, eager.data_ptr(), cap, eager_cnt.data_ptr(), upper=upper)
        torch.cuda.synchronize()
        total = int(eager_cnt.item())
        assert 10_000 < total <= cap, total
        stage(f"capture (upper={upper}, {total} pairs)")
        pairs = torch.zeros((cap, 2), dtype=torch.int32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            sh = torch.cuda.current_stream(dev).cuda_stream
            eng.poly_near_broad_pairs(sa, sb_, margin, pairs.data_ptr(), cap, cnt.data_ptr(), upper=upper, stream=sh)
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
    print(f"near broad graph ok: {n_a} x {n_b}, two-set and self upper, 3 replays each equal the eager call; fresh-ctx capture refused",
          flush=True)
    eng.close()


if __name__ == "__main__":
    main()
