"""Graph-capture check of c2d_sat_poly_cross_mask, run as a separate process by tests/test_gpu_sat_poly_cross.py.

torch must be imported before libc2d.so in a process that uses both (tests/graph_capture_check.py says why).  One capture
of the mask form, with its count, on a single stream; three replays must give the eager call's mask and count."""
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


def main():
    eng = pkg.Engine(0)
    dev = torch.device("cuda", 0)
    n_a, n_b = 3000, 5001
    a = wl.random_convex_polygon_set(n_a, seed=101, extent=12.0)
    b = wl.random_convex_polygon_set(n_b, seed=102, extent=12.0, kmax=12, rows=12)
    t = [[torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in s] for s in (a, b)]
    sa = eng.poly_set(t[0][0].data_ptr(), t[0][1].data_ptr(), t[0][2].data_ptr(), n_a, 16)
    sb = eng.poly_set(t[1][0].data_ptr(), t[1][1].data_ptr(), t[1][2].data_ptr(), n_b, 12)
    words = (n_b + 63) // 64
    for upper in (False, True):
        eager = torch.zeros((n_a, words), dtype=torch.int64, device=dev)
        eager_cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        eng.sat_poly_cross_mask(sa, sb, eager.data_ptr(), upper=upper, count=eager_cnt.data_ptr())
        torch.cuda.synchronize()
        mask = torch.zeros((n_a, words), dtype=torch.int64, device=dev)
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.graph(g, stream=side):
            sh = torch.cuda.current_stream(dev).cuda_stream
            eng.sat_poly_cross_mask(sa, sb, mask.data_ptr(), upper=upper, count=cnt.data_ptr(), stream=sh)
        for rep in range(3):
            mask.fill_(-1)
            cnt.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(mask, eager), f"replay {rep} (upper={upper}): mask differs from the eager call"
            assert int(cnt.item()) == int(eager_cnt.item()) > 0, f"replay {rep} (upper={upper}): count differs"
        del g
    eng.check_async()
    print(f"poly cross graph ok: {n_a} x {n_b}, full and upper, 3 replays each equal the eager call")
    eng.close()


if __name__ == "__main__":
    main()
