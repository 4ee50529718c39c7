"""Graph-capture check of c2d_poly_set_clearances_grid, run as a separate process by tests/test_gpu_clearances_grid.py, after
tests/pair_search_graph_check.py.

torch must be imported before libc2d.so in a process that uses both (tests/graph_capture_check.py says why).  A capture on a
fresh ctx must be refused before it enqueues anything (the ctx scratch would have to grow).  After one eager call of the same
size, one capture on a single stream, replayed three times, must give the eager call's bytes, for two sets and for one set
against itself under SKIP_SELF.  Each stage is printed as it starts, so that a failure names its stage."""
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
    n_a, n_b = 20_000, 12_001
    eng = pkg.Engine(0)

    def device_set(n, seed):
        t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in wl.random_convex_polygon_set(n, seed=seed, extent=120.0)]
        return t, eng.poly_set(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), n, wl.KMAX)

    ta, sa = device_set(n_a, 211)
    tb, sb = device_set(n_b, 212)
    margin = 0.5
    side = torch.cuda.Stream(device=dev)
    words = n_a * 8                       # a c2d_clearance is eight 32-bit words

    stage("capture on a fresh ctx")
    out = torch.full((words,), -1, dtype=torch.int32, device=dev)
    g = torch.cuda.CUDAGraph()
    status = None
    with torch.cuda.graph(g, stream=side):
        try:
            eng.poly_set_clearances_grid(sa, sb, margin, out.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
        except pkg.C2DError as e:
            status = e.status
    del g
    torch.cuda.synchronize()
    assert status == -1, f"a capture that has to grow the scratch was not refused (status {status})"
    assert bool((out == -1).all()), "the refused call wrote something"

    for flags, sb_ in ((0, sb), (pkg.CLEARANCE_SKIP_SELF, sa)):
        stage(f"eager call (flags={flags})")
        eager = torch.full((words,), -1, dtype=torch.int32, device=dev)
        eng.poly_set_clearances_grid(sa, sb_, margin, eager.data_ptr(), flags=flags)
        torch.cuda.synchronize()
        rec = eager.cpu().numpy().view(pkg.CLEARANCE_DT)
        winners = int((rec["poly"] != 0xFFFFFFFF).sum())
        assert winners > 1000, winners
        stage(f"capture (flags={flags}, {winners} winners)")
        out = torch.zeros((words,), dtype=torch.int32, device=dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            sh = torch.cuda.current_stream(dev).cuda_stream
            eng.poly_set_clearances_grid(sa, sb_, margin, out.data_ptr(), flags=flags, stream=sh)
        for rep in range(3):
            stage(f"replay {rep} (flags={flags})")
            out.fill_(-1)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager), f"replay {rep} (flags={flags}): the records differ from the eager call's"
        del g
        torch.cuda.synchronize()
    eng.check_async()
    print(f"clearance grid graph ok: {n_a} x {n_b}, two sets and self under SKIP_SELF, 3 replays each equal the eager call; fresh-ctx capture refused",
          flush=True)
    eng.close()


if __name__ == "__main__":
    main()
