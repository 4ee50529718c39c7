"""Graph-capture check of c2d_poly_pair_distances, run as a separate process by tests/test_gpu_distances.py.

torch must be imported before libc2d.so in a process that uses both (tests/graph_capture_check.py says why).  One distances call
with d_n_pairs is captured on a single stream and replayed with different counts written to the device in between: after every
replay the first min(capacity, count) records equal the reference (tests/distance_ref.py) and every record beyond them is
untouched.  Each stage is printed as it starts, so that a failure names its stage."""
import importlib
import os
import sys

import torch  # noqa: F401  (first: see above)
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from __graft_entry__ import load_package  # noqa: E402
import contact_cases as cases  # noqa: E402
import distance_ref as ref  # noqa: E402

pkg = load_package()
wl = importlib.import_module("c2d_amd.workloads")


def stage(msg):
    print(msg, flush=True)


def main():
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    a, b = cases.dense_poly_sets(wl, n=64, extent=3.0)
    pairs = cases.all_pairs(64, 75)[::2]
    cap = len(pairs)
    want = ref.poly_distances(a, b, pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64))
    assert 0.1 < want["hit"].mean() < 0.9
    ta = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in a]
    tb = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in b]
    sa = eng.poly_set(ta[0].data_ptr(), ta[1].data_ptr(), ta[2].data_ptr(), 64, wl.KMAX)
    sb = eng.poly_set(tb[0].data_ptr(), tb[1].data_ptr(), tb[2].data_ptr(), 75, wl.KMAX)
    t_pairs = torch.from_numpy(pairs.astype(np.int64).astype(np.int32)).to(dev)
    out = torch.full((cap + 8, 32), 0xA5, dtype=torch.uint8, device=dev)      # four guard records on either side
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)

    stage(f"capture ({cap} entries)")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        sh = torch.cuda.current_stream(dev).cuda_stream
        eng.poly_pair_distances(sa, sb, t_pairs.data_ptr(), cap, out.data_ptr() + 128, n_pairs_dev=cnt.data_ptr(), stream=sh)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()), "the capture itself wrote something"
    for count in (100, cap - 1, 0, 1, cap + 1000, 65):
        stage(f"replay with count {count}")
        out.fill_(0xA5)
        cnt.fill_(count)
        g.replay()
        torch.cuda.synchronize()
        host = out.cpu().numpy()
        bound = min(cap, count)
        assert (host[:4] == 0xA5).all() and (host[4 + bound:] == 0xA5).all(), f"count {count}: written beyond the bound"
        got = host[4:4 + bound].copy().view(ref.DISTANCE_DT).reshape(-1)
        assert ref.same(got, want[:bound]).all(), f"count {count}: records differ from the reference"
    del g
    torch.cuda.synchronize()
    eng.check_async()
    print(f"distance graph ok: one capture of {cap} entries, 6 replays followed the device count", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
