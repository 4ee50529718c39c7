"""Graph-capture check of c2d_poly_pair_overlaps, run as a separate process by tests/test_gpu_overlaps_contract.py, after
tests/pair_list_graph_check.py (which resolves its query from pair_list_harness.QUERIES; the overlap row is tests/overlap_query.py's):
    python tests/overlap_graph_check.py

torch must be imported before libc2d.so in a process that uses both (tests/graph_capture_check.py says why).  One call with
d_n_pairs is captured on a single stream and replayed with the counts 100, capacity - 1, 0, 1, capacity + 1000 and 65 written to the
device in between: after every replay the first min(capacity, count) records equal the reference and every record beyond them is
untouched.  The 64 x 75 sets of the shared script; the list mixes hits and misses above 0.1 each.
Each stage is printed as it starts, so that a failure names its stage."""
import importlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import pair_list_harness as h  # noqa: E402   (numpy and pytest only: it loads neither torch nor the library)
from overlap_query import OVERLAPS as Q  # noqa: E402

import torch  # noqa: E402, F401  (before the library: see above)
import numpy as np  # noqa: E402

from __graft_entry__ import load_package  # noqa: E402
import contact_cases as cases  # noqa: E402

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
    want = Q.poly_ref(a, b, *h.local(pairs))
    assert Q.mixed(want, 1) and (want["area"] > 0).mean() > 0.1, "the list does not mix hits and misses"
    ta = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in a]
    tb = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in b]
    sa = eng.poly_set(ta[0].data_ptr(), ta[1].data_ptr(), ta[2].data_ptr(), 64, wl.KMAX)
    sb = eng.poly_set(tb[0].data_ptr(), tb[1].data_ptr(), tb[2].data_ptr(), 75, wl.KMAX)
    t_pairs = torch.from_numpy(pairs.astype(np.int64).astype(np.int32)).to(dev)
    dt = Q.dts[0]
    out = torch.full((cap + 2 * h.GUARD, dt.itemsize), h.BAND, dtype=torch.uint8, device=dev)    # guard records on either side
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)

    stage(f"capture ({cap} entries)")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        sh = torch.cuda.current_stream(dev).cuda_stream
        eng.poly_pair_overlaps(sa, sb, t_pairs.data_ptr(), cap, out.data_ptr() + dt.itemsize * h.GUARD, n_pairs_dev=cnt.data_ptr(), stream=sh)
    torch.cuda.synchronize()
    assert bool((out == h.BAND).all()), "the capture itself wrote something"
    for count in (100, cap - 1, 0, 1, cap + 1000, 65):
        stage(f"replay with count {count}")
        out.fill_(h.BAND)
        cnt.fill_(count)
        g.replay()
        torch.cuda.synchronize()
        bound = min(cap, count)
        host = out.cpu().numpy()
        assert (host[:h.GUARD] == h.BAND).all() and (host[h.GUARD + bound:] == h.BAND).all(), f"count {count}: written beyond the bound"
        got = host[h.GUARD:h.GUARD + bound].copy().view(dt).reshape(-1)
        assert Q.sames[0](got, want[:bound]).all(), f"count {count}: records differ from the reference"
    del g
    torch.cuda.synchronize()
    eng.check_async()
    print(f"overlaps graph ok: one capture of {cap} entries, 6 replays followed the device count", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
