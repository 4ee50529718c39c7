"""Graph-capture check of a list-driven query's polygon call, run as a separate process by tests/test_gpu_pair_list_contract.py:
    python tests/pair_list_graph_check.py contacts|manifolds|distances|sweeps

torch must be imported before libc2d.so in a process that uses both (tests/graph_capture_check.py says why).  One call with
d_n_pairs (and, for the sweeps, both sets' motion planes) is captured on a single stream and replayed with different counts written
to the device in between: after every replay the first min(capacity, count) records of every output equal the query's reference
and every record beyond them is untouched.  The list mixes the query's classes (Query.mix: hits and misses above 0.1 each; the
sweeps: start overlap between 0.1 and 0.9, moving hits above 0.05, misses above 0.05).
Each stage is printed as it starts, so that a failure names its stage."""
import importlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import pair_list_harness as h  # noqa: E402   (numpy and pytest only: it loads neither torch nor the library)

BY_NAME = {q.name: q for q in h.QUERIES}
if len(sys.argv) != 2 or sys.argv[1] not in BY_NAME:
    sys.exit(f"usage: {os.path.basename(sys.argv[0])} {'|'.join(BY_NAME)}")

import torch  # noqa: E402, F401  (before the library: see above)
import numpy as np  # noqa: E402

from __graft_entry__ import load_package  # noqa: E402
import contact_cases as cases  # noqa: E402

pkg = load_package()
wl = importlib.import_module("c2d_amd.workloads")


def stage(msg):
    print(msg, flush=True)


def main(q):
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    a, b = cases.dense_poly_sets(wl, n=64, extent=3.0)
    pairs = cases.all_pairs(64, 75)[::2]
    cap = len(pairs)
    x = q.extras(9201, 64, 75, 3.0)
    wants = h.outputs(q.poly_ref(a, b, *h.local(pairs), *x))
    assert q.mixed(wants, 1), "the list does not mix the query's classes"
    ta = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in a]
    tb = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in b]
    sa = eng.poly_set(ta[0].data_ptr(), ta[1].data_ptr(), ta[2].data_ptr(), 64, wl.KMAX)
    sb = eng.poly_set(tb[0].data_ptr(), tb[1].data_ptr(), tb[2].data_ptr(), 75, wl.KMAX)
    tx = [[torch.from_numpy(plane).to(dev) for plane in m] for m in x]
    kw = {name: tuple(t.data_ptr() for t in m) for name, m in zip(("a_motion", "b_motion"), tx)}
    t_pairs = torch.from_numpy(pairs.astype(np.int64).astype(np.int32)).to(dev)
    outs = [torch.full((cap + 2 * h.GUARD, dt.itemsize), h.BAND, dtype=torch.uint8, device=dev) for dt in q.dts]    # guard records on either side
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)

    stage(f"capture ({cap} entries)")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        sh = torch.cuda.current_stream(dev).cuda_stream
        getattr(eng, q.poly)(sa, sb, t_pairs.data_ptr(), cap, *[o.data_ptr() + dt.itemsize * h.GUARD for o, dt in zip(outs, q.dts)],
                             n_pairs_dev=cnt.data_ptr(), stream=sh, **kw)
    torch.cuda.synchronize()
    assert all(bool((o == h.BAND).all()) for o in outs), "the capture itself wrote something"
    for count in (100, cap - 1, 0, 1, cap + 1000, 65):
        stage(f"replay with count {count}")
        for o in outs:
            o.fill_(h.BAND)
        cnt.fill_(count)
        g.replay()
        torch.cuda.synchronize()
        bound = min(cap, count)
        for o, dt, same, want, noun in zip(outs, q.dts, q.sames, wants, q.nouns):
            host = o.cpu().numpy()
            assert (host[:h.GUARD] == h.BAND).all() and (host[h.GUARD + bound:] == h.BAND).all(), f"count {count}: written beyond the bound"
            got = host[h.GUARD:h.GUARD + bound].copy().view(dt).reshape(-1)
            assert same(got, want[:bound]).all(), f"count {count}: {noun} differ from the reference"
    del g
    torch.cuda.synchronize()
    eng.check_async()
    print(f"{q.name} graph ok: one capture of {cap} entries, 6 replays followed the device count", flush=True)
    eng.close()


if __name__ == "__main__":
    main(BY_NAME[sys.argv[1]])
