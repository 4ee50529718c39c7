"""Graph-capture check of c2d_poly_set_casts_grid, run as a separate process by tests/test_gpu_casts_grid.py, after
tests/cast_graph_check.py and tests/clearance_grid_graph_check.py:
    python tests/cast_grid_graph_check.py

torch must be imported before libc2d.so in a process that uses both (tests/graph_capture_check.py says why).  A capture on a fresh
ctx must be refused before it enqueues anything (the ctx scratch would have to grow).  After one eager warm-up call of the same size,
one call is captured on a single stream and replayed six times after the queries, the polygons, the motions and the output have been
rewritten on the device: after every replay the records equal the reference of what the buffers hold THEN, and the guard records
around the output are untouched.  Each stage is printed as it starts, so that a failure names its stage."""
import importlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import pair_list_harness as h  # noqa: E402   (numpy and pytest only: it loads neither torch nor the library)
import cast_cases as cases  # noqa: E402
import cast_ref as ref  # noqa: E402

import torch  # noqa: E402, F401  (before the library: see above)
import numpy as np  # noqa: E402

from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
wl = importlib.import_module("c2d_amd.workloads")


def stage(msg):
    print(msg, flush=True)


def main():
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    n, n_b, row_base, col_base = 300, 150, 40, 1000
    a, b, ma, mb = cases.scene(wl, n_a=900, n_b=n_b, extent=30.0, reach=5.0)
    t_a = [torch.from_numpy(np.ascontiguousarray(x[..., :n])).to(dev) for x in a + ma]
    t_b = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in b + mb]
    sa = eng.poly_set(t_a[0].data_ptr(), t_a[1].data_ptr(), t_a[2].data_ptr(), n, wl.KMAX)
    sb = eng.poly_set(t_b[0].data_ptr(), t_b[1].data_ptr(), t_b[2].data_ptr(), n_b, wl.KMAX)
    size = ref.CAST_DT.itemsize
    out = torch.full((n + 2 * h.GUARD, size), h.BAND, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(device=dev)
    args = (sa, sb, (t_a[3].data_ptr(), t_a[4].data_ptr()), (t_b[3].data_ptr(), t_b[4].data_ptr()), row_base, col_base, 0, out.data_ptr() + size * h.GUARD)

    stage("capture on a fresh ctx")
    g = torch.cuda.CUDAGraph()
    status = None
    with torch.cuda.graph(g, stream=side):
        try:
            eng.poly_set_casts_grid(*args, torch.cuda.current_stream(dev).cuda_stream)
        except pkg.C2DError as e:
            status = e.status
    del g
    torch.cuda.synchronize()
    assert status == -1, f"a capture that has to grow the scratch was not refused (status {status})"
    assert bool((out == h.BAND).all()), "the refused call wrote something"

    stage(f"warm-up ({n} queries x {n_b} polygons)")
    eng.poly_set_casts_grid(*args)
    torch.cuda.synchronize()
    eager = out.cpu().numpy()[h.GUARD:h.GUARD + n].copy().view(ref.CAST_DT).reshape(-1)
    want = ref.casts(tuple(np.ascontiguousarray(x[..., :n]) for x in a), b, tuple(m[:n] for m in ma), mb, row_base=row_base, col_base=col_base)
    assert ref.same(eager, want).all(), "the warm-up call differs from the reference"
    out.fill_(h.BAND)

    stage("capture")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        eng.poly_set_casts_grid(*args, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert bool((out == h.BAND).all()), "the capture itself wrote something"
    variants = [(0, 1.0, None), (300, 1.0, None), (600, 1.0, None), (0, 0.5, None), (300, -1.0, 40), (0, 1.0, None)]
    for first, scale, drop in variants:
        stage(f"replay with queries {first}..{first + n}, the motions of B scaled by {scale}, count of polygon {drop} zeroed")
        cur_a = tuple(np.ascontiguousarray(x[..., first:first + n]) for x in a + ma)
        k = b[2].copy()
        if drop is not None:
            k[drop] = 0
        cur_b = (b[0], b[1], k, (mb[0] * np.float32(scale)).astype(np.float32), (mb[1] * np.float32(scale)).astype(np.float32))
        for t, x in zip(t_a + t_b, cur_a + cur_b):
            t.copy_(torch.from_numpy(np.ascontiguousarray(x)))
        out.fill_(h.BAND)
        g.replay()
        torch.cuda.synchronize()
        host = out.cpu().numpy()
        assert (host[:h.GUARD] == h.BAND).all() and (host[h.GUARD + n:] == h.BAND).all(), "written outside the output"
        got = host[h.GUARD:h.GUARD + n].copy().view(ref.CAST_DT).reshape(-1)
        want = ref.casts(cur_a[:3], cur_b[:3], cur_a[3:], cur_b[3:], row_base=row_base, col_base=col_base)
        assert 0.1 < (want["hit"] == 1).mean() < 0.95 and ((want["hit"] == 1) & (want["toi"] > 0)).mean() > 0.05
        assert ref.same(got, want).all(), "the records differ from the reference"
        if drop is None:
            eng.check_async()
        else:
            try:
                eng.check_async()
                raise AssertionError("the bad vertex count of a replay was not reported")
            except pkg.C2DError:
                pass
    del g
    torch.cuda.synchronize()
    eng.check_async()
    print(f"cast grid graph ok: fresh-ctx capture refused; after a warm-up one capture of {n} queries x {n_b} polygons, {len(variants)} replays followed "
          f"the device buffers", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
