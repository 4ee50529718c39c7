"""Graph-capture check of c2d_poly_ray_casts_grid, run as a separate process by tests/test_gpu_ray_casts_grid.py:
    python tests/ray_grid_graph_check.py

torch must be imported before libc2d.so in a process that uses both (tests/graph_capture_check.py says why).  A capture on a fresh
ctx must be refused before it enqueues anything (the ctx scratch would have to grow).  After one eager call of the same size, one
call is captured on a single stream and replayed after the rays, the polygons and the output have been rewritten on the device:
after every replay the records equal the reference of what the buffers hold THEN, and the guard records around the output are
untouched.  A capture of a larger call than the eager one is refused again.  Each stage is printed as it starts."""
import importlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import pair_list_harness as h  # noqa: E402   (numpy and pytest only: it loads neither torch nor the library)
import ray_cases as cases  # noqa: E402
import ray_grid_ref as gref  # noqa: E402

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
    rays, b = cases.ray_scene(wl)
    n, n_b, col_base = 700, 311, 1000
    t_rays = torch.zeros((4, 2 * n), dtype=torch.float32, device=dev)
    t_b = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in b]
    sb = eng.poly_set(t_b[0].data_ptr(), t_b[1].data_ptr(), t_b[2].data_ptr(), n_b, wl.KMAX)
    out = torch.full((2 * n + 2 * h.GUARD, 16), h.BAND, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(device=dev)
    planes = [t_rays[p].data_ptr() for p in range(4)]

    def refused_capture(n_rays, what):
        stage(what)
        g = torch.cuda.CUDAGraph()
        status = None
        with torch.cuda.graph(g, stream=side):
            try:
                eng.poly_ray_casts_grid(planes, n_rays, sb, out.data_ptr() + 16 * h.GUARD, col_base=col_base,
                                        stream=torch.cuda.current_stream(dev).cuda_stream)
            except pkg.C2DError as e:
                status = e.status
        del g
        torch.cuda.synchronize()
        assert status == -1, f"a capture that has to grow the scratch was not refused (status {status})"
        assert bool((out == h.BAND).all()), "the refused call wrote something"

    refused_capture(n, "capture on a fresh ctx")
    stage("eager call")
    eng.poly_ray_casts_grid(planes, n, sb, out.data_ptr() + 16 * h.GUARD, col_base=col_base)
    torch.cuda.synchronize()
    out.fill_(h.BAND)
    torch.cuda.synchronize()

    stage(f"capture ({n} rays x {n_b} polygons)")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        sh = torch.cuda.current_stream(dev).cuda_stream
        eng.poly_ray_casts_grid(planes, n, sb, out.data_ptr() + 16 * h.GUARD, col_base=col_base, stream=sh)
    torch.cuda.synchronize()
    assert bool((out == h.BAND).all()), "the capture itself wrote something"
    variants = [(0, 1.0, None), (700, 1.0, None), (1300, 1.0, None), (0, 0.5, None), (700, 1.0, 40), (0, 1.0, None)]
    for first, scale, drop in variants:
        stage(f"replay with rays {first}..{first + n}, polygons scaled by {scale}, count of polygon {drop} zeroed")
        cur = tuple(np.ascontiguousarray(r[first:first + n]) for r in rays)
        k = b[2].copy()
        if drop is not None:
            k[drop] = 0
        cur_b = ((b[0] * np.float32(scale)).astype(np.float32), (b[1] * np.float32(scale)).astype(np.float32), k)
        t_rays[:, :n].copy_(torch.from_numpy(np.stack(cur)))
        for t, x in zip(t_b, cur_b):
            t.copy_(torch.from_numpy(np.ascontiguousarray(x)))
        out.fill_(h.BAND)
        g.replay()
        torch.cuda.synchronize()
        host = out.cpu().numpy()
        assert (host[:h.GUARD] == h.BAND).all() and (host[h.GUARD + n:] == h.BAND).all(), "written outside the output"
        got = host[h.GUARD:h.GUARD + n].copy().view(gref.RAY_HIT_DT).reshape(-1)
        want = gref.ray_casts(cur, cur_b, col_base=col_base)
        assert 0.2 < (want["hit"] == 1).mean() < 0.9
        assert gref.same(got, want).all(), "the records differ from the reference"
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
    out.fill_(h.BAND)
    torch.cuda.synchronize()
    refused_capture(2 * n, "capture of a larger call than the eager one")
    eng.check_async()
    print(f"ray grid graph ok: one capture of {n} rays x {n_b} polygons, {len(variants)} replays followed the device buffers; growing captures refused",
          flush=True)
    eng.close()


if __name__ == "__main__":
    main()
