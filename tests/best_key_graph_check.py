"""Graph-capture check of the best-key queries, run as a separate process by the graph tests of tests/test_gpu_ray_casts.py,
test_gpu_ray_casts_grid.py, test_gpu_clearances.py, test_gpu_casts.py and test_gpu_casts_grid.py:
    best_key_graph_check.py ray | ray_grid | clearance | cast | cast_grid

torch must be imported before libc2d.so in a process that uses both (tests/graph_capture_check.py says why).  One call is captured
on a single stream and replayed after the queries, the polygons (the casts: B's motions) and the output have been rewritten on the
device: after every replay the records equal the reference of what the buffers hold THEN, and the guard records around the output
are untouched.  The grid queries work through the ctx scratch: a capture on a fresh ctx must be refused before it enqueues anything
(the scratch would have to grow), and the capture follows one eager call of the same size; ray_grid also tries a capture of a larger
call at the end, which is refused again.  Each stage is printed as it starts, so that a failure names its stage.  The queries
differ in CHECKS alone: the scene with its tensors, and what a variant rewrites.  (c2d_poly_set_clearances_grid has a check of
its own, tests/clearance_grid_graph_check.py: 20 000 x 12 001 against the eager call's bytes.)"""
import importlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import best_key_harness as best  # noqa: E402   (numpy, pytest and the references only: it loads neither torch nor the library)
import cast_cases  # noqa: E402
import clearance_cases  # noqa: E402
import pair_list_harness as h  # noqa: E402
import ray_cases  # noqa: E402

import torch  # noqa: E402, F401  (before the library: see above)
import numpy as np  # noqa: E402

from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
wl = importlib.import_module("c2d_amd.workloads")
F = np.float32


def stage(msg):
    print(msg, flush=True)


def on_device(dev, arrays):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in arrays]


def poly_set(eng, t, n):
    return eng.poly_set(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), n, wl.KMAX)


def scaled(b, scale, drop):
    """the polygons b scaled, the count of polygon `drop` zeroed"""
    k = b[2].copy()
    if drop is not None:
        k[drop] = 0
    return (b[0] * F(scale)).astype(F), (b[1] * F(scale)).astype(F), k


class Rays:
    """700 of the ray scene's rays against its 311 polygons; a variant takes other rays and scales the polygons"""
    n, n_b, nouns, col_base = 700, 311, "rays", 1000
    variants = [(0, 1.0, None), (700, 1.0, None), (1300, 1.0, None), (0, 0.5, None), (700, 1.0, 40), (0, 1.0, None)]
    rewrites = "polygons"

    def __init__(self, eng, dev, room):
        self.rays, self.b = ray_cases.ray_scene(wl)
        self.t_rays = torch.zeros((4, room * self.n), dtype=torch.float32, device=dev)
        self.t_b = on_device(dev, self.b)
        self.sb = poly_set(eng, self.t_b, self.n_b)
        self.ptrs = [self.t_rays[p].data_ptr() for p in range(4)]      # (best_key_harness lays RaysOnDevice.ptrs)

    def args(self, n):
        return (self, n, self.sb), dict(col_base=self.col_base)

    def rewrite(self, first, scale, drop):
        cur, cur_b = tuple(np.ascontiguousarray(r[first:first + self.n]) for r in self.rays), scaled(self.b, scale, drop)
        self.t_rays[:, :self.n].copy_(torch.from_numpy(np.stack(cur)))
        for t, x in zip(self.t_b, cur_b):
            t.copy_(torch.from_numpy(np.ascontiguousarray(x)))
        return (cur, cur_b), dict(col_base=self.col_base)

    @staticmethod
    def mixed(want):
        return 0.2 < (want["hit"] == 1).mean() < 0.9


class Sets:
    """300 of the scene's 900 queries against its 150 polygons; a variant takes other queries and scales the polygons"""
    n, n_b, nouns, bases = 300, 150, "queries", dict(row_base=40, col_base=1000)
    variants = [(0, 1.0, None), (300, 1.0, None), (600, 1.0, None), (0, 0.5, None), (300, 1.0, 40), (0, 1.0, None)]
    rewrites = "polygons"

    def scene(self):
        return clearance_cases.scene(wl, n_a=900, n_b=self.n_b, extent=24.0)

    def __init__(self, eng, dev, room):
        self.a, self.b = self.scene()                                  # (the casts: each set with its two motion planes behind)
        self.t_a, self.t_b = on_device(dev, [x[..., :self.n] for x in self.a]), on_device(dev, self.b)
        self.sa, self.sb = poly_set(eng, self.t_a, self.n), poly_set(eng, self.t_b, self.n_b)

    def args(self, n):
        return (self.sa, self.sb, n), self.bases

    def upload(self, cur_a, cur_b):
        for t, x in zip(self.t_a + self.t_b, cur_a + cur_b):
            t.copy_(torch.from_numpy(np.ascontiguousarray(x)))

    def rewrite(self, first, scale, drop):
        cur_a, cur_b = tuple(np.ascontiguousarray(x[..., first:first + self.n]) for x in self.a), scaled(self.b, scale, drop)
        self.upload(cur_a, cur_b)
        return (cur_a, cur_b), self.bases

    @staticmethod
    def mixed(want):
        return 0.1 < (want["hit"] == 1).mean() < 0.9


class MovingSets(Sets):
    """the same of the cast scene, both sets moving; a variant takes other queries and scales B's motions"""
    variants = [(0, 1.0, None), (300, 1.0, None), (600, 1.0, None), (0, 0.5, None), (300, -1.0, 40), (0, 1.0, None)]
    rewrites = "the motions of B"

    def scene(self):
        a, b, ma, mb = cast_cases.scene(wl, n_a=900, n_b=self.n_b, extent=30.0, reach=5.0)
        return a + ma, b + mb

    def args(self, n):
        return (self.sa, self.sb, n, (self.t_a[3].data_ptr(), self.t_a[4].data_ptr()), (self.t_b[3].data_ptr(), self.t_b[4].data_ptr())), self.bases

    def rewrite(self, first, scale, drop):
        cur_a, b = tuple(np.ascontiguousarray(x[..., first:first + self.n]) for x in self.a), self.b
        cur_b = (b[0], b[1], scaled(b, 1.0, drop)[2], (b[3] * F(scale)).astype(F), (b[4] * F(scale)).astype(F))
        self.upload(cur_a, cur_b)
        return (cur_a[:3], cur_b[:3], cur_a[3:], cur_b[3:]), self.bases

    @staticmethod
    def mixed(want):
        return 0.1 < (want["hit"] == 1).mean() < 0.95 and ((want["hit"] == 1) & (want["toi"] > 0)).mean() > 0.05


# query -> (the frame's entry, the scene, the stage of the eager call before the capture (the grid queries) and whether that call is
# judged, the capture's stage, whether a larger capture is tried at the end, the last line)
CHECKS = {
    "ray": (best.RAY_CASTS, Rays, None, False, "capture ({n} rays x {n_b} polygons)", False,
            "ray graph ok: one capture of {n} rays x {n_b} polygons, {v} replays followed the device buffers"),
    "ray_grid": (best.RAY_CASTS_GRID, Rays, "eager call", False, "capture ({n} rays x {n_b} polygons)", True,
                 "ray grid graph ok: one capture of {n} rays x {n_b} polygons, {v} replays followed the device buffers; growing captures refused"),
    "clearance": (best.CLEARANCES, Sets, None, False, "capture ({n} queries x {n_b} polygons)", False,
                  "clearance graph ok: one capture of {n} queries x {n_b} polygons, {v} replays followed the device buffers"),
    "cast": (best.CASTS, MovingSets, None, False, "capture ({n} queries x {n_b} polygons)", False,
             "cast graph ok: one capture of {n} queries x {n_b} polygons, {v} replays followed the device buffers"),
    "cast_grid": (best.CASTS_GRID, MovingSets, "warm-up ({n} queries x {n_b} polygons)", True, "capture", False,
                  "cast grid graph ok: fresh-ctx capture refused; after a warm-up one capture of {n} queries x {n_b} polygons, {v} replays followed "
                  "the device buffers"),
}


def main(name):
    query, Scene, eager, judged, capture, larger, last = CHECKS[name]
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    room = 2 if larger else 1
    sc = Scene(eng, dev, room)
    n, size = sc.n, query.dt.itemsize
    words = dict(n=n, n_b=sc.n_b, v=len(sc.variants))
    out = torch.full((room * n + 2 * h.GUARD, size), h.BAND, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(device=dev)

    def launch(n_records, **stream):
        args, kw = sc.args(n_records)
        query.lay(getattr(eng, query.method), out.data_ptr() + size * h.GUARD, *args, **kw, **stream)

    def records():
        host = out.cpu().numpy()
        assert (host[:h.GUARD] == h.BAND).all() and (host[h.GUARD + n:] == h.BAND).all(), "written outside the output"
        return host[h.GUARD:h.GUARD + n].copy().view(query.dt).reshape(-1)

    def refused_capture(n_records, what):
        stage(what)
        g = torch.cuda.CUDAGraph()
        status = None
        with torch.cuda.graph(g, stream=side):
            try:
                launch(n_records, stream=torch.cuda.current_stream(dev).cuda_stream)
            except pkg.C2DError as e:
                status = e.status
        del g
        torch.cuda.synchronize()
        assert status == -1, f"a capture that has to grow the scratch was not refused (status {status})"
        assert bool((out == h.BAND).all()), "the refused call wrote something"

    if eager is not None:
        refused_capture(n, "capture on a fresh ctx")
        stage(eager.format(**words))
        launch(n)
        torch.cuda.synchronize()
        if judged:
            args, kw = sc.rewrite(*sc.variants[0])                     # (what the buffers hold already)
            assert query.ref.same(records(), query.reference(*args, **kw)).all(), "the warm-up call differs from the reference"
        out.fill_(h.BAND)
        torch.cuda.synchronize()

    stage(capture.format(**words))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        launch(n, stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert bool((out == h.BAND).all()), "the capture itself wrote something"
    for first, scale, drop in sc.variants:
        stage(f"replay with {sc.nouns} {first}..{first + n}, {sc.rewrites} scaled by {scale}, count of polygon {drop} zeroed")
        args, kw = sc.rewrite(first, scale, drop)
        out.fill_(h.BAND)
        g.replay()
        torch.cuda.synchronize()
        got, want = records(), query.reference(*args, **kw)
        assert sc.mixed(want)
        assert query.ref.same(got, want).all(), "the records differ from the reference"
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
    if larger:
        out.fill_(h.BAND)
        torch.cuda.synchronize()
        refused_capture(2 * n, "capture of a larger call than the eager one")
    eng.check_async()
    print(last.format(**words), flush=True)
    eng.close()


if __name__ == "__main__":
    main(sys.argv[1])
