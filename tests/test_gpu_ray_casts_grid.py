"""GPU tests of the grid-accelerated ray queries (c2d_poly_ray_casts_grid): every field of every record equals tests/ray_grid_ref.py — the
numpy restatement of the contract of include/c2d.h, pinned by tests/test_ray_grid_ref_cpu.py — t and u bit for bit (+0 and -0 equal);
on the project's scenes the records also equal c2d_poly_ray_casts' byte for byte, in the same run.  Every output buffer handed to the
library sits between guard bands that are checked afterwards (tests/ray_harness.py, tests/pair_list_harness.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import best_key_harness as best  # noqa: E402
import ray_cases as cases  # noqa: E402
import ray_grid_cases as gcases  # noqa: E402
import ray_grid_ref as gref  # noqa: E402
import ray_ref as ref  # noqa: E402
from pair_list_harness import Uploaded  # noqa: E402
from ray_harness import RaysOnDevice, assert_same, cast, cast_grid  # noqa: E402
from ray_harness import check_grid as check, twice_grid as twice  # noqa: E402

pytestmark = pytest.mark.gpu
FUZZ_SEED = 20417
F = np.float32
DT = ref.RAY_HIT_DT
CAP = gcases.WALK_CAP


@pytest.fixture(scope="module")
def scene(wl):
    """the ray scene's polygons with 4099 rays of the same generator, and their reference records, computed once"""
    rays, b = cases.ray_scene(wl, n_rays=4099)
    want = gref.ray_casts(rays, b)
    want.setflags(write=False)
    assert want.tobytes() == ref.ray_casts(rays, b).tobytes()        # (on this scene the two contracts agree)
    return rays, b, want


def test_every_number_of_rays_and_polygons(eng, wl, scene):
    """n_rays of 1, 63..65 and 255..257 against the scene's 311 polygons; 257 rays against 1, 63..65 polygons of the scene and 513 of
    the same generator"""
    rays, b, want = scene
    ub, dr = Uploaded(eng, b), RaysOnDevice(eng, rays)
    for n in (1, 63, 64, 65, 255, 256, 257):
        got = cast_grid(eng, dr, n, ub.set, capacity=max(n, 4))
        assert_same(got[:n], want[:n], f"{n} rays")
    ub.free()
    more = wl.random_convex_polygon_set(513, seed=7103, kmin=3, kmax=16, extent=48.0, rows=16)
    for n_b, s in [(n, b) for n in (1, 63, 64, 65)] + [(513, more)]:
        sub = tuple(x[..., :n_b] for x in s)
        check(eng, rays, sub, f"{n_b} polygons", n_rays=257, on_device=dr)
    dr.free()
    eng.check_async()


def test_layout_variants(eng, wl, scene):
    """rows 4, 8 and 16; k == rows with d_k == NULL; a plane offset and a stride larger than n; a pointer-offset shard of B with
    col_base up to col_base + n_b == 2^32; ray planes at odd 4-byte offsets; n_b == 0; n_rays == 0."""
    rays, b, _ = scene
    rays = tuple(r[:600] for r in rays)
    dr = RaysOnDevice(eng, rays, offsets=(1, 3, 0, 2))
    for rows in (4, 8, 16):
        s = wl.random_convex_polygon_set(200, seed=7110 + rows, kmin=3, kmax=rows, extent=48.0, rows=rows)
        ub = Uploaded(eng, s, offset=1, stride=200 + 7)
        check(eng, rays, s, f"rows {rows}", uploaded=ub, on_device=dr)
        ub.free()
        full = wl.random_convex_polygon_set(130, seed=7120 + rows, kmin=rows, kmax=rows, extent=30.0, rows=rows)
        ub = Uploaded(eng, full, with_k=False)
        assert ub.dk is None
        got, _ = check(eng, rays, full, f"rows {rows}, d_k == NULL", uploaded=ub, on_device=dr)
        assert (got["hit"] == 1).any()
        ub.free()
    ub = Uploaded(eng, b, offset=3, stride=311 + 5)
    c0, c1, base = 37, 290, 4_000_000_000
    shard = tuple(x[..., c0:c1] for x in b)
    want = gref.ray_casts(rays, shard, col_base=base)
    assert (want["poly"][want["hit"] == 1] >= base).all()
    assert_same(cast_grid(eng, dr, 600, ub.sub(c0, c1), col_base=base), want, "a shard of B with col_base")
    top = (1 << 32) - (c1 - c0)
    assert_same(cast_grid(eng, dr, 600, ub.sub(c0, c1), col_base=top), gref.ray_casts(rays, shard, col_base=top), "col_base + n_b == 2^32")
    none = gref.ray_casts(rays, tuple(x[..., :0] for x in b))
    assert (none["hit"] == 0).all() and (none["poly"] == 0xFFFFFFFF).all()
    assert_same(cast_grid(eng, dr, 600, ub.sub(5, 5)), none, "n_b == 0")
    assert_same(cast_grid(eng, dr, 600, eng.poly_set(0, 0, None, 0, 16)), none, "n_b == 0, no planes")
    cast_grid(eng, dr, 0, ub.set, capacity=8)      # n_rays == 0: nothing is touched
    eng.check_async()
    ub.free()
    dr.free()


@pytest.mark.parametrize("name", sorted(cases.hand_cases()))
def test_hand_cases(eng, name):
    rays, b, want = cases.hand_cases()[name]
    got, _ = check(eng, rays, b, name)
    assert cases.as_tuples(got) == [tuple(w) for w in want], name
    eng.check_async()


@pytest.mark.parametrize("n_cluster", [CAP - 1, CAP, CAP + 1])
def test_both_sides_of_the_walk_cap(eng, n_cluster):
    """A cell that holds exactly cap - 1, cap and cap + 1 polygons (tests/ray_grid_cases.py cluster_scene): the two rays that look at
    that cell alone are walked up to the cap and listed beyond it; the records are the same on both routes."""
    b, rays = gcases.cluster_scene(n_cluster)
    got, stats = check(eng, rays, b, f"a cell of {n_cluster}", col_base=9)
    assert stats["listed"] == (2 if n_cluster > CAP else 0), stats
    assert stats["outliers"] == 0 and stats["visited"] >= 2 * min(n_cluster, CAP)
    if n_cluster <= CAP:
        assert stats["visited"] < 2 * n_cluster + 64 and stats["candidates"] >= 2 * n_cluster      # (the third ray sees a few far squares)
    assert cases.as_tuples(got[:2]) == [(9, 0.0, 0.0, 0xFFFF, 1, 1), (9, 0.5, 0.5, 3, 1, 0)]
    assert got["hit"][2] == 1 and got["poly"][2] >= 9 + n_cluster
    eng.check_async()


def test_constructions(eng, wl, scene):
    """One polygon 1025 times (every ray that reaches it is listed); a polygon that spans many cells and one with a NaN vertex
    among regular ones; a diagonal ray across the whole grid; rays wholly outside B's bounds."""
    n = 1025
    rays = cases.rays_of(*[(-1 - 0.25 * (i % 7), 0.125 * (i % 8) + 0.0625, 4 + (i % 5), 0) for i in range(300)],
                         *[(0.25 + 0.001 * i, 0.5, 0, 0) for i in range(50)], *[(5, 5, 1, 1)] * 3)
    same_poly = cases.polys(*[cases.UNIT] * n)
    got, stats = check(eng, rays, same_poly, "one square 1025 times", col_base=77)
    assert (got["hit"][:350] == 1).all() and (got["poly"][:350] == 77).all() and (got["hit"][350:] == 0).all()
    assert stats["listed"] == len(rays[0]), stats      # (one cell holds all 1025: every ray looks at it)
    # among the scene's 311 polygons: a triangle over the whole scene, a polygon with a NaN vertex whose clean edges are still hit, far outliers
    srays, b, want_clean = scene
    srays = tuple(r[:1000] for r in srays)
    vx, vy, k = (x.copy() for x in b)
    vx[:3, 5], vy[:3, 5], k[5] = (-60, 60, 0), (-55, -55, 70), 3
    vx[0, 11] = np.nan
    vx[:, 20] += F(5000.0)                                       # far from the others: the bounds grow
    vx[:, 21], vy[:, 21] = vx[:, 21] * F(300.0) + F(1e6), vy[:, 21] * F(300.0) + F(1e6)      # large and beyond the bounds: a regular outlier
    big = (vx, vy, k)
    extra = cases.rays_of((-70, -70, 140, 140), (-70, 70, 140, -140), (-300, 0, 600, 1),          # across the whole grid
                          (4990, -50, 30, 100), (0, 6000, 5, 5), (-900, -900, -5, 0), (1e4, 1e4, 0, 0),   # outside the bounds
                          (float(vx[1, 21]), float(vy[1, 21]), 0, 0),                                # on a vertex of the outlier
                          (float(vx[1, 20]), float(vy[1, 20]), 0, 0))                               # on a vertex of the far polygon
    all_rays = tuple(np.concatenate([a, e]) for a, e in zip(srays, extra))
    got, stats = check(eng, all_rays, big, "outsized, unboxed and far polygons")
    brute = ref.ray_casts(all_rays, big)
    assert got.tobytes() == brute.tobytes() or ref.same(got, brute).all()      # (nothing near-collinear here: the contracts agree)
    assert (got["poly"] == 5).sum() > 100 and got["poly"][-1] == 20 and got["poly"][-2] == 21 and got["hit"][-4] == 0
    assert stats["listed"] == 0 and stats["outliers"] == 1, stats
    eng.check_async()


def test_non_finite_and_huge_inputs(eng, wl, scene):
    """The scene at 1e-30 .. 1e30 (at 1e30 every ray is beyond 2^60 and is listed), with NaN / inf injected into rays and into
    vertices, and rays with an infinite direction."""
    rays, b, _ = scene
    rays = tuple(r[:1000] for r in rays)
    for scale in (1e30, 1e15, 1e10, 1e-10, 1e-30, 1e-42):
        sr, sb = tuple((r * F(scale)).astype(F) for r in rays), (b[0] * F(scale), b[1] * F(scale), b[2])
        got, stats = check(eng, sr, sb, f"scale {scale}")
        assert got.tobytes() == ref.ray_casts(sr, sb).tobytes() or ref.same(got, ref.ray_casts(sr, sb)).all()
        assert stats["listed"] == (1000 if scale == 1e30 else 0), (scale, stats)
        if scale in (1e15, 1e10, 1e-10):
            assert 0.3 < (got["hit"] == 1).mean() < 0.8
    nf_rays = tuple(wl.inject_non_finite(r[None, :].copy(), seed=7130 + p, frac=0.05)[0] for p, r in enumerate(rays))
    nf_b = (wl.inject_non_finite(b[0].copy(), seed=7140, frac=0.02), wl.inject_non_finite(b[1].copy(), seed=7141, frac=0.02), b[2])
    inf_dir = tuple(x.copy() for x in rays)
    inf_dir[2][::3], inf_dir[3][1::3] = np.inf, -np.inf
    huge = tuple(x.copy() for x in rays)
    huge[0][::4], huge[2][1::4] = F(2.0 ** 60), F(-2.0 ** 61)
    for name, (r, s) in {"non-finite rays": (nf_rays, b), "non-finite vertices": (rays, nf_b), "both": (nf_rays, nf_b),
                         "infinite directions": (inf_dir, b), "huge rays": (huge, b)}.items():
        got, stats = check(eng, r, s, name)
        assert (got["hit"] == 1).any() and (got["hit"] == 0).any(), name
        if name != "non-finite vertices":
            assert stats["listed"] > 100, (name, stats)
    eng.check_async()


def test_bad_vertex_count_in_the_middle(eng, scene):
    """Counts of 0, 17 and 255 in the middle of B: those polygons are in no hit, the others still win, and the error is reported by the
    next synchronise, once."""
    rays, b, want_clean = scene
    rays = tuple(r[:1000] for r in rays)
    k = b[2].copy()
    winners = np.unique(want_clean["poly"][:1000][want_clean["hit"][:1000] == 1])
    bad = winners[[len(winners) // 3, len(winners) // 2, 2 * len(winners) // 3]]
    k[bad] = (0, 17, 255)
    s = (b[0], b[1], k)
    want = gref.ray_casts(rays, s)
    assert not np.isin(want["poly"], bad).any() and (want["hit"] == 1).sum() > 300
    assert (want["poly"] != want_clean["poly"][:1000]).any()
    dr, ub = RaysOnDevice(eng, rays), Uploaded(eng, s)
    assert_same(cast_grid(eng, dr, 1000, ub.set, expect_error=True), want, "bad counts")
    dr.free()
    ub.free()
    eng.check_async()


def test_scenes_equal_the_brute_force_call_in_the_same_run(eng, wl):
    """The ray scene and the 4096-polygon sparse scene: the records of c2d_poly_ray_casts_grid are c2d_poly_ray_casts' bytes, and the
    reference's; the walk visits a small multiple of the candidates, not of the number of polygons."""
    for name, (rays, b) in {"ray scene": cases.ray_scene(wl), "sparse scene": gcases.sparse_scene(wl)}.items():
        n, n_b = len(rays[0]), b[0].shape[1]
        dr, ub = RaysOnDevice(eng, rays), Uploaded(eng, b)
        got = twice(eng, dr, n, ub.set, name)
        stats = eng.poly_ray_casts_grid_stats()
        brute = cast(eng, dr, n, ub.set)
        assert got.tobytes() == brute.tobytes(), f"{name}: differs from c2d_poly_ray_casts"
        assert_same(got, gref.ray_casts(rays, b), name)
        cand = int(gref.candidates(rays, b).sum())
        print(f"{name}: {n} rays x {n_b} polygons, {cand} candidates, {stats}")
        assert stats["listed"] == 0 and stats["candidates"] == cand, (stats, cand)
        assert stats["visited"] < 0.05 * n * n_b
        dr.free()
        ub.free()
    eng.check_async()


def test_argument_errors(eng, pkg, scene):
    """every refusal, with a ctx: status -1 before anything is enqueued, and the output untouched"""
    rays, b, _ = scene
    dr, ub = RaysOnDevice(eng, tuple(r[:64] for r in rays)), Uploaded(eng, b)
    d_out = eng.empty(66, DT)
    eng.memset(d_out, 0xA5, d_out.nbytes)
    out = d_out.ptr + 16
    lib, binding = eng.lib, pkg.binding
    planes = (C.c_void_p * 4)(*dr.ptrs)

    def status(planes=planes, n=64, s=ub.set, cb=0, o=out):
        return lib.c2d_poly_ray_casts_grid(eng.h, planes, n, None if s is None else C.byref(s), cb, C.c_void_p(o) if o is not None else None, None)

    assert status(planes=None) == -1 and status(s=None) == -1 and status(o=None) == -1
    assert status(planes=(C.c_void_p * 4)(dr.ptrs[0], 0, dr.ptrs[2], dr.ptrs[3])) == -1                   # a NULL plane
    assert status(planes=(C.c_void_p * 4)(dr.ptrs[0] + 2, *dr.ptrs[1:])) == -1                           # a plane off 4 bytes
    assert status(o=out + 8) == -1 and status(o=out + 4) == -1                                           # a misaligned output
    for rows in (0, 17):
        assert status(s=binding._PolySet(rows, 311, 0, ub.px, ub.py, ub.dk.ptr)) == -1
        assert status(s=binding._PolySet(rows, 0, 0, 0, 0, 0)) == -1
    assert status(s=binding._PolySet(16, 311, 310, ub.px, ub.py, ub.dk.ptr)) == -1                      # stride < n
    assert status(s=binding._PolySet(16, 311, 0, 0, ub.py, ub.dk.ptr)) == -1                            # a NULL vertex plane
    assert status(cb=(1 << 32) - 310) == -1 and status(cb=1 << 40) == -1                                 # col_base + n_b > 2^32
    assert status(n=(1 << 32) + 1) == -1
    assert b"c2d_poly_ray_casts_grid" in lib.c2d_last_error(eng.h)
    assert lib.c2d_poly_ray_casts_grid_stats(eng.h, None) == -1
    assert status(n=0, o=out + 8) == 0                                                                   # n_rays == 0: a no-op
    eng.synchronize()
    assert (d_out.get().view(np.uint8) == 0xA5).all()
    assert status(cb=(1 << 32) - 311) == 0                                                               # the largest col_base
    eng.synchronize()
    for x in (dr, ub, d_out):
        x.free()
    eng.check_async()


def test_graph_capture_in_a_child_process():
    """tests/best_key_graph_check.py ray_grid: a growing capture is refused; capture after an eager call, replay with changed rays and polygons"""
    out = subprocess.run([sys.executable, os.path.join(HERE, "best_key_graph_check.py"), "ray_grid"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "ray grid graph ok" in out.stdout


def test_fuzzer_configurations_at_a_fixed_seed(eng):
    """tests/tools/ray_grid_fuzz.py at a fixed seed, each configuration from its own stream (seed, index): sixteen configurations"""
    fz = best.load_tool("ray_grid_fuzz")
    compared = listed = 0
    for i in range(16):
        ok, (desc, n) = fz.one(eng, np.random.default_rng([FUZZ_SEED, i]), i)
        assert ok, desc
        compared += n
        listed += fz.LAST["listed"]
    assert compared > 1000 and listed > 0
    eng.check_async()
