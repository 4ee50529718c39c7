"""GPU tests of the ray queries (c2d_poly_ray_casts): every field of every record equals tests/ray_ref.py — the numpy restatement of
the contract of include/c2d.h, pinned by tests/test_ray_ref_cpu.py — t and u bit for bit (+0 and -0 equal), and `hit` also equals
the engine's own N x M polygon test on the segments as 2-gons.  Every output buffer handed to the library sits between guard bands
that are checked afterwards."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import best_key_harness as best  # noqa: E402
import contact_cases  # noqa: E402
import ray_cases as cases  # noqa: E402
import ray_ref as ref  # noqa: E402
from pair_list_harness import Uploaded  # noqa: E402
from ray_harness import RaysOnDevice, assert_same, cast, twice  # noqa: E402

pytestmark = pytest.mark.gpu
FUZZ_SEED = 20264
F = np.float32
@pytest.fixture(scope="module")
def long_scene(wl):
    """the ray scene's polygons with 4099 rays of the same generator, and their reference records, computed once"""
    rays, b = cases.ray_scene(wl, n_rays=4099)
    want = ref.ray_casts(rays, b)
    want.setflags(write=False)
    assert 0.3 < (want["hit"] == 1).mean() < 0.8 and 0.05 < (want["flags"] == ref.START_INSIDE).mean() < 0.3
    return rays, b, want


def test_every_number_of_rays(eng, long_scene):
    """0, 1, 63, 64, 65, 255, 256, 257, 1000 and 4099 rays against the scene's 311 polygons (five column tiles, one strip each)."""
    rays, b, want = long_scene
    ub, dr = Uploaded(eng, b), RaysOnDevice(eng, rays)
    for n in contact_cases.LIST_LENGTHS:
        got = cast(eng, dr, n, ub.set, capacity=max(n, 4))
        assert_same(got[:n], want[:n], f"{n} rays")
        assert best.strips_of(eng.info()["compute_units"], max(n, 1), 311) == 5
    eng.check_async()
    ub.free()
    dr.free()


def test_every_number_of_polygons(eng, wl, long_scene):
    """The first 257 rays against prefixes of the scene's polygons on both sides of every power-of-two tile up to 256, and against
    513 polygons from the same generator: one strip while B fits one tile, one strip per tile beyond."""
    rays, b, _ = long_scene
    rays = tuple(r[:257] for r in rays)
    dr = RaysOnDevice(eng, rays)
    more = wl.random_convex_polygon_set(513, seed=7103, kmin=3, kmax=16, extent=48.0, rows=16)
    seen = set()
    for n_b, s in [(n, b) for n in (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 311)] + [(513, more)]:
        sub = tuple(x[..., :n_b] for x in s)
        ub = Uploaded(eng, sub)
        want = ref.ray_casts(rays, sub)
        assert_same(twice(eng, dr, 257, ub.set, f"{n_b} polygons"), want, f"{n_b} polygons")
        seen.add(best.strips_of(eng.info()["compute_units"], 257, n_b))
        ub.free()
    assert {1, 2, 3, 4, 5, 9} <= seen
    eng.check_async()
    dr.free()


def test_both_sides_of_the_strip_rule(eng, long_scene):
    """Many rays: the scene's first 2000 rays repeated until the row tiles alone fill the device, so that every block walks all
    five column tiles of B in turn (one strip), and a number in between (several tiles per strip, several strips per row tile).
    The records repeat with the rays."""
    rays, b, want = long_scene
    cus = eng.info()["compute_units"]
    ub = Uploaded(eng, b)
    wanted = set()
    for row_tiles in (8 * cus + 3, 8 * cus // 3):
        reps = -(-row_tiles * best.TILE_ROWS // 2000)
        n = reps * 2000
        wanted.add(best.strips_of(eng.info()["compute_units"], n, 311))
        dr = RaysOnDevice(eng, tuple(np.tile(r[:2000], reps) for r in rays))
        got = cast(eng, dr, n, ub.set)
        dr.free()
        differs = np.flatnonzero(got.reshape(reps, 2000).view(np.uint8).reshape(reps, -1) != want[:2000].view(np.uint8)[None, :])
        if len(differs):     # (not the same bytes: +0 against -0 would still be the same record)
            assert_same(got, np.tile(want[:2000], reps), f"{n} rays")
    assert wanted == {1, 2} or (1 in wanted and len(wanted) == 2)
    eng.check_async()
    ub.free()


def test_layout_variants(eng, wl, long_scene):
    """rows 4, 8 and 16; k == rows with d_k == NULL; a plane offset and a stride larger than n; a pointer-offset shard of B with
    col_base; ray planes at odd 4-byte offsets; n_b == 0; n_rays == 0."""
    rays, b, _ = long_scene
    rays = tuple(r[:600] for r in rays)
    dr = RaysOnDevice(eng, rays, offsets=(1, 3, 0, 2))
    for rows in (4, 8, 16):
        s = wl.random_convex_polygon_set(200, seed=7110 + rows, kmin=3, kmax=rows, extent=48.0, rows=rows)
        ub = Uploaded(eng, s, offset=1, stride=200 + 7)
        assert_same(cast(eng, dr, 600, ub.set), ref.ray_casts(rays, s), f"rows {rows}")
        ub.free()
        full = wl.random_convex_polygon_set(130, seed=7120 + rows, kmin=rows, kmax=rows, extent=30.0, rows=rows)
        ub = Uploaded(eng, full, with_k=False)
        assert ub.dk is None
        want = ref.ray_casts(rays, full)
        assert (want["hit"] == 1).any()
        assert_same(cast(eng, dr, 600, ub.set), want, f"rows {rows}, d_k == NULL")
        ub.free()
    ub = Uploaded(eng, b, offset=3, stride=311 + 5)
    c0, c1, base = 37, 290, 4_000_000_000
    shard = tuple(x[..., c0:c1] for x in b)
    want = ref.ray_casts(rays, shard, col_base=base)
    assert (want["poly"][want["hit"] == 1] >= base).all()
    assert_same(cast(eng, dr, 600, ub.sub(c0, c1), col_base=base), want, "a shard of B with col_base")
    top = (1 << 32) - (c1 - c0)
    assert_same(cast(eng, dr, 600, ub.sub(c0, c1), col_base=top), ref.ray_casts(rays, shard, col_base=top), "col_base + n_b == 2^32")
    # n_b == 0: the no-hit record for every ray, with and without planes behind the empty set
    none = ref.ray_casts(rays, tuple(x[..., :0] for x in b))
    assert (none["hit"] == 0).all() and (none["poly"] == 0xFFFFFFFF).all()
    assert_same(cast(eng, dr, 600, ub.sub(5, 5)), none, "n_b == 0")
    assert_same(cast(eng, dr, 600, eng.poly_set(0, 0, None, 0, 16)), none, "n_b == 0, no planes")
    # n_rays == 0: nothing is touched (cast() checks every record at or beyond n_rays)
    cast(eng, dr, 0, ub.set, capacity=8)
    eng.check_async()
    ub.free()
    dr.free()


def test_order_independence_by_construction(eng):
    """1025 polygons are 17 column tiles, one strip each for a few rays: the winner is found by the atomic minimum over 17 blocks.
    One square 1025 times: the first wins for every ray.  The nearest obstacle last of 1025.  A ray through a vertex that two
    polygons in different tiles share.  Each case twice: the same bytes."""
    n = 1025
    rays = cases.rays_of(*[(-1 - 0.25 * (i % 7), 0.125 * (i % 8) + 0.0625, 4 + (i % 5), 0) for i in range(300)],
                         *[(0.25 + 0.001 * i, 0.5, 0, 0) for i in range(50)], *[(5, 5, 1, 1)] * 3)
    dr = RaysOnDevice(eng, rays)
    same = cases.polys(*[cases.UNIT] * n)
    ub = Uploaded(eng, same)
    want = ref.ray_casts(rays, same, col_base=77)
    assert (want["hit"][:350] == 1).all() and (want["poly"][:350] == 77).all() and (want["hit"][350:] == 0).all()
    assert_same(twice(eng, dr, len(rays[0]), ub.set, "duplicates", col_base=77), want, "one square 1025 times")
    ub.free()
    far_first = cases.polys(*[cases.square(2.0 + 0.001 * j, 0.0) for j in range(n - 1)], cases.UNIT)
    ub = Uploaded(eng, far_first)
    want = ref.ray_casts(rays, far_first)
    assert (want["poly"][:350] == n - 1).all()
    assert_same(twice(eng, dr, len(rays[0]), ub.set, "nearest last"), want, "the nearest obstacle last of 1025")
    ub.free()
    # polygons 3 and 900 share the vertex (1, 1); the ray from (0, 0) along (4, 4) reaches both at t = 1/4; everything else is far away
    filler = [cases.square(100.0 + j, 50.0) for j in range(n)]
    filler[3] = [(1, 1), (2, 1), (2, 0.5)]                  # below the diagonal
    filler[900] = [(1, 1), (0.5, 2), (1, 2)]                # above it
    shared = cases.polys(*filler)
    diag = cases.rays_of((0, 0, 4, 4), (0, 0, 2, 2), (0, 0, 1, 1), (0, 0, 0.5, 0.5))
    want = ref.ray_casts(diag, shared)
    assert cases.as_tuples(want[:1]) == [(3, 0.25, 0.0, 0, 1, 0)] and (want["poly"][:3] == 3).all() and want["hit"][3] == 0
    dd = RaysOnDevice(eng, diag)
    ub = Uploaded(eng, shared)
    assert_same(twice(eng, dd, 4, ub.set, "shared vertex"), want, "a vertex shared by polygons of two tiles")
    ub.free()
    dd.free()
    dr.free()
    eng.check_async()


@pytest.mark.parametrize("name", sorted(cases.hand_cases()))
def test_hand_cases(eng, name):
    rays, b, want = cases.hand_cases()[name]
    dr, ub = RaysOnDevice(eng, rays), Uploaded(eng, b)
    got = cast(eng, dr, len(rays[0]), ub.set)
    assert cases.as_tuples(got) == [tuple(w) for w in want], name
    assert_same(got, ref.ray_casts(rays, b), name)
    dr.free()
    ub.free()
    eng.check_async()


def test_non_finite_and_huge_inputs(eng, wl, long_scene):
    """The scene at 1e30 (every product overflows or nearly), at 1e-30 and 1e-42 (subnormal products), with NaN / inf injected into
    rays and into vertices, and rays with an infinite direction (a usable edge then has u = inf / inf)."""
    rays, b, base = long_scene
    rays = tuple(r[:1000] for r in rays)
    for scale in (1e30, 1e18, 1e-18, 1e-30, 1e-42):
        sr, sb = tuple((r * F(scale)).astype(F) for r in rays), (b[0] * F(scale), b[1] * F(scale), b[2])
        want = ref.ray_casts(sr, sb)
        dr, ub = RaysOnDevice(eng, sr), Uploaded(eng, sb)
        assert_same(cast(eng, dr, 1000, ub.set), want, f"scale {scale}")
        dr.free()
        ub.free()
        if scale in (1e18, 1e-18):
            assert 0.3 < (want["hit"] == 1).mean() < 0.8
    nf_rays = tuple(wl.inject_non_finite(r[None, :].copy(), seed=7130 + p, frac=0.05)[0] for p, r in enumerate(rays))
    nf_b = (wl.inject_non_finite(b[0].copy(), seed=7140, frac=0.02), wl.inject_non_finite(b[1].copy(), seed=7141, frac=0.02), b[2])
    inf_dir = tuple(x.copy() for x in rays)
    inf_dir[2][::3], inf_dir[3][1::3] = np.inf, -np.inf
    for name, (r, s) in {"non-finite rays": (nf_rays, b), "non-finite vertices": (rays, nf_b), "both": (nf_rays, nf_b), "infinite directions": (inf_dir, b)}.items():
        want = ref.ray_casts(r, s)
        assert (want["hit"] == 1).any() and (want["hit"] == 0).any(), name
        dr, ub = RaysOnDevice(eng, r), Uploaded(eng, s)
        assert_same(cast(eng, dr, 1000, ub.set), want, name)
        dr.free()
        ub.free()
    assert np.isnan(ref.ray_casts(inf_dir, b)["u"]).any()
    eng.check_async()


def test_bad_vertex_count_in_the_middle(eng, long_scene):
    """Counts of 0, 17 and 255 in the middle of B: those polygons are in no hit, the others still win, and the error is reported by the
    next synchronise, once."""
    rays, b, want_clean = long_scene
    rays = tuple(r[:1000] for r in rays)
    k = b[2].copy()
    winners = np.unique(want_clean["poly"][:1000][want_clean["hit"][:1000] == 1])
    bad = winners[[len(winners) // 3, len(winners) // 2, 2 * len(winners) // 3]]
    k[bad] = (0, 17, 255)
    s = (b[0], b[1], k)
    want = ref.ray_casts(rays, s)
    assert not np.isin(want["poly"], bad).any() and (want["hit"] == 1).sum() > 300
    assert (want["poly"] != want_clean["poly"][:1000]).any()
    dr, ub = RaysOnDevice(eng, rays), Uploaded(eng, s)
    assert_same(cast(eng, dr, 1000, ub.set, expect_error=True), want, "bad counts")
    dr.free()
    ub.free()
    eng.check_async()


def test_against_the_engine_itself(eng, wl):
    """On the ray scene, `hit` is the OR over each row of c2d_sat_poly_cross_mask with the segments as 2-gons, and `poly` of every
    hit ray is a set bit of that row."""
    rays, b = cases.ray_scene(wl)
    segs = cases.segments_as_2gons(rays)
    dr, ub, us = RaysOnDevice(eng, rays), Uploaded(eng, b), Uploaded(eng, segs)
    got = cast(eng, dr, 2000, ub.set)
    words = (311 + 63) // 64
    d_mask = eng.zeros((2000, words), np.uint64)
    eng.sat_poly_cross_mask(us.set, ub.set, d_mask)
    eng.synchronize()
    mask = d_mask.get()
    bits = np.unpackbits(mask.view(np.uint8).reshape(2000, -1), axis=1, bitorder="little")[:, :311].astype(bool)
    assert np.array_equal(bits.any(axis=1), got["hit"] == 1)
    rows = np.flatnonzero(got["hit"] == 1)
    assert len(rows) > 500 and bits[rows, got["poly"][rows]].all()
    for x in (dr, ub, us, d_mask):
        x.free()
    eng.check_async()


def test_argument_errors(eng, pkg, long_scene):
    """every refusal, with a ctx: status -1 before anything is enqueued, and the output untouched"""
    rays, b, _ = long_scene
    dr, ub = RaysOnDevice(eng, tuple(r[:64] for r in rays)), Uploaded(eng, b)
    d_out = eng.empty(66, ref.RAY_HIT_DT)
    eng.memset(d_out, 0xA5, d_out.nbytes)
    out = d_out.ptr + 16
    lib, binding = eng.lib, pkg.binding
    planes = (C.c_void_p * 4)(*dr.ptrs)

    def status(planes=planes, n=64, s=ub.set, cb=0, o=out):
        return lib.c2d_poly_ray_casts(eng.h, planes, n, None if s is None else C.byref(s), cb, C.c_void_p(o) if o is not None else None, None)

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
    assert b"c2d_poly_ray_casts" in lib.c2d_last_error(eng.h)
    assert status(n=0, o=out + 8) == 0                                                                   # n_rays == 0: a no-op
    eng.synchronize()
    assert (d_out.get().view(np.uint8) == 0xA5).all()
    assert status(cb=(1 << 32) - 311) == 0                                                               # the largest col_base
    eng.synchronize()
    for x in (dr, ub, d_out):
        x.free()
    eng.check_async()


def test_graph_capture_in_a_child_process():
    """tests/best_key_graph_check.py ray: capture the call, replay with changed rays and polygons"""
    out = subprocess.run([sys.executable, os.path.join(HERE, "best_key_graph_check.py"), "ray"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "ray graph ok" in out.stdout


def test_fuzzer_configurations_at_a_fixed_seed(eng):
    """tests/tools/ray_fuzz.py at a fixed seed, each configuration from its own stream (seed, index): sixteen configurations"""
    fz = best.load_tool("ray_fuzz")
    compared = 0
    for i in range(16):
        ok, (desc, n) = fz.one(eng, np.random.default_rng([FUZZ_SEED, i]), i)
        assert ok, desc
        compared += n
    assert compared > 1000
    eng.check_async()
