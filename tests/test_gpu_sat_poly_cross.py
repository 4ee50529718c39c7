"""GPU tests of the all-pairs convex polygon entry points (c2d_sat_poly_cross_mask / _pairs): result (i, j) must be the boolean of
the pairwise polygon path on (A_i, B_j), bit for bit.  The reference materialises the pairs (np.repeat / np.tile, chunks of at most
1e6 pairs) and runs the CPU oracle on them up to a few million pairs; above that the same pairs go through the pairwise GPU kernel
(c2d_sat_poly_pairs_rows, itself pinned to the oracle by test_gpu_sat.py) in chunks (tests/sat_cross_harness.py).  Never the code under
test.  Every mask and list buffer handed to the library sits between guard rows that are checked afterwards (run_mask there, run
of tests/pair_search_harness.py)."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pair_search_harness as psh
from pair_search_harness import SENTINEL, DeviceSet
from sat_cross_harness import check_mask, degenerate_set, mask_bits, reference, run_mask, touching_sets

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PKG_DIR = os.path.join(os.path.dirname(HERE), "convex-2d-gpu-collision-detection_amd")
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000, 4099]
FUZZ_SEED = 2026


@pytest.fixture(scope="module")
def big_sets(eng, oracle, wl):
    """A and B of 4099 polygons each, K ~ U{3..16}, extent 40, with the full reference"""
    a, b = wl.random_convex_polygon_set(4099, seed=11, extent=40.0), wl.random_convex_polygon_set(4099, seed=12, extent=40.0)
    return a, b, reference(eng, oracle, a, b)


def test_shape_of_the_call(eng, big_sets):
    """Every size pair of 1, 63, 64, 65, 255, 256, 257, 1000, 4099, planes shifted by 0 to 3 floats, stride > n on every other set,
    every other call on a stream of its own: the mask is the reference's prefix block, the tail bits are 0, the count its popcount."""
    a, b, ref = big_sets
    assert 0.001 < ref.mean() < 0.01, ref.mean()   # (the oracle's rate at extent 40 is 0.28 %: not an all-zero scene)
    s = eng.stream_create()
    try:
        for ia, n_a in enumerate(SIZES):
            for ib, n_b in enumerate(SIZES):
                sa = tuple(x[..., :n_a] for x in a)
                sb = tuple(x[..., :n_b] for x in b)
                ua = DeviceSet(eng, sa, offset=(ia + ib) % 4, stride=n_a + (7 if (ia + ib) % 2 else 0))
                ub = DeviceSet(eng, sb, offset=(ia + 2 * ib + 1) % 4, stride=n_b + (5 if ib % 2 else 0))
                m, c = run_mask(eng, ua.set, ub.set, stream=s if (ia + ib) % 2 else 0)
                want = ref[:n_a, :n_b]
                bits = np.unpackbits(m.view(np.uint8), bitorder="little", axis=-1).reshape(n_a, -1)
                assert np.array_equal(bits[:, :n_b].astype(bool), want), (n_a, n_b)
                assert not bits[:, n_b:].any(), (n_a, n_b)
                assert c == int(want.sum()), (n_a, n_b)
                ua.free()
                ub.free()
    finally:
        eng.stream_destroy(s)
    eng.check_async()


def test_layout_padding_words_untouched(eng, oracle, wl):
    n_a, n_b = 300, 1000
    a, b = wl.random_convex_polygon_set(n_a, seed=21, extent=8.0), wl.random_convex_polygon_set(n_b, seed=22, extent=8.0)
    ref = reference(eng, oracle, a, b)
    assert 0.02 < ref.mean() < 0.15
    ua, ub = DeviceSet(eng, a), DeviceSet(eng, b)
    words = (n_b + 63) // 64
    m, c = run_mask(eng, ua.set, ub.set, ld=words + 3)
    assert (m[:, words:] == SENTINEL).all(), "padding words were written"
    bits = np.unpackbits(m[:, :words].copy().view(np.uint8), bitorder="little", axis=-1).reshape(n_a, -1)
    assert not bits[:, n_b:].any(), "tail bits j >= n_b are not 0"
    assert np.array_equal(bits[:, :n_b].astype(bool), ref) and c == int(ref.sum())
    ua.free()
    ub.free()


def test_upper_mode_and_shards(eng, oracle, wl):
    """One set against itself: a symmetric full mask with an all-ones diagonal that equals the oracle, the strict upper triangle,
    (full - n) / 2 pairs counted; row shards (pointer offset + stride, row_base) and column tiles (col_base) reproduce it."""
    n = 1000
    s = wl.random_convex_polygon_set(n, seed=31, extent=8.0)
    us = DeviceSet(eng, s, offset=1, stride=n + 3)
    full, full_c = run_mask(eng, us.set, us.set)
    full_bits = mask_bits(full, n)
    assert np.array_equal(full_bits, reference(eng, oracle, s, s))
    assert np.array_equal(full_bits, full_bits.T), "the test is symmetric"
    assert full_c == int(full_bits.sum()) and full_bits.diagonal().all() and full_c > 3 * n
    up, up_c = run_mask(eng, us.set, us.set, upper=True)
    up_bits = mask_bits(up, n)
    tri = np.triu(np.ones((n, n), bool), 1)
    assert not up_bits[~tri].any(), "bits on or below the diagonal"
    assert np.array_equal(up_bits[tri], full_bits[tri])
    assert up_c == int(up_bits.sum()) == (full_c - n) // 2
    cut = 389
    parts = []
    for r0, r1 in ((0, cut), (cut, n)):
        m, c = run_mask(eng, us.sub(r0, r1), us.set, upper=True, row_base=r0)
        parts.append(m)
        assert c == int(mask_bits(m, n).sum())
    assert np.array_equal(np.concatenate(parts), up)
    m, _ = run_mask(eng, us.set, us.sub(448, n), upper=True, col_base=448)
    assert np.array_equal(mask_bits(m, n - 448), up_bits[:, 448:])
    r0, c0, nr, nc = 301, 517, 200, 333   # an off-grid block
    m, c = run_mask(eng, us.sub(r0, r0 + nr), us.sub(c0, c0 + nc), upper=True, row_base=r0, col_base=c0)
    assert np.array_equal(mask_bits(m, nc), up_bits[r0:r0 + nr, c0:c0 + nc]) and c == int(up_bits[r0:r0 + nr, c0:c0 + nc].sum())
    m, _ = run_mask(eng, us.sub(r0, r0 + nr), us.sub(c0, c0 + nc), row_base=r0, col_base=c0)
    assert np.array_equal(mask_bits(m, nc), full_bits[r0:r0 + nr, c0:c0 + nc])
    us.free()
    eng.check_async()


def test_diagonal_identity(eng, wl):
    """For a padded pair batch, mask[i][i] of (its A half) x (its B half) — two sets made of the batch's own memory through
    `stride`, no copy — equals c2d_sat_poly_pairs on the batch."""
    n = 12_000
    vx, vy, k = wl.random_convex_polygons(n, seed=41, extent=3.0)
    d_vx, d_vy, d_k = eng.to_device(vx), eng.to_device(vy), eng.to_device(k)
    d_out = eng.zeros(n, np.uint8)
    eng.sat_poly_pairs(d_vx, d_vy, d_k, n, d_out)
    pairwise = d_out.get().astype(bool)
    assert 0.1 < pairwise.mean() < 0.9
    half = 4 * wl.KMAX * n
    a = eng.poly_set(d_vx.ptr, d_vy.ptr, d_k.ptr, n, wl.KMAX, n)
    b = eng.poly_set(d_vx.ptr + half, d_vy.ptr + half, d_k.ptr + n, n, wl.KMAX, n)
    m, _ = run_mask(eng, a, b)
    assert np.array_equal(mask_bits(m, n).diagonal(), pairwise)
    for x in (d_vx, d_vy, d_k, d_out):
        x.free()


def test_mixed_layouts(eng, oracle, wl):
    """rows 4, 8, 12, 16 on either side in every combination, d_k == NULL on either side, clockwise polygons."""
    n = 300
    total = 0
    for ra in (4, 8, 12, 16):
        for rb in (4, 8, 12, 16):
            a = wl.random_convex_polygon_set(n, seed=50 + ra, kmin=min(3, ra), kmax=ra, extent=5.0, rows=ra)
            b = wl.random_convex_polygon_set(n, seed=70 + rb, kmin=min(3, rb), kmax=rb, extent=5.0, rows=rb)
            total += int(check_mask(eng, oracle, a, b, offsets=((ra % 4, rb % 3),)).sum())
    assert total > 0.05 * 16 * n * n
    # every polygon has exactly `rows` vertices: no count plane on A, on B, on both
    a = wl.random_convex_polygon_set(400, seed=91, kmin=8, kmax=8, extent=5.0, rows=8)
    b = wl.random_convex_polygon_set(500, seed=92, kmin=12, kmax=12, extent=5.0, rows=12)
    c = wl.random_convex_polygon_set(500, seed=93, extent=5.0)
    for x, y in ((a, c), (c, b), (a, b)):
        ref = reference(eng, oracle, x, y)
        assert ref.mean() > 0.05
        nx = (x[0], x[1], None) if x is not c else x
        ny = (y[0], y[1], None) if y is not c else y
        check_mask(eng, oracle, nx, ny, ref=ref)
    # clockwise polygons (inward-pointing (-ey, ex)) against counter-clockwise ones and against themselves
    rng = np.random.default_rng(94)
    m = 500
    vx, vy, k = np.zeros((16, m), np.float32), np.zeros((16, m), np.float32), rng.integers(3, 17, m).astype(np.uint8)
    for q in range(m):
        xs, ys = wl.convex_polygon(int(k[q]), rng, rng.uniform(0.3, 2.5), rng.uniform(0.3, 2.5), rng.uniform(0, 6.28), clockwise=True)
        vx[:k[q], q], vy[:k[q], q] = xs + np.float32(rng.uniform(-5, 5)), ys + np.float32(rng.uniform(-5, 5))
    cw = (vx, vy, k)
    for x, y in ((cw, c), (c, cw), (cw, cw)):
        assert check_mask(eng, oracle, x, y).mean() > 0.05


def test_degenerate_and_touching(eng, oracle, wl):
    n = 1200
    a, b = degenerate_set(wl, n, 101), degenerate_set(wl, n, 102)
    ref = check_mask(eng, oracle, a, b)
    assert 0.05 < ref.mean() < 0.95
    pts = np.flatnonzero(a[2] == 1)
    assert ref[pts][:, b[2] == 1].all(), "two points read 'collide' (their only axis is the zero vector)"
    ta, tb = touching_sets(1000)
    ref = check_mask(eng, oracle, ta, tb)
    assert ref.diagonal().all(), "pairs that share an edge or a vertex touch: strict < does not separate them"
    assert 0.0005 < ref.mean() < 0.02


@pytest.mark.parametrize("scale", [1e-30, 1e30, 1e-42])
def test_extreme_scales(eng, oracle, wl, scale):
    """Coordinates around 1e-30 and 1e30 and denormal ones (1e-42: every coordinate below 2^-126)."""
    n = 1200
    out = []
    for seed in (111, 112):
        vx, vy, k = wl.random_convex_polygon_set(n, seed=seed, extent=4.0)
        out.append(((vx.astype(np.float64) * scale).astype(np.float32), (vy.astype(np.float64) * scale).astype(np.float32), k))
    if scale < 1e-38:
        assert (np.abs(out[0][0][out[0][0] != 0]) < 1.2e-38).all()
    ref = check_mask(eng, oracle, *out)
    assert ref.mean() > (0.02 if scale > 1e-38 else 0.0)


def test_non_finite_vertices(eng, oracle, wl):
    """NaN / inf / +-3e38 coordinates, a NaN at vertex 0 (every pair of that polygon reads 'collide') and at a later vertex."""
    n = 1100
    a, b = wl.random_convex_polygon_set(n, seed=121, extent=3.0), wl.random_convex_polygon_set(n, seed=122, extent=3.0)
    fin = reference(eng, oracle, a, b)

    def inject(s, seed):
        both = wl.inject_non_finite(np.concatenate([s[0], s[1]]), seed=seed, frac=0.2)
        return both[:16].copy(), both[16:].copy(), s[2]

    a, b = inject(a, 123), inject(b, 124)
    a[0][0, 10:20] = np.nan          # x of vertex 0 of A_10 .. A_19
    a[1][2, 30:40] = np.nan          # y of vertex 2 of A_30 .. A_39
    b[1][0, 50:60] = np.nan          # y of vertex 0 of B_50 .. B_59
    b[0][1, 70:80] = np.nan          # x of vertex 1 of B_70 .. B_79
    ref = check_mask(eng, oracle, a, b)
    assert (ref != fin).mean() > 0.01, "the injected values no longer change results"
    assert ref[10:20].all(), "a NaN at vertex 0 of A reads 'collide' with every B"
    assert ref[:, 50:60].all(), "a NaN at vertex 0 of B reads 'collide' with every A"


def test_dense_scene(eng, oracle, wl):
    n = 1500
    a, b = wl.random_convex_polygon_set(n, seed=131, extent=0.8), wl.random_convex_polygon_set(n, seed=132, extent=0.8)
    ref = check_mask(eng, oracle, a, b, offsets=((2, 1),))
    assert ref.mean() > 0.5, ref.mean()


def test_out_of_range_counts(eng, pkg, oracle, wl):
    """Counts 0, rows + 1 and 255 in A, in B and in both: those rows / columns are all 0 and uncounted, every other bit equals the
    reference (computed from the valid polygons only: the oracle refuses such counts), and the error is reported once by the
    next synchronise and then is clear."""
    n_a, n_b = 700, 900
    a, b = wl.random_convex_polygon_set(n_a, seed=141, kmax=12, extent=6.0, rows=12), wl.random_convex_polygon_set(n_b, seed=142, extent=6.0)
    bad_a, bad_b = np.array([0, 5, 63, 64, 300, 699]), np.array([1, 64, 255, 256, 511, 899])
    ka, kb = a[2].copy(), b[2].copy()
    ka[bad_a] = [0, 13, 255, 0, 16, 200]
    kb[bad_b] = [0, 17, 255, 0, 17, 100]
    ref = reference(eng, oracle, a, b)   # (every polygon with its valid count)
    assert ref.mean() > 0.02
    eng.check_async()
    words = (n_b + 63) // 64
    for which in ("a", "b", "both"):
        ua = DeviceSet(eng, (a[0], a[1], ka if which != "b" else a[2]))
        ub = DeviceSet(eng, (b[0], b[1], kb if which != "a" else b[2]))
        want = ref.copy()
        if which != "b":
            want[bad_a] = False
        if which != "a":
            want[:, bad_b] = False
        d_mask = eng.empty((n_a + 2, words), np.uint64)
        eng.memset(d_mask, 0xA5, d_mask.nbytes)
        d_cnt = eng.zeros(1, np.uint64)
        eng.sat_poly_cross_mask(ua.set, ub.set, d_mask.ptr + 8 * words, count=d_cnt)
        with pytest.raises(pkg.C2DError):
            eng.synchronize()
        eng.synchronize()
        eng.check_async()   # reported once, then clear
        m = d_mask.get()
        assert (m[0] == SENTINEL).all() and (m[-1] == SENTINEL).all()
        got = mask_bits(m[1:-1], n_b)
        assert np.array_equal(got, want) and int(d_cnt.get()[0]) == int(want.sum())
        # the list form counts and emits the same pairs
        p, c = psh.run(eng, psh.poly_cross(eng, ua, ub), int(want.sum()), absent=True)
        eng.check_async()
        assert psh.compare(p, c, np.argwhere(want)) is None
        for x in (d_mask, d_cnt, ua, ub):
            x.free()


def test_pair_list(eng, oracle, wl):
    """The list equals np.argwhere(mask) + (row_base, col_base) in the same order, full and upper; a capacity below the count
    gives exactly the row-major prefix with nothing written behind it and the full total; the same call twice gives the same
    bytes; a count-only call; the host convenience."""
    n_a, n_b = 700, 2100
    a, b = wl.random_convex_polygon_set(n_a, seed=151, extent=8.0), wl.random_convex_polygon_set(n_b, seed=152, extent=8.0, rows=16)
    ref = reference(eng, oracle, a, b)
    ua, ub = DeviceSet(eng, a, offset=2, stride=n_a + 9), DeviceSet(eng, b, offset=1)
    for upper, rb, cb in ((False, 0, 0), (False, 1000, 77), (True, 0, 0), (True, 500, 100)):
        m, total = run_mask(eng, ua.set, ub.set, upper=upper, row_base=rb, col_base=cb)
        bits = mask_bits(m, n_b)
        if not upper:
            assert np.array_equal(bits, ref)
        else:
            assert np.array_equal(bits, ref & ((np.arange(n_b)[None, :] + cb) > (np.arange(n_a)[:, None] + rb)))
        want = (np.argwhere(bits) + (rb, cb)).astype(np.uint32)
        assert total == len(want) and total > 1000
        call = psh.poly_cross(eng, ua, ub, upper, rb, cb)
        p, c = psh.run(eng, call, total)            # (run checks the guard entries in front of the list and past the capacity)
        assert c == total and np.array_equal(p, want)
        cap = total // 3 + 1
        p, c = psh.run(eng, call, cap)
        assert c == total and np.array_equal(p, want[:cap])
        p2, _ = psh.run(eng, call, cap)
        assert p.tobytes() == p2.tobytes()
    d_cnt = eng.zeros(1, np.uint64)
    eng.sat_poly_cross_pairs(ua.set, ub.set, None, 0, d_cnt)   # capacity 0 with no buffer: a count-only call
    assert int(d_cnt.get()[0]) == int(ref.sum())
    d_cnt.free()
    got = eng.poly_cross_pairs_host(*a, *b)
    assert got.dtype == np.uint32 and np.array_equal(got, np.argwhere(ref).astype(np.uint32))
    got = eng.poly_cross_pairs_host(*a, *a, upper=True)
    assert np.array_equal(got, np.argwhere(np.triu(reference(eng, oracle, a, a), 1)).astype(np.uint32))
    ua.free()
    ub.free()
    eng.check_async()


def test_pair_list_several_passes(eng, oracle, wl):
    """A row of 2^23 + 1 columns takes just over 1 MiB of mask, so the 256-MiB scratch holds 255 rows per pass: 600 rows run in
    three passes, and the running base carried on the device between them must keep the order.  B is a 4099-polygon block
    (triangles and quadrilaterals in 4 rows) repeated."""
    n_a, n_b, blk = 600, (1 << 23) + 1, 4099
    a = wl.random_convex_polygon_set(n_a, seed=161, extent=3.0)
    bb = wl.random_convex_polygon_set(blk, seed=162, kmax=4, extent=300.0, rows=4)
    reps = n_b // blk + 1
    b = (np.tile(bb[0], (1, reps))[:, :n_b], np.tile(bb[1], (1, reps))[:, :n_b], np.tile(bb[2], reps)[:n_b])
    ua, ub = DeviceSet(eng, a), DeviceSet(eng, b)
    ref_block = reference(eng, oracle, a, bb)
    per_row = ref_block.sum(1) * (n_b // blk) + ref_block[:, : n_b % blk].sum(1)
    total = int(per_row.sum())
    assert total > 10_000
    p, c = psh.run(eng, psh.poly_cross(eng, ua, ub), total)
    assert c == total
    p = p.astype(np.int64)
    assert np.array_equal(np.bincount(p[:, 0], minlength=n_a), per_row)
    assert (np.diff(p[:, 0] * n_b + p[:, 1]) > 0).all(), "not in row-major order"
    assert ref_block[p[:, 0], p[:, 1] % blk].all()
    ua.free()
    ub.free()
    eng.check_async()


def test_argument_errors(eng, pkg, wl):
    a = wl.random_convex_polygon_set(100, seed=5, extent=3.0)
    ua = DeviceSet(eng, a)
    d_mask = eng.zeros((100, 4), np.uint64)
    d_cnt = eng.zeros(1, np.uint64)
    S = ua.set
    mk = lambda **kw: eng.poly_set(kw.get("vx", ua.px), kw.get("vy", ua.py), ua.dk, kw.get("n", 100), kw.get("rows", 16), kw.get("stride", 0))  # noqa: E731
    eng.sat_poly_cross_mask(mk(n=0), S, d_mask)          # n_a == 0: a no-op
    eng.sat_poly_cross_mask(S, mk(n=0), d_mask)          # n_b == 0: a no-op
    eng.sat_poly_cross_pairs(mk(n=0), S, None, 0, None)
    raw = eng.lib.c2d_sat_poly_cross_mask
    assert raw(eng.h, None, C.byref(S), 0, 0, 0, d_mask.ptr, 2, None, None) == -1                  # NULL set
    assert raw(eng.h, C.byref(S), None, 0, 0, 0, d_mask.ptr, 2, None, None) == -1
    assert raw(eng.h, C.byref(S), C.byref(S), 0, 0, 2, d_mask.ptr, 2, None, None) == -1            # unknown flag
    assert raw(eng.h, C.byref(S), C.byref(S), 0, 0, -1, d_mask.ptr, 2, None, None) == -1
    assert eng.lib.c2d_sat_poly_cross_pairs(eng.h, None, C.byref(S), 0, 0, 0, None, 0, d_cnt.ptr, None) == -1
    bad = [
        lambda: eng.sat_poly_cross_mask(mk(vx=0), S, d_mask),                                        # a NULL plane
        lambda: eng.sat_poly_cross_mask(S, mk(vy=0), d_mask),
        lambda: eng.sat_poly_cross_mask(mk(rows=0), S, d_mask),                                      # rows 0 or 17
        lambda: eng.sat_poly_cross_mask(S, mk(rows=17), d_mask),
        lambda: eng.sat_poly_cross_mask(mk(stride=99), S, d_mask),                                   # stride < n
        lambda: eng.sat_poly_cross_mask(S, S, d_mask.ptr + 4),                                       # mask not 8-byte aligned
        lambda: eng.sat_poly_cross_mask(S, S, None),
        lambda: eng.sat_poly_cross_mask(S, S, d_mask, ld_words=1),                                   # ld_words < ceil(n_b / 64)
        lambda: eng.sat_poly_cross_pairs(S, S, d_mask, 10, None),                                    # no count
        lambda: eng.sat_poly_cross_pairs(S, S, None, 10, d_cnt),                                     # no buffer
        lambda: eng.sat_poly_cross_pairs(mk(rows=17), S, d_mask, 10, d_cnt),
        lambda: eng.sat_poly_cross_pairs(S, S, d_mask, 10, d_cnt, row_base=(1 << 32) - 99),          # row index 2^32
        lambda: eng.sat_poly_cross_pairs(S, S, d_mask, 10, d_cnt, col_base=(1 << 32) - 50),
    ]
    for q, call in enumerate(bad):
        with pytest.raises(pkg.C2DError) as e:
            call()
        assert e.value.status == -1, q
    # the largest bases the u32 list allows are accepted
    eng.sat_poly_cross_pairs(S, S, d_mask, 10, d_cnt, row_base=(1 << 32) - 100, col_base=(1 << 32) - 100)
    eng.synchronize()
    eng.check_async()
    for x in (d_mask, d_cnt):
        x.free()
    ua.free()


@pytest.mark.parametrize("k", [1, 2])
def test_fused_validation_builds_match_their_own_pairwise_kernel(eng, pkg, oracle, wl, k):
    """libc2d_fmad{1,2}.so: the N x M mask equals the pairwise polygon kernel OF THAT BUILD on the same pairs (the hoisted
    quantities contract exactly as the pair kernel's do)."""
    fe = pkg.Engine(0, lib_path=os.path.join(PKG_DIR, "lib", f"libc2d_fmad{k}.so"))
    try:
        a, b = wl.random_convex_polygon_set(600, seed=171, extent=4.0), wl.random_convex_polygon_set(700, seed=172, extent=4.0, rows=16)
        ref = reference(eng, oracle, a, b, force_gpu=True, fe=fe)
        assert 0.05 < ref.mean() < 0.9
        ua, ub = DeviceSet(fe, a, offset=1), DeviceSet(fe, b)
        m, c = run_mask(fe, ua.set, ub.set)
        assert np.array_equal(mask_bits(m, ub.n), ref) and c == int(ref.sum())
        ua.free()
        ub.free()
    finally:
        fe.close()


def test_mask_form_graph_capture():
    """One capture of the mask form on a single stream, replayed three times: the same mask and count as the eager call
    (tests/poly_cross_graph_check.py, its own process: torch has to be imported before libc2d.so)."""
    out = subprocess.run([sys.executable, os.path.join(HERE, "poly_cross_graph_check.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "poly cross graph ok" in out.stdout


def test_fuzzer_configurations_at_a_fixed_seed(eng, oracle):
    """tests/tools/poly_cross_fuzz.py at a fixed seed, each configuration from its own stream (seed, index): sixteen configurations, chosen
    so that they hold what the tool is for — the upper triangle with unequal bases, a list capacity below the total, a count-only call,
    A and B the same memory, non-finite real vertices, ld_words beyond the row's words, a vertex count out of range, d_k == NULL"""
    spec = importlib.util.spec_from_file_location("poly_cross_fuzz", os.path.join(HERE, "tools", "poly_cross_fuzz.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    seen, compared = [], 0
    for i in range(16):
        ok, (desc, n) = fz.one(eng, np.random.default_rng([FUZZ_SEED, i]), i, None, oracle)
        assert ok, desc
        seen.append(desc)
        compared += n
    assert any(re.search(r"upper True, bases \d+, \d+ \(unequal\)", d) for d in seen), seen           # a shifted diagonal
    assert any("below the total" in d for d in seen) and any("count-only list call" in d for d in seen), seen
    assert any("the same memory" in d for d in seen) and any("non-finite" in d for d in seen), seen
    assert any(re.search(r"ld_words \d+ > words", d) for d in seen), seen
    assert any(re.search(r"bad count in (A|B|both)", d) for d in seen) and any(re.search(r"d_k (NULL /|\w+ / NULL)", d) for d in seen), seen
    assert compared > 1000
    eng.check_async()
