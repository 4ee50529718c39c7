"""GPU tests of the distance queries (c2d_poly_pair_distances / c2d_rect_pair_distances): every field of every record equals
tests/distance_ref.py — the numpy restatement of the contract of include/c2d.h, pinned by tests/test_distance_ref_cpu.py — floats
bit for bit (+0 and -0 equal), and `hit` also equals the pairwise GPU path.  Every output buffer handed to the library sits between
guard bands that are checked afterwards."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import contact_cases as cases  # noqa: E402
import distance_ref as ref  # noqa: E402
import test_gpu_contacts as base  # noqa: E402   (the uploads, the pairwise GPU path)

pytestmark = pytest.mark.gpu
GUARD = 4            # guard records in front of and behind every output
BAND = 0xA5
FUZZ_SEED = 20263
Uploaded, RectsOnDevice, local, pairwise_gpu = base.Uploaded, base.RectsOnDevice, base.local, base.pairwise_gpu


def run(eng, call, pairs, capacity=None, n_dev=None, expect_error=False):
    """call(d_pairs, capacity, d_out, d_n) queues the distances call.  -> DISTANCE_DT[capacity]: the output, taken from between two
    guard bands that must be intact; every record at or beyond min(capacity, n_dev) must be untouched as well (it reads as BAND bytes)."""
    cap = len(pairs) if capacity is None else capacity
    host_pairs = np.full((max(cap, 1), 2), 0xFFFFFFFF, np.uint32)   # entries beyond the list: indices no set has
    host_pairs[:len(pairs)] = pairs
    d_pairs = eng.to_device(host_pairs)
    d_out = eng.empty(cap + 2 * GUARD, ref.DISTANCE_DT)
    eng.memset(d_out, BAND, d_out.nbytes)
    d_n = None if n_dev is None else eng.to_device(np.array([n_dev], np.uint64))
    try:
        call(d_pairs, cap, d_out.ptr + 32 * GUARD, d_n)
        if expect_error:
            with pytest.raises(Exception) as e:
                eng.synchronize()
            assert getattr(e.value, "status", None) == -1
            eng.synchronize()
            eng.check_async()      # reported once, then clear
        else:
            eng.synchronize()
        out = d_out.get()
    finally:
        for x in (d_pairs, d_out, d_n):
            if x is not None:
                x.free()
    raw = out.view(np.uint8).reshape(-1, 32)
    assert (raw[:GUARD] == BAND).all() and (raw[GUARD + cap:] == BAND).all(), "written outside the output"
    bound = cap if n_dev is None else min(cap, n_dev)
    assert (raw[GUARD + bound: GUARD + cap] == BAND).all(), "written at or beyond min(n_pairs, *d_n_pairs)"
    return out[GUARD: GUARD + cap]


def poly_call(eng, a, b, row_base=0, col_base=0):
    return lambda d_pairs, cap, out, d_n: eng.poly_pair_distances(a, b, d_pairs, cap, out, n_pairs_dev=d_n, row_base=row_base, col_base=col_base)


def rect_call(eng, a, b, row_base=0, col_base=0):
    return lambda d_pairs, cap, out, d_n: eng.rect_pair_distances(a.ptrs, a.n, b.ptrs, b.n, d_pairs, cap, out, n_pairs_dev=d_n, row_base=row_base,
                                                                  col_base=col_base)


def assert_same(got, want, what):
    ok = ref.same(got, want)
    if not ok.all():
        q = int(np.flatnonzero(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {len(want)} records differ; first at {q}: got {got[q]}, want {want[q]}")


def rect_pairwise_gpu(eng, a, b, pairs):
    """the boolean of c2d_sat_rect_pairs_verts on the listed pairs"""
    i, j = local(pairs)
    d = eng.to_device(np.concatenate([a[:, i], b[:, j]]))
    d_out = eng.zeros(len(pairs), np.uint8)
    eng.sat_rect_pairs_verts([d.row(k) for k in range(16)], len(pairs), d_out)
    out = d_out.get()
    d.free()
    d_out.free()
    return out


@pytest.fixture(scope="module")
def dense(wl):
    """the dense sets (300 x 311 polygons) with the reference records of ALL their pairs, computed once"""
    a, b = cases.dense_poly_sets(wl)
    pairs = cases.all_pairs(a[0].shape[1], b[0].shape[1])
    want = ref.poly_distances(a, b, *local(pairs))
    want.setflags(write=False)
    assert 0.1 < want["hit"].mean() < 0.5
    return a, b, pairs, want


def test_values_for_every_list_length(eng, dense):
    """Lists of 0, 1, 63, 64, 65, 255, 256, 257, 1000 and 4099 entries cut from the all-pairs enumeration: hit pairs only (every wave
    skips the candidate loops), separated pairs only, and every 17th pair (mixed waves)."""
    a, b, pairs, want = dense
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    hits, seps = np.flatnonzero(want["hit"] == 1), np.flatnonzero(want["hit"] == 0)
    mixed = np.arange(0, len(pairs), 17)
    assert len(hits) >= 4099 and len(seps) >= 4099 and len(mixed) >= 4099 and 0.1 < want["hit"][mixed].mean() < 0.5
    for length in cases.LIST_LENGTHS:
        for name, sel in (("hit", hits[-length:] if length else hits[:0]), ("separated", seps[:length]), ("mixed", mixed[:length])):
            got = run(eng, poly_call(eng, ua.set, ub.set), pairs[sel])
            assert_same(got, want[sel], f"{name} list of {length}")
    eng.check_async()
    ua.free()
    ub.free()


def test_dense_batch_in_order_and_shuffled(eng, dense):
    """All 93 300 pairs row-major (long runs of one row per wave), and the same list in a fixed shuffle: a wave then mixes rows, sides,
    regions and hit pairs."""
    a, b, pairs, want = dense
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    got = run(eng, poly_call(eng, ua.set, ub.set), pairs)
    assert_same(got, want, "all pairs")
    assert np.array_equal(got["hit"], pairwise_gpu(eng, a, b, pairs)), "hit differs from c2d_sat_poly_pairs_rows"
    order = np.random.default_rng(8301).permutation(len(pairs))
    assert_same(run(eng, poly_call(eng, ua.set, ub.set), pairs[order]), want[order], "all pairs, shuffled")
    eng.check_async()
    ua.free()
    ub.free()


def test_device_count_bounds_the_work(eng, dense):
    """n_pairs = capacity with the count on the device: smaller, equal, larger (clamped to n_pairs), and no count at all.  run() checks
    the guard bands and every record beyond the bound."""
    a, b, pairs, want = dense
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    sel = np.arange(5, len(pairs), 311)[:300]
    for n_dev in (0, 1, 63, 64, 137, 299, 300, 301, 1 << 40, (1 << 64) - 1, None):
        got = run(eng, poly_call(eng, ua.set, ub.set), pairs[sel], capacity=300, n_dev=n_dev)
        bound = 300 if n_dev is None else min(300, n_dev)
        assert_same(got[:bound], want[sel][:bound], f"device count {n_dev}")
    got = run(eng, poly_call(eng, ua.set, ub.set), pairs[sel], capacity=1000, n_dev=300)
    assert_same(got[:300], want[sel], "capacity 1000, count 300")
    eng.check_async()
    ua.free()
    ub.free()


def test_layout_variants(eng, wl):
    """rows 4, 8 and 16 on either side (different rows for A and B), k == rows with d_k == NULL, stride > n with the planes shifted by
    one float, A and B the same memory, and shards with row_base / col_base."""
    for ra, rb in ((4, 4), (4, 16), (8, 4), (16, 8), (8, 8)):
        a, b = cases.dense_poly_sets(wl, n=90, extent=3.0, rows_a=ra, rows_b=rb, seeds=(7500 + ra, 7600 + rb))
        pairs = cases.all_pairs(90, 101)[::3]
        want = ref.poly_distances(a, b, *local(pairs))
        ua, ub = Uploaded(eng, a, offset=1, stride=90 + 7), Uploaded(eng, b, offset=1, stride=101 + 3)
        assert_same(run(eng, poly_call(eng, ua.set, ub.set), pairs), want, f"rows {ra} x {rb}")
        ua.free()
        ub.free()
    # every polygon has exactly `rows` vertices (the closing edge is slot 16 = slot 0 at rows = 16): no count plane on A, on B, on both
    a = wl.random_convex_polygon_set(80, seed=7701, kmin=16, kmax=16, extent=3.0, rows=16)
    b = wl.random_convex_polygon_set(90, seed=7702, kmin=4, kmax=4, extent=3.0, rows=4)
    c = wl.random_convex_polygon_set(90, seed=7703, extent=3.0)
    d = wl.random_convex_polygon_set(80, seed=7705, kmin=8, kmax=8, extent=3.0, rows=8)
    for x, y in ((a, c), (c, b), (a, b), (d, a)):
        pairs = cases.all_pairs(x[0].shape[1], y[0].shape[1])[::2]
        want = ref.poly_distances(x, y, *local(pairs))
        assert 0.02 < want["hit"].mean() < 0.9
        ux, uy = Uploaded(eng, x, with_k=x is c), Uploaded(eng, y, with_k=y is c)
        assert (ux.dk is None) or (uy.dk is None)
        assert_same(run(eng, poly_call(eng, ux.set, uy.set), pairs), want, "d_k == NULL")
        ux.free()
        uy.free()
    # one set against itself, and shards of it with their bases
    n = 150
    s = wl.random_convex_polygon_set(n, seed=7704, extent=3.0)
    us = Uploaded(eng, s, offset=1, stride=n + 5)
    pairs = cases.all_pairs(n, n)[::5]
    want = ref.poly_distances(s, s, *local(pairs))
    assert_same(run(eng, poly_call(eng, us.set, us.set), pairs), want, "the same memory")
    diag = want[pairs[:, 0] == pairs[:, 1]]
    assert len(diag) > 10 and (diag["hit"] == 1).all() and (diag["dist"] == 0).all()
    r0, r1, c0, c1, rb, cb = 37, 111, 20, 150, 1000, 4_000_000_000
    block = cases.all_pairs(r1 - r0, c1 - c0)[::3]
    sub = (tuple(x[..., r0:r1] for x in s), tuple(x[..., c0:c1] for x in s))
    want = ref.poly_distances(*sub, *local(block))
    listed = (block.astype(np.int64) + (rb, cb)).astype(np.uint32)
    assert_same(run(eng, poly_call(eng, us.sub(r0, r1), us.sub(c0, c1), row_base=rb, col_base=cb), listed), want, "shards with bases")
    eng.check_async()
    us.free()


HARD = None


def hard_batches(wl):
    global HARD
    if HARD is None:
        HARD = cases.hard_poly_batches(wl)
    return HARD


HARD_NAMES = ["clockwise", "clockwise_both", "repeated_vertices", "k1_k2", "touching", "equal_shapes", "equal_boxes", "scale_1e30", "scale_1e-30",
              "scale_1e-42", "scale_1e18", "scale_1e-18", "non_finite_vertex0", "non_finite_later_vertex", "overflowing_len2"]


@pytest.mark.parametrize("name", HARD_NAMES)
def test_hard_inputs(eng, wl, name):
    """one small batch per class of tests/contact_cases.py: where masking the padding, the closing edge, k = 1 / 2, exact ties and
    non-finite input go wrong"""
    a, b, pairs, finite = hard_batches(wl)[name]
    assert sorted(hard_batches(wl)) == sorted(HARD_NAMES), "a batch of hard_poly_batches is not run"
    want = ref.poly_distances(a, b, *local(pairs))
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    got = run(eng, poly_call(eng, ua.set, ub.set), pairs)
    ua.free()
    ub.free()
    assert_same(got, want, name)
    assert np.array_equal(got["hit"], pairwise_gpu(eng, a, b, pairs))
    sep = got["hit"] == 0
    if finite:
        assert (got["flags"][sep] & (ref.NO_CANDIDATE | ref.BAD_PAIR) == 0).all() and np.isfinite(got["dist"]).all()
        assert sep.any() or name == "equal_boxes"
    if name in ("touching", "equal_boxes"):
        assert (got["hit"][:100] == 1).all() and (got["dist"][:100] == 0).all()
    if name == "k1_k2":
        ka, kb = a[2][pairs[:, 0]], b[2][pairs[:, 1]]
        assert (sep & (ka == 1)).any() and (sep & (kb == 1)).any() and (sep & (ka == 2) & (kb == 2)).any()
    if name == "scale_1e30":
        assert (got["dist"][sep] == np.inf).any()        # d2 overflows; +inf is usable
    eng.check_async()


def grid_boxes(n=2048, seed=8302):
    """boxes on a 1/64 grid that share a rotation of 0 (every second: 90 degrees, i.e. another first vertex), B face to face with A
    at an exact gap, with equal or unequal heights and offsets: vertex-to-vertex and vertex-to-edge minima reached by many
    candidates with the same bits -> (a, b) as 4-gon sets, (a, b) as planes f32[8][n]"""
    rng = np.random.default_rng(seed)
    g = lambda lo, hi: rng.integers(int(lo * 64), int(hi * 64) + 1, n) / 64.0  # noqa: E731
    x0, y0, wa, ha, wb, hb = g(-4, 4), g(-4, 4), g(0.25, 2), g(0.25, 2), g(0.25, 2), g(0.25, 2)
    gap, off = g(1 / 64, 1), np.where(rng.random(n) < 0.5, 0.0, g(-1, 1))
    hb = np.where(rng.random(n) < 0.4, ha, hb)
    side = rng.integers(0, 4, n)       # B to the right, above, to the left, below
    bx = np.where(side == 0, x0 + wa + gap, np.where(side == 2, x0 - gap - wb, x0 + off))
    by = np.where(side == 1, y0 + ha + gap, np.where(side == 3, y0 - gap - hb, y0 + off))
    corner = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float64)
    out = []
    for px, py, w, h in ((x0, y0, wa, ha), (bx, by, wb, hb)):
        first = rng.integers(0, 4, n)
        c = corner[(first[:, None] + np.arange(4)[None, :]) % 4]
        out.append(np.stack([px[:, None] + w[:, None] * c[..., 0], py[:, None] + h[:, None] * c[..., 1]], axis=-1))
    four = np.full(n, 4)
    return (cases._as_poly_set(out[0], four, rows=4), cases._as_poly_set(out[1], four, rows=4)), (cases._as_planes(out[0]), cases._as_planes(out[1]))


def test_boxes_on_a_grid_many_way_ties(eng):
    """grid_boxes as 4-gons through the polygon call and as planes through the rectangle call: the minimum is reached by several
    candidates with the same bits, the winner among them is the rule's first, and the two calls give the same records"""
    (pa, pb), (ra, rb) = grid_boxes()
    n = pa[0].shape[1]
    pairs = np.stack([np.arange(n), np.arange(n)], axis=1).astype(np.uint32)
    want = ref.poly_distances(pa, pb, *local(pairs))
    assert (want["hit"] == 0).all() and (want["flags"] & ref.INTERIOR != 0).mean() > 0.2 and (want["flags"] & ref.INTERIOR == 0).mean() > 0.2
    assert ref.same(ref.rect_distances(ra, rb, *local(pairs)), want).all()
    ua, ub = Uploaded(eng, pa), Uploaded(eng, pb)
    assert_same(run(eng, poly_call(eng, ua.set, ub.set), pairs), want, "boxes as 4-gons")
    ua.free()
    ub.free()
    da, db = RectsOnDevice(eng, ra), RectsOnDevice(eng, rb)
    assert_same(run(eng, rect_call(eng, da, db), pairs), want, "boxes as planes")
    da.free()
    db.free()
    eng.check_async()


def test_rectangles(eng, oracle, wl):
    """About 500 rectangles per set: the list of rect_cross_pairs_host (all hit), every list length, a list with separated pairs,
    shards with bases, quads that are no rectangles, and a batch with non-finite vertices."""
    ra, rb = cases.rect_sets(oracle, wl)
    da, db = RectsOnDevice(eng, ra), RectsOnDevice(eng, rb)
    cross = eng.rect_cross_pairs_host(ra, rb)
    assert len(cross) > 4099
    got = run(eng, rect_call(eng, da, db), cross)
    assert_same(got, ref.rect_distances(ra, rb, *local(cross)), "the cross list")
    assert (got["hit"] == 1).all() and (got["dist"] == 0).all()
    mixed = cases.all_pairs(500, 500)[::41]
    want = ref.rect_distances(ra, rb, *local(mixed))
    assert len(mixed) >= 4099 and 0.02 < want["hit"].mean() < 0.5
    for length in cases.LIST_LENGTHS:
        assert_same(run(eng, rect_call(eng, da, db), mixed[:length]), want[:length], f"list of {length}")
    got = run(eng, rect_call(eng, da, db), mixed)
    assert_same(got, want, "mixed list")
    assert np.array_equal(got["hit"], rect_pairwise_gpu(eng, ra, rb, mixed))
    rb0, cb0 = 70_000, 12
    shard = cases.all_pairs(100, 80)[::3]
    d_sa, d_sb = RectsOnDevice(eng, ra[:, 200:300]), RectsOnDevice(eng, rb[:, 40:120])
    listed = (shard.astype(np.int64) + (rb0, cb0)).astype(np.uint32)
    assert_same(run(eng, rect_call(eng, d_sa, d_sb, row_base=rb0, col_base=cb0), listed), ref.rect_distances(ra[:, 200:300], rb[:, 40:120], *local(shard)),
                "shards with bases")
    qa, qb = cases.quad_sets()
    nf = wl.inject_non_finite(ra[:, :200], seed=7801, frac=0.3)
    grid = cases.all_pairs(200, 200)[::3]
    i, j = local(grid)
    for name, (sa, sb) in {"quads": (qa, qb), "non-finite": (nf, qb)}.items():
        d_x, d_y = RectsOnDevice(eng, sa), RectsOnDevice(eng, sb)
        got = run(eng, rect_call(eng, d_x, d_y), grid)
        assert_same(got, ref.rect_distances(sa, sb, i, j), name)
        assert np.array_equal(got["hit"], rect_pairwise_gpu(eng, sa, sb, grid)), name
        d_x.free()
        d_y.free()
    for x in (da, db, d_sa, d_sb):
        x.free()
    eng.check_async()


def test_bad_pairs_read_nothing_and_are_reported_once(eng, wl):
    """Indices equal to n, 0xFFFFFFFF and below the base, in either column, and polygons with a vertex count of 0 and 17: those
    entries carry BAD_PAIR, every other entry is correct, and the error is reported once by the next synchronise.  The planes end
    where their allocations end."""
    n_a, n_b, rb, cb = 50, 64, 1000, 5
    a = wl.random_convex_polygon_set(n_a, seed=8001, extent=2.5)
    b = wl.random_convex_polygon_set(n_b, seed=8002, kmax=8, extent=2.5, rows=8)
    kb = b[2].copy()
    kb[[3, 40]] = [0, 17]
    b = (b[0], b[1], kb)
    d = [eng.to_device(x) for x in (*a, *b)]        # exact allocations: nothing behind the last plane row
    sa, sb = eng.poly_set(d[0], d[1], d[2], n_a, 16), eng.poly_set(d[3], d[4], d[5], n_b, 8)
    good = cases.all_pairs(n_a, n_b)[::7].astype(np.int64) + (rb, cb)
    bad = np.array([[rb + n_a, cb], [0xFFFFFFFF, cb + 1], [rb - 1, cb + 2], [rb + 1, cb + n_b], [rb + 2, 0xFFFFFFFF], [rb + 3, cb - 1],
                    [0, 0], [0xFFFFFFFF, 0xFFFFFFFF], [rb + n_a + 70, cb + 3]], np.int64)
    listed = good.copy()
    at = np.array([0, 1, 63, 64, 65, 200, 255, 256, len(good) - 1])
    listed[at] = bad
    want = ref.poly_distances(a, b, listed[:, 0] - rb, listed[:, 1] - cb)
    assert (want["flags"][at] == ref.BAD_PAIR).all() and (want["flags"] == ref.BAD_PAIR).sum() > len(at)   # (the bad counts as well)
    assert (want["flags"] != ref.BAD_PAIR).sum() > 300
    eng.check_async()
    got = run(eng, poly_call(eng, sa, sb, row_base=rb, col_base=cb), listed.astype(np.uint32), expect_error=True)
    assert_same(got, want, "list with bad pairs")
    ra = np.ascontiguousarray(np.concatenate([a[0][:4], a[1][:4]])[[0, 4, 1, 5, 2, 6, 3, 7]])
    da = RectsOnDevice(eng, ra)
    want = ref.rect_distances(ra, ra, listed[:, 0] - rb, listed[:, 1] - cb)
    got = run(eng, rect_call(eng, da, da, row_base=rb, col_base=cb), listed.astype(np.uint32), expect_error=True)
    assert_same(got, want, "rectangle list with bad pairs")
    # a clean call afterwards reports nothing
    sound = good[(kb[good[:, 1] - cb] >= 1) & (kb[good[:, 1] - cb] <= 8)][:10]
    clean = run(eng, poly_call(eng, sa, sb, row_base=rb, col_base=cb), sound.astype(np.uint32))
    assert (clean["flags"] & ref.BAD_PAIR == 0).all()
    eng.check_async()
    for x in d + [da]:
        x.free()


def test_pipeline_from_the_list_calls(eng, wl):
    """Broad list -> distances on one stream with the list's device count and no read-back in between: every listed pair is hit.  And
    the full cross enumeration of two small sets (a caller's own list: all pairs) -> distances."""
    n = 4099
    a = wl.random_convex_polygon_set(n, seed=7901, extent=70.0)
    ua = Uploaded(eng, a)
    cross = eng.poly_cross_pairs_host(*a, *a, upper=True)
    cap = len(cross) + 100
    assert len(cross) > 1000
    d_pairs, d_cnt = eng.empty((cap, 2), np.uint32), eng.zeros(1, np.uint64)
    d_out = eng.empty(cap, ref.DISTANCE_DT)
    eng.memset(d_out, BAND, d_out.nbytes)
    eng.sat_poly_broad_pairs(ua.set, ua.set, d_pairs, cap, d_cnt, upper=True)
    eng.poly_pair_distances(ua.set, ua.set, d_pairs, cap, d_out, n_pairs_dev=d_cnt)
    eng.synchronize()
    out, listed = d_out.get(), d_pairs.get()[:len(cross)]
    assert int(d_cnt.get()[0]) == len(cross) and np.array_equal(listed, cross)
    assert_same(out[:len(cross)], ref.poly_distances(a, a, *local(cross)), "broad list -> distances")
    assert (out["hit"][:len(cross)] == 1).all() and (out[len(cross):].view(np.uint8) == BAND).all()
    for x in (d_pairs, d_cnt, d_out, ua):
        x.free()
    s, t = cases.dense_poly_sets(wl, n=40, extent=6.0, seeds=(7905, 7906))
    pairs = cases.all_pairs(40, 51)
    us, ut = Uploaded(eng, s), Uploaded(eng, t)
    got = run(eng, poly_call(eng, us.set, ut.set), pairs)
    assert_same(got, ref.poly_distances(s, t, *local(pairs)), "all pairs of two small sets")
    clearance = got["dist"].reshape(40, 51).min(axis=1)        # what a planner asks: each A's distance from the nearest B
    assert (clearance >= 0).all() and (clearance > 0).any()
    us.free()
    ut.free()
    eng.check_async()


def test_list_longer_than_one_grid(eng, oracle, wl):
    """2^24 + 197 entries (a 4099-entry mixed list of the rectangle batch, tiled): the launch is capped at 65 536 blocks of 256, so
    the last 197 entries are the second trip of the grid-stride loop.  Once without a device count, once with 2^24 + 70: the
    127 records beyond it keep the band bytes (run() checks them).  The whole output is compared."""
    ra, rb = cases.rect_sets(oracle, wl)
    mixed = cases.all_pairs(500, 500)[::41][:4099]
    want = ref.rect_distances(ra, rb, *local(mixed))
    assert len(mixed) == 4099 and 0.02 < want["hit"].mean() < 0.5
    total = (1 << 24) + 197
    tile = np.arange(total) % 4099
    listed = mixed[tile]
    want32 = np.ascontiguousarray(want).view(np.uint32).reshape(-1, 8)
    da, db = RectsOnDevice(eng, ra), RectsOnDevice(eng, rb)
    for n_dev in (None, (1 << 24) + 70):
        bound = total if n_dev is None else n_dev
        got = run(eng, rect_call(eng, da, db), listed, n_dev=n_dev)[:bound]
        got32 = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 8)
        whole = bound // 4099 * 4099
        differs = np.concatenate([(got32[:whole].reshape(-1, 4099, 8) != want32[None]).any(axis=2).ravel(),
                                  (got32[whole:] != want32[:bound - whole]).any(axis=1)])
        at = np.flatnonzero(differs)        # not the same bytes: +0 against -0 is still the same record
        if len(at):
            ok = ref.same(got[at], want[tile[at]])
            assert ok.all(), (f"device count {n_dev}: {int((~ok).sum())} of {bound} records differ; first at entry {int(at[~ok][0])}: "
                              f"got {got[at[~ok][0]]}, want {want[tile[at[~ok][0]]]}")
    da.free()
    db.free()
    eng.check_async()


def test_argument_errors(eng, pkg, wl):
    a = wl.random_convex_polygon_set(100, seed=5, extent=3.0)
    ua = Uploaded(eng, a)
    S = ua.set
    d_pairs = eng.zeros((16, 2), np.uint32)
    d_out = eng.zeros(16, ref.DISTANCE_DT)
    d_n = eng.zeros(1, np.uint64)
    mk = lambda **kw: eng.poly_set(kw.get("vx", ua.px), kw.get("vy", ua.py), ua.dk, kw.get("n", 100), kw.get("rows", 16), kw.get("stride", 0))  # noqa: E731
    planes = [ua.px] * 8
    raw = eng.lib.c2d_poly_pair_distances
    assert raw(eng.h, None, C.byref(S), d_pairs.ptr, 16, None, 0, 0, d_out.ptr, None) == -1
    assert raw(eng.h, C.byref(S), None, d_pairs.ptr, 16, None, 0, 0, d_out.ptr, None) == -1
    bad = [
        lambda: eng.poly_pair_distances(mk(vx=0), S, d_pairs, 16, d_out),                       # a NULL plane
        lambda: eng.poly_pair_distances(S, mk(vy=0), d_pairs, 16, d_out),
        lambda: eng.poly_pair_distances(mk(rows=0), S, d_pairs, 16, d_out),                     # rows 0 or 17
        lambda: eng.poly_pair_distances(S, mk(rows=17), d_pairs, 16, d_out),
        lambda: eng.poly_pair_distances(mk(stride=99), S, d_pairs, 16, d_out),                  # stride < n
        lambda: eng.poly_pair_distances(mk(vx=ua.px + 2), S, d_pairs, 16, d_out),               # a misaligned plane
        lambda: eng.poly_pair_distances(S, S, None, 16, d_out),                                 # no list
        lambda: eng.poly_pair_distances(S, S, d_pairs, 16, None),                               # no output
        lambda: eng.poly_pair_distances(S, S, d_pairs, 15, d_out.ptr + 8),                      # output not 16-byte aligned
        lambda: eng.poly_pair_distances(S, S, d_pairs.ptr + 2, 15, d_out),                      # list not 4-byte aligned
        lambda: eng.poly_pair_distances(S, S, d_pairs, 16, d_out, n_pairs_dev=d_n.ptr + 4),     # count not 8-byte aligned
        lambda: eng.poly_pair_distances(S, S, d_pairs, 1 << 62 | 1, d_out),                     # n_pairs beyond 2^62
        lambda: eng.poly_pair_distances(S, S, d_pairs, 16, d_out, row_base=1 << 62),            # bases beyond 2^62
        lambda: eng.poly_pair_distances(S, S, d_pairs, 16, d_out, col_base=1 << 62),
        lambda: eng.rect_pair_distances(planes[:7] + [0], 100, planes, 100, d_pairs, 16, d_out),
        lambda: eng.rect_pair_distances(planes, 100, planes[:7] + [0], 100, d_pairs, 16, d_out),
        lambda: eng.rect_pair_distances(planes, 100, planes, 100, None, 16, d_out),
        lambda: eng.rect_pair_distances(planes, 100, planes, 100, d_pairs, 16, None),
        lambda: eng.rect_pair_distances(planes, 100, planes, 100, d_pairs, 15, d_out.ptr + 4),
        lambda: eng.rect_pair_distances(planes, 100, planes, 100, d_pairs, 16, d_out, col_base=1 << 62),
    ]
    for q, call in enumerate(bad):
        with pytest.raises(pkg.C2DError) as e:
            call()
        assert e.value.status == -1, q
    eng.poly_pair_distances(S, S, None, 0, None)                      # n_pairs == 0: a no-op
    eng.rect_pair_distances(planes, 100, planes, 100, None, 0, None)
    eng.synchronize()
    assert (d_out.get().view(np.uint8) == 0).all(), "a refused call wrote something"
    for x in (d_pairs, d_out, d_n, ua):
        x.free()


def test_graph_capture_follows_the_device_count():
    """One capture of a distances call with d_n_pairs, replayed with different counts written to the device in between
    (tests/distance_graph_check.py, its own process: torch has to be imported before libc2d.so)."""
    out = subprocess.run([sys.executable, os.path.join(HERE, "distance_graph_check.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "distance graph ok" in out.stdout


def test_fuzzer_configurations_at_a_fixed_seed(eng):
    """tests/tools/distance_fuzz.py at a fixed seed, each configuration from its own stream (seed, index): sixteen configurations,
    polygons and rectangles among them"""
    spec = importlib.util.spec_from_file_location("distance_fuzz", os.path.join(HERE, "tools", "distance_fuzz.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    seen, compared = [], 0
    for i in range(16):
        ok, (desc, bound) = fz.one(eng, np.random.default_rng([FUZZ_SEED, i]), i)
        assert ok, desc
        seen.append(desc)
        compared += bound
    assert any("polygons" in d for d in seen) and any("rectangles" in d for d in seen), seen
    assert compared > 1000
    eng.check_async()
