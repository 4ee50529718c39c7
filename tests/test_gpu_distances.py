"""GPU tests of the distance queries (c2d_poly_pair_distances / c2d_rect_pair_distances): every field of every record equals
tests/distance_ref.py — the numpy restatement of the contract of include/c2d.h, pinned by tests/test_distance_ref_cpu.py — floats
bit for bit (+0 and -0 equal), and `hit` also equals the pairwise GPU path.  Every output buffer handed to the library sits between
guard bands that are checked afterwards."""
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import contact_cases as cases  # noqa: E402
import distance_ref as ref  # noqa: E402
import pair_list_harness as h  # noqa: E402
from pair_list_harness import BAND, RectsOnDevice, Uploaded, local, pairwise_gpu, rect_pairwise_gpu  # noqa: E402

pytestmark = pytest.mark.gpu
FUZZ_SEED = 20263
Q = h.DISTANCES
run, poly_call, rect_call, assert_same = Q.run, Q.poly_call, Q.rect_call, Q.assert_same


@pytest.fixture(scope="module")
def dense(wl):
    """the dense sets (300 x 311 polygons) with the reference records of ALL their pairs, computed once"""
    return h.dense(wl, Q)


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


HARD_NAMES = ["clockwise", "clockwise_both", "repeated_vertices", "k1_k2", "touching", "equal_shapes", "equal_boxes", "scale_1e30", "scale_1e-30",
              "scale_1e-42", "scale_1e18", "scale_1e-18", "non_finite_vertex0", "non_finite_later_vertex", "overflowing_len2"]


@pytest.mark.parametrize("name", HARD_NAMES)
def test_hard_inputs(eng, wl, name):
    """one small batch per class of tests/contact_cases.py: where masking the padding, the closing edge, k = 1 / 2, exact ties and
    non-finite input go wrong"""
    a, b, pairs, finite = h.hard_batches(wl)[name]
    assert sorted(h.hard_batches(wl)) == sorted(HARD_NAMES), "a batch of hard_poly_batches is not run"
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
    pairs = h.diag(n)
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
