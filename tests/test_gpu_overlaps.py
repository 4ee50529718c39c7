"""GPU tests of the overlap queries (c2d_poly_pair_overlaps / c2d_rect_pair_overlaps): every record equals tests/overlap_ref.py — the
numpy restatement of the contract of include/c2d.h, pinned by tests/test_overlap_ref_cpu.py — byte for byte, and `hit` also equals
the pairwise GPU path.  Every output buffer handed to the library sits between guard bands that are checked afterwards (h.run)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import contact_cases as cases  # noqa: E402
import overlap_cases as oc  # noqa: E402
import overlap_ref as ref  # noqa: E402
import pair_list_harness as h  # noqa: E402
from best_key_harness import load_tool  # noqa: E402
from overlap_query import OVERLAPS as Q  # noqa: E402
from pair_list_harness import BAND, RectsOnDevice, Uploaded, local, pairwise_gpu, rect_pairwise_gpu  # noqa: E402

pytestmark = pytest.mark.gpu
FUZZ_SEED = 20275
run, poly_call, rect_call, assert_same = Q.run, Q.poly_call, Q.rect_call, Q.assert_same


@pytest.fixture(scope="module")
def dense(wl):
    """the dense sets (300 x 311 polygons) with the reference records of ALL their pairs, computed once"""
    return h.dense(wl, Q)


def test_dense_batch_in_order_and_shuffled(eng, dense):
    """All 93 300 pairs row-major (long runs of one row per wave; whole waves of misses skip the clip), and the same list in a fixed
    shuffle: a wave then mixes rows, vertex counts, windings, hits and misses."""
    a, b, pairs, want = dense
    assert (want["area"] > 0).mean() > 0.1 and (want["pieces_b"] > 0).mean() > 0.1 and ((want["flags"] & ref.CLAMPED) != 0).any()
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    got = run(eng, poly_call(eng, ua.set, ub.set), pairs)
    assert_same(got, want, "all pairs")
    assert np.array_equal(got["hit"], pairwise_gpu(eng, a, b, pairs)), "hit differs from c2d_sat_poly_pairs_rows"
    order = np.random.default_rng(8401).permutation(len(pairs))
    assert_same(run(eng, poly_call(eng, ua.set, ub.set), pairs[order]), want[order], "all pairs, shuffled")
    eng.check_async()
    ua.free()
    ub.free()


def test_list_lengths_across_a_wave_and_a_block(eng, dense):
    """Lists of 1, 63, 64, 65 and 257 entries: hit pairs only, missed pairs only (every wave skips the clip), and every 17th pair."""
    a, b, pairs, want = dense
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    hits, misses, mixed = np.flatnonzero(want["hit"] == 1), np.flatnonzero(want["hit"] == 0), np.arange(0, len(pairs), 17)
    assert 0.1 < want["hit"][mixed[:257]].mean() < 0.5
    for length in (1, 63, 64, 65, 257):
        for name, sel in (("hit", hits[-length:]), ("missed", misses[:length]), ("mixed", mixed[:length])):
            assert_same(run(eng, poly_call(eng, ua.set, ub.set), pairs[sel]), want[sel], f"{name} list of {length}")
    eng.check_async()
    ua.free()
    ub.free()


HARD_NAMES = ["clockwise", "clockwise_both", "repeated_vertices", "k1_k2", "touching", "equal_shapes", "equal_boxes", "scale_1e30", "scale_1e-30",
              "scale_1e-42", "scale_1e18", "scale_1e-18", "non_finite_vertex0", "non_finite_later_vertex", "overflowing_len2"]


@pytest.mark.parametrize("name", HARD_NAMES)
def test_hard_inputs(eng, wl, name):
    """one small batch per class of tests/contact_cases.py: clockwise sets, repeated vertices, points and segments, shapes that only
    touch, equal shapes (every boundary shared), scales where products overflow or vanish, and non-finite vertices"""
    a, b, pairs, finite = h.hard_batches(wl)[name]
    assert sorted(h.hard_batches(wl)) == sorted(HARD_NAMES), "a batch of hard_poly_batches is not run"
    want = ref.poly_overlaps(a, b, *local(pairs))
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    got = run(eng, poly_call(eng, ua.set, ub.set), pairs)
    ua.free()
    ub.free()
    assert_same(got, want, name)
    assert np.array_equal(got["hit"], pairwise_gpu(eng, a, b, pairs))
    if name in ("clockwise", "clockwise_both", "repeated_vertices", "scale_1e18"):
        assert (got["area"] > 0).any() and (got["hit"] == 0).any()
    if name == "k1_k2":
        assert ((got["flags"] & ref.DEGENERATE) != 0).any() and (got["area"][(got["flags"] & ref.DEGENERATE) != 0] == 0).all()
    if name == "touching":
        assert (got["hit"][:100] == 1).all() and (got["area"][:100] == 0).all() and (got["flags"][:100] == ref.NO_CENTROID).all()
    if name == "equal_boxes":
        assert (got["area"] == got["area_a"]).all() and (got["iou"] == 1).all() and (got["pieces_b"] == 0).all() and (got["pieces_a"] == 4).all()
    eng.check_async()


def test_layout_variants_and_shards(eng, wl):
    """Sets in 8 and in 16 rows (and 4 against 16) with the planes shifted by three floats and a stride of n + 5; one set against
    itself, where the diagonal gives area == area_a to the bit wherever the reference says so; and shards of it with their bases."""
    for ra, rb in ((8, 8), (16, 8), (8, 16), (4, 16)):
        a, b = cases.dense_poly_sets(wl, n=90, extent=3.0, rows_a=ra, rows_b=rb, seeds=(8500 + ra, 8600 + rb))
        pairs = cases.all_pairs(90, 101)[::3]
        want = ref.poly_overlaps(a, b, *local(pairs))
        assert 0.05 < (want["area"] > 0).mean() < 0.9
        ua, ub = Uploaded(eng, a, offset=3, stride=90 + 5), Uploaded(eng, b, offset=3, stride=101 + 5)
        assert_same(run(eng, poly_call(eng, ua.set, ub.set), pairs), want, f"rows {ra} x {rb}")
        ua.free()
        ub.free()
    # every polygon has exactly `rows` vertices (the closing edge is slot 16 = slot 0 at rows = 16): no count plane
    a = wl.random_convex_polygon_set(80, seed=8701, kmin=16, kmax=16, extent=3.0, rows=16)
    b = wl.random_convex_polygon_set(90, seed=8702, kmin=4, kmax=4, extent=3.0, rows=4)
    pairs = cases.all_pairs(80, 90)[::2]
    want = ref.poly_overlaps(a, b, *local(pairs))
    assert 0.02 < want["hit"].mean() < 0.9
    ua, ub = Uploaded(eng, a, with_k=False), Uploaded(eng, b, with_k=False)
    assert_same(run(eng, poly_call(eng, ua.set, ub.set), pairs), want, "d_k == NULL")
    ua.free()
    ub.free()
    n = 150
    s = wl.random_convex_polygon_set(n, seed=8704, extent=3.0)
    us = Uploaded(eng, s, offset=3, stride=n + 5)
    pairs = np.concatenate([cases.all_pairs(n, n)[::5], h.diag(n)])
    want = ref.poly_overlaps(s, s, *local(pairs))
    got = run(eng, poly_call(eng, us.set, us.set), pairs)
    assert_same(got, want, "the same memory")
    diag = pairs[:, 0] == pairs[:, 1]
    whole = diag & (want["area"] == want["area_a"])
    assert diag.sum() >= n and (want["hit"][diag] == 1).all() and whole.sum() > 0.9 * diag.sum()      # (elsewhere the last bits differ, both ways)
    assert (got["area"][whole] == got["area_a"][whole]).all() and (got["iou"][whole] == 1).all() and (got["pieces_b"][whole] == 0).all()
    r0, r1, c0, c1, rb, cb = 37, 111, 20, 150, 1000, 4_000_000_000
    block = cases.all_pairs(r1 - r0, c1 - c0)[::3]
    sub = (tuple(x[..., r0:r1] for x in s), tuple(x[..., c0:c1] for x in s))
    want = ref.poly_overlaps(*sub, *local(block))
    listed = (block.astype(np.int64) + (rb, cb)).astype(np.uint32)
    assert_same(run(eng, poly_call(eng, us.sub(r0, r1), us.sub(c0, c1), row_base=rb, col_base=cb), listed), want, "shards with bases")
    eng.check_async()
    us.free()


def test_exact_cases_on_the_grid(eng):
    """the hand-computed cases of tests/overlap_cases.py as one small list, with NaN and with 1e30 behind each polygon's vertices: the
    table's own values, which are the reference's (tests/test_overlap_ref_cpu.py)"""
    for junk in (np.nan, 1e30):
        a, b, want = oc.exact_sets(junk)
        ua, ub = Uploaded(eng, a), Uploaded(eng, b)
        got = run(eng, poly_call(eng, ua.set, ub.set), h.diag(len(want)))
        assert_same(got, want, f"exact cases, junk {junk}")
        ua.free()
        ub.free()
    eng.check_async()


def test_rectangles(eng, oracle, wl):
    """Rectangles from poses (a broad list, all hit, and a mixed list), random quads, quads with non-finite vertices, shards with
    bases; and boxes on a 1/16 grid through the rectangle call and, as 4-gons, through the polygon call: the same bytes."""
    ra, rb = cases.rect_sets(oracle, wl)
    da, db = RectsOnDevice(eng, ra), RectsOnDevice(eng, rb)
    cross = eng.rect_cross_pairs_host(ra, rb)[:5000]
    got = run(eng, rect_call(eng, da, db), cross)
    assert_same(got, ref.rect_overlaps(ra, rb, *local(cross)), "the cross list")
    assert len(cross) > 4000 and (got["hit"] == 1).all() and (got["area"] > 0).mean() > 0.9
    mixed = cases.all_pairs(500, 500)[::41]
    want = ref.rect_overlaps(ra, rb, *local(mixed))
    assert 0.02 < want["hit"].mean() < 0.5
    for length in (1, 63, 64, 65, 257, len(mixed)):
        assert_same(run(eng, rect_call(eng, da, db), mixed[:length]), want[:length], f"list of {length}")
    assert np.array_equal(want["hit"], rect_pairwise_gpu(eng, ra, rb, mixed))
    rb0, cb0 = 70_000, 12
    shard = cases.all_pairs(100, 80)[::3]
    d_sa, d_sb = RectsOnDevice(eng, ra[:, 200:300]), RectsOnDevice(eng, rb[:, 40:120])
    listed = (shard.astype(np.int64) + (rb0, cb0)).astype(np.uint32)
    assert_same(run(eng, rect_call(eng, d_sa, d_sb, row_base=rb0, col_base=cb0), listed), ref.rect_overlaps(ra[:, 200:300], rb[:, 40:120], *local(shard)),
                "shards with bases")
    qa, qb = cases.quad_sets()
    nf = wl.inject_non_finite(ra[:, :200], seed=8801, frac=0.3)
    grid = cases.all_pairs(200, 200)[::3]
    for name, (sa, sb) in {"quads": (qa, qb), "non-finite": (nf, qb)}.items():
        d_x, d_y = RectsOnDevice(eng, sa), RectsOnDevice(eng, sb)
        assert_same(run(eng, rect_call(eng, d_x, d_y), grid), ref.rect_overlaps(sa, sb, *local(grid)), name)
        d_x.free()
        d_y.free()
    for x in (da, db, d_sa, d_sb):
        x.free()
    (pa, pb), (ga, gb) = oc.overlapping_grid_boxes()
    pairs = h.diag(pa[0].shape[1])
    want = ref.poly_overlaps(pa, pb, *local(pairs))
    assert (want["hit"] == 0).mean() > 0.1 and (want["area"] > 0).mean() > 0.3 and ((want["hit"] == 1) & (want["area"] == 0)).mean() > 0.02
    assert (want["iou"] == 1).any() and ref.same(ref.rect_overlaps(ga, gb, *local(pairs)), want).all()
    ua, ub = Uploaded(eng, pa), Uploaded(eng, pb)
    as_polys = run(eng, poly_call(eng, ua.set, ub.set), pairs)
    ua.free()
    ub.free()
    da, db = RectsOnDevice(eng, ga), RectsOnDevice(eng, gb)
    as_rects = run(eng, rect_call(eng, da, db), pairs)
    da.free()
    db.free()
    assert_same(as_polys, want, "grid boxes as 4-gons")
    assert_same(as_rects, want, "grid boxes as planes")
    assert as_rects.tobytes() == as_polys.tobytes()
    eng.check_async()


def test_pipeline_from_the_broad_list(eng, wl):
    """Broad list -> overlaps on one stream with the list's device count and no read-back in between: every record has hit == 1."""
    n = 4099
    a = wl.random_convex_polygon_set(n, seed=8901, extent=70.0)
    ua = Uploaded(eng, a)
    cross = eng.poly_cross_pairs_host(*a, *a, upper=True)
    cap = len(cross) + 100
    assert len(cross) > 1000
    d_pairs, d_cnt = eng.empty((cap, 2), np.uint32), eng.zeros(1, np.uint64)
    d_out = eng.empty(cap, ref.OVERLAP_DT)
    eng.memset(d_out, BAND, d_out.nbytes)
    eng.sat_poly_broad_pairs(ua.set, ua.set, d_pairs, cap, d_cnt, upper=True)
    eng.poly_pair_overlaps(ua.set, ua.set, d_pairs, cap, d_out, n_pairs_dev=d_cnt)
    eng.synchronize()
    out, listed = d_out.get(), d_pairs.get()[:len(cross)]
    assert int(d_cnt.get()[0]) == len(cross) and np.array_equal(listed, cross)
    assert_same(out[:len(cross)], ref.poly_overlaps(a, a, *local(cross)), "broad list -> overlaps")
    assert (out["hit"][:len(cross)] == 1).all() and (out["area"][:len(cross)] > 0).mean() > 0.9 and (out[len(cross):].view(np.uint8) == BAND).all()
    for x in (d_pairs, d_cnt, d_out, ua):
        x.free()
    eng.check_async()


def test_fuzzer_configurations_at_a_fixed_seed(eng):
    """tests/tools/overlap_fuzz.py at a fixed seed, each configuration from its own stream (seed, index): sixteen configurations,
    polygons and rectangles among them"""
    fz = load_tool("overlap_fuzz")
    seen, compared, areas = [], 0, 0
    for i in range(16):
        ok, (desc, bound) = fz.one(eng, np.random.default_rng([FUZZ_SEED, i]), i)
        assert ok, desc
        seen.append(desc)
        compared += bound
        areas += fz.LAST["areas"]
    assert any("polygons" in d for d in seen) and any("rectangles" in d for d in seen), seen
    assert compared > 1000 and areas > 100
    eng.check_async()
