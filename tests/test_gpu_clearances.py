"""GPU tests of the clearance query (c2d_poly_set_clearances): every field of every record equals tests/clearance_ref.py — the numpy
restatement of the contract of include/c2d.h, the reduction over tests/distance_ref.py, pinned by tests/test_clearance_ref_cpu.py —
the five floats bit for bit (+0 and -0 equal); each record also equals what c2d_poly_pair_distances gives for the pair (i, winner)
on the GPU, and `hit` the OR of the row of c2d_sat_poly_cross_mask.  Every output buffer handed to the library sits between guard
bands that are checked afterwards.  No test case asks the numpy reference for more than 1e5 pairs.

The finalise pass recomputes the winner's record, so what the main kernel's own copy of the pairwise test and its own d2min got wrong
shows only in WHO wins.  Four tests make that visible (their inputs are proved on the reference alone in test_clearance_cases_cpu.py):
test_hard_batches_whole                       the hard input classes of contact_cases.py, each batch's A against its whole B
test_every_pairs_boolean_through_a_witness    every pair of those batches alone beside a witness that hits every query, in one tile
                                              and across two strips: `poly` says what the main kernel's walk decided, and it must be
                                              what c2d_sat_poly_pairs_rows decides on the GPU in the same run
test_near_ties_between_obstacles              130 different obstacles within a few ulp of dist of each other, and exactly tied, as
                                              built, reversed and spread over 17 strips
test_between_one_strip_and_one_per_tile       1 < strips < column tiles, an uneven split, many row tiles"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import best_key_harness as best  # noqa: E402
import clearance_cases as cases  # noqa: E402
import clearance_harness as ch  # noqa: E402
import clearance_ref as ref  # noqa: E402
import contact_cases  # noqa: E402
import distance_ref  # noqa: E402
import pair_list_harness as h  # noqa: E402
from pair_list_harness import Uploaded  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
FUZZ_SEED = 20318
FUZZ_UNDERFLOW_CONFIGS = (0, 9)      # the configurations of FUZZ_SEED drawn in the band where d2 underflows to 0 (17 and 76 such winners)
N_B_SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513]


@pytest.fixture(scope="module")
def sparse(wl):
    """64 queries and 513 polygons of the sparse scene's generator, with the per-pair records of all 32 832 pairs, computed once"""
    a, b = cases.scene(wl, n_a=64, n_b=513, extent=80.0)
    D = ref.pair_records(a, b)
    D.setflags(write=False)
    return a, b, D


@pytest.fixture(scope="module")
def many_queries(wl):
    """4099 queries against 24 polygons in a box where a fifth of the queries touch something: 98 376 reference pairs, once"""
    a = wl.random_convex_polygon_set(4099, seed=9311, extent=12.0)
    b = wl.random_convex_polygon_set(24, seed=9312, extent=12.0)
    want = ref.clearances(a, b)
    want.setflags(write=False)
    assert 0.05 < (want["hit"] == 1).mean() < 0.8 and (want["hit"] == 0).mean() > 0.2
    return a, b, want


HARD_NAMES = ["clockwise", "clockwise_both", "repeated_vertices", "k1_k2", "touching", "equal_shapes", "equal_boxes", "scale_1e30", "scale_1e-30",
              "scale_1e-42", "scale_1e18", "scale_1e-18", "non_finite_vertex0", "non_finite_later_vertex", "overflowing_len2"]


@pytest.mark.parametrize("name", HARD_NAMES)
def test_hard_batches_whole(eng, wl, name):
    """one small batch per class of tests/contact_cases.py, the batch's queries against all of its obstacles, twice (the same bytes):
    where masking the padding, the closing edge, k = 1 / 2, exact ties, overflow, underflow and the two NaN rules go wrong in the
    main kernel's own walk of the axes"""
    assert sorted(contact_cases.hard_poly_batches(wl)) == sorted(HARD_NAMES), "a batch of hard_poly_batches is not run"
    a, b, _, _ = cases.witness_batches(wl)[name]
    D, _ = ch.witness_records(wl, name)
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    got = ch.twice(eng, ua.set, ub.set, a[0].shape[1], name)
    ch.assert_same(got, ref.reduce(D, ref.bad_counts(a), ref.bad_counts(b)), name)
    eng.check_async()
    ua.free()
    ub.free()


@pytest.mark.parametrize("name", HARD_NAMES)
def test_every_pairs_boolean_through_a_witness(eng, wl, name):
    """Every obstacle j of a hard batch alone with a witness W that hits every query: [B_j, W] in one staged tile, and [B_j x 64, W]
    with W alone in tile 1 (one row tile: another strip, so the atomic minimum decides).  One call per obstacle on a pointer shard,
    col_base the shard's offset.  The winner is the shard's index 0 exactly when the pair (A_i, B_j) is a hit (or at dist +0), else
    W: every boolean of the main kernel's walk is in `poly`, and must be c2d_sat_poly_pairs_rows' boolean of the pair, computed on
    the GPU here."""
    a, b, w, layouts = cases.witness_batches(wl)[name]
    D, _ = ch.witness_records(wl, name)
    n_a, n_b = a[0].shape[1], b[0].shape[1]
    pairwise = h.pairwise_gpu(eng, a, b, contact_cases.all_pairs(n_a, n_b)).reshape(n_a, n_b) != 0
    first = pairwise | (D["dist"] == 0)
    ua = Uploaded(eng, a)
    band = h.banded(eng, n_a, ch.DT)
    for layout, (s, width) in layouts.items():
        ub = Uploaded(eng, s)
        assert best.strips_of(eng.info()["compute_units"], n_a, width) == -(-width // best.TILE_COLS)
        for j in range(n_b):
            what = f"{name}, {layout}, obstacle {j}"
            got = ch.call(eng, ua.set, ub.sub(width * j, width * (j + 1)), n_a, band=band, col_base=width * j)
            ch.assert_same(got, ch.witness_reference(wl, name, layout, j), what)
            wrong = np.flatnonzero((got["poly"] == width * j) != first[:, j])
            assert len(wrong) == 0, f"{what}: the main kernel and c2d_sat_poly_pairs_rows disagree on the pairs of queries {wrong[:8]}"
            assert np.isin(got["poly"], [width * j, width * j + width - 1]).all(), what
        ub.free()
    eng.check_async()
    band.free()
    ua.free()


def test_near_ties_between_obstacles(eng):
    """tests/clearance_cases.py slid_near_ties: 64 slabs against 130 pentagons that are all 0.75 away in exact arithmetic.  At the
    origin the runner-up is 1..4 ulp of dist behind the winner for a quarter of the queries and more; at (100, -50) most queries
    have their best exactly tied between different obstacles.  The main kernel's d2min must be the contract's to the last bit, its
    comparison strict and its ties the smallest index: as built and reversed (each twice, the same bytes), and at the origin
    tiled to 1 025 obstacles, the near-tied ones in 17 different strips"""
    for theta in cases.NEAR_TIE_THETAS:
        for offset in cases.NEAR_TIE_OFFSETS:
            a, b, D = ch.near_tie_records(theta, offset)
            ia = np.arange(a[0].shape[1])
            orders = {"as built": np.arange(130), "reversed": np.arange(130)[::-1]}
            if offset == cases.NEAR_TIE_OFFSETS[0]:
                orders["tiled to 1025"] = np.resize(np.arange(130), 1025)
            ua = Uploaded(eng, a)
            for order, ib in orders.items():
                what = f"theta {theta}, offset {offset}, {order}"
                ub = Uploaded(eng, ch.take(b, ib))
                got = ch.twice(eng, ua.set, ub.set, 64, what)
                ch.assert_same(got, ch.indexed_reference(a, ia, b, ib, D=D), what)
                assert best.strips_of(eng.info()["compute_units"], 64, len(ib)) == -(-len(ib) // best.TILE_COLS)
                ub.free()
            ua.free()
    eng.check_async()


@pytest.mark.parametrize("s", [2, 4])
def test_between_one_strip_and_one_per_tile(eng, sparse, s):
    """8 * cus / s row tiles (the last one of 5 queries) against 513 polygons, 9 column tiles: 1 < strips < 9 and 9 is no multiple
    of it, so the strips hold unequal numbers of tiles (on 256 CUs: 2 strips of 5 + 4 and 4 of 3 + 2 + 2 + 2), a lane's best is
    carried from tile to tile while the other strips race it through the atomic minimum, and blockIdx.x / strips and % strips
    run over many row tiles.  The queries are drawn from 64 distinct polygons."""
    a, b, D = sparse
    cus = eng.info()["compute_units"]
    row_tiles = 8 * cus // s
    n = best.TILE_ROWS * row_tiles - 251
    strips = best.strips_of(eng.info()["compute_units"], n, 513) if n > 0 else 0
    if not (1 < strips < 9 and 9 % strips != 0):
        pytest.skip(f"{cus} compute units give {strips} strips for 8 * cus / {s} row tiles against 9 column tiles: not strictly between, unevenly split")
    print(f"{cus} compute units, {row_tiles} row tiles, {n} queries: {strips} strips over 9 column tiles")
    ia = np.random.default_rng(9361 + s).integers(0, 64, n)
    ua, ub = Uploaded(eng, ch.take(a, ia)), Uploaded(eng, b)
    got = ch.twice(eng, ua.set, ub.set, n, f"{strips} strips")
    ch.assert_same(got, ref.reduce(D, ref.bad_counts(a), ref.bad_counts(b))[ia], f"{n} queries against 513 in {strips} strips")
    eng.check_async()
    ua.free()
    ub.free()


def test_every_number_of_queries(eng, many_queries):
    """0, 1, 63, 64, 65, 255, 256, 257, 1000 and 4099 queries against 24 polygons (one column tile, one strip)"""
    a, b, want = many_queries
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    for n in contact_cases.LIST_LENGTHS:
        got = ch.call(eng, ua.sub(0, n), ub.set, n)
        ch.assert_same(got, want[:n], f"{n} queries")
        assert best.strips_of(eng.info()["compute_units"], max(n, 1), 24) == 1
    eng.check_async()
    ua.free()
    ub.free()


def test_every_number_of_polygons(eng, sparse):
    """n_b from 1 to 513 on both sides of every power-of-two tile against 64 queries: one row tile against several column tiles takes
    several strips (the atomic minimum joins them), a B of one tile takes one; each run twice, the same bytes"""
    a, b, D = sparse
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    bad_a, bad_b = ref.bad_counts(a), ref.bad_counts(b)
    for n_b in N_B_SIZES:
        want = ref.reduce(D[:, :n_b], bad_a, bad_b[:n_b])
        got = ch.twice(eng, ua.set, ub.sub(0, n_b), 64, f"{n_b} polygons")
        ch.assert_same(got, want, f"{n_b} polygons")
        assert best.strips_of(eng.info()["compute_units"], 64, n_b) == -(-n_b // best.TILE_COLS)
    full = ref.reduce(D, bad_a, bad_b)
    assert (full["hit"] == 0).mean() > 0.3 and (full["hit"] == 1).mean() > 0.05 and len(np.unique(full["poly"])) > 20
    eng.check_async()
    ua.free()
    ub.free()


def test_one_strip_walks_every_tile(eng, sparse):
    """2^19 + 5 queries: the row tiles alone fill the device, so each block walks all column tiles in one strip.  Against 2 polygons
    (and against 130: three tiles in one strip) with the queries drawn from 64 distinct polygons"""
    a, b, D = sparse
    n = (1 << 19) + 5
    rng = np.random.default_rng(9321)
    ia = rng.integers(0, 64, n)
    ua = Uploaded(eng, ch.take(a, ia))
    ub = Uploaded(eng, b)
    bad_a, bad_b = ref.bad_counts(a), ref.bad_counts(b)
    for n_b in (2, 130):
        assert best.strips_of(eng.info()["compute_units"], n, n_b) == 1
        want = ref.reduce(D[:, :n_b], bad_a, bad_b[:n_b])[ia]
        got = ch.call(eng, ua.set, ub.sub(0, n_b), n)
        ch.assert_same(got, want, f"2^19 + 5 queries against {n_b}")
    eng.check_async()
    ua.free()
    ub.free()


@pytest.mark.parametrize("rows_a,rows_b", [(4, 4), (8, 16), (16, 8), (4, 16)])
def test_row_layouts_strides_and_offsets(eng, wl, rows_a, rows_b):
    """rows 4 / 8 / 16 on either side, d_k == NULL (every polygon has `rows` vertices), strides above n and plane offsets"""
    a = wl.random_convex_polygon_set(70, seed=9331, kmin=min(3, rows_a), kmax=rows_a, extent=6.0, rows=rows_a)
    b = wl.random_convex_polygon_set(90, seed=9332, kmin=min(3, rows_b), kmax=rows_b, extent=6.0, rows=rows_b)
    want = ref.clearances(a, b)
    for offset, extra in ((0, 0), (3, 5)):
        ua, ub = Uploaded(eng, a, offset=offset, stride=70 + extra), Uploaded(eng, b, offset=offset + 1, stride=90 + 2 * extra)
        ch.assert_same(ch.call(eng, ua.set, ub.set, 70), want, f"rows {rows_a} / {rows_b}, offset {offset}")
        ua.free()
        ub.free()
    full_a = (a[0], a[1], np.full(70, rows_a, np.uint8))
    full_b = (b[0], b[1], np.full(90, rows_b, np.uint8))     # (the padded slots are zeros: now they are vertices)
    ua, ub = Uploaded(eng, full_a, with_k=False), Uploaded(eng, full_b, with_k=False)
    ch.assert_same(ch.call(eng, ua.set, ub.set, 70), ref.clearances(full_a, full_b), "d_k == NULL")
    eng.check_async()
    ua.free()
    ub.free()


def test_self_clearance_and_shards(eng, sparse):
    """a and b the same memory under SKIP_SELF; shards of both sets with their bases, up to row_base + n_a = col_base + n_b = 2^32"""
    a, b, D = sparse
    s = ch.take(b, np.arange(200))
    Ds = ref.pair_records(s, s)
    bad = ref.bad_counts(s)
    us = Uploaded(eng, s)
    ch.assert_same(ch.twice(eng, us.set, us.set, 200, "self", flags=ref.SKIP_SELF), ref.reduce(Ds, bad, bad, flags=ref.SKIP_SELF), "one set under SKIP_SELF")
    plain = ch.call(eng, us.set, us.set, 200)
    assert (plain["hit"] == 1).all() and (plain["poly"] <= np.arange(200)).all()      # without the flag every polygon touches itself
    top = 1 << 32
    for r0, r1, c0, c1 in ((0, 200, 0, 200), (100, 200, 0, 150), (37, 101, 90, 200)):
        for rb, cb in ((r0, c0), (top - 200 + r0, top - 200 + c0), (5 + r0, 1000 + c0)):
            want = ref.reduce(Ds[r0:r1, c0:c1], bad[r0:r1], bad[c0:c1], row_base=rb, col_base=cb, flags=ref.SKIP_SELF)
            got = ch.call(eng, us.sub(r0, r1), us.sub(c0, c1), r1 - r0, row_base=rb, col_base=cb, flags=ref.SKIP_SELF)
            ch.assert_same(got, want, f"shard rows {r0}..{r1} x columns {c0}..{c1}, bases {rb} / {cb}")
    eng.check_async()
    us.free()


def test_order_independence_by_construction(eng, sparse):
    """One obstacle 1 025 times; the nearest obstacle last of 1 025 (the skip never fires before it); first of 1 025 (the skip fires
    for all the rest); two equidistant obstacles in different tiles and in different strips.  Each twice, the same bytes."""
    a, b, D = sparse
    bad_a, bad_b = ref.bad_counts(a), ref.bad_counts(b)
    full = ref.reduce(D, bad_a, bad_b)
    far = np.argsort(np.where(D["hit"] == 1, 0, D["dist"]).min(axis=0))[::-1][:8]      # obstacles that are nobody's nearest
    near = int(np.bincount(full["poly"], minlength=513).argmax())
    ua = Uploaded(eng, a)
    layouts = {
        "one obstacle 1025 times": np.full(1025, near),
        "the nearest last": np.concatenate([np.resize(far, 1024), [near]]),
        "the nearest first": np.concatenate([[near], np.resize(far, 1024)]),
        "equidistant in tiles 0 and 9": np.concatenate([np.resize(far, 5), [near], np.resize(far, 600), [near], np.resize(far, 418)]),
        "equidistant in one tile": np.concatenate([np.resize(far, 70), [near, near], np.resize(far, 953)]),
    }
    for name, ib in layouts.items():
        ub = Uploaded(eng, ch.take(b, ib))
        want = ref.reduce(D[:, ib], bad_a, bad_b[ib])
        got = ch.twice(eng, ua.set, ub.set, 64, name)
        ch.assert_same(got, want, name)
        assert best.strips_of(eng.info()["compute_units"], 64, len(ib)) == 17
        ub.free()
    eng.check_async()
    ua.free()


def test_hand_cases(eng):
    """the hand cases of tests/clearance_cases.py: the reference, and the values the contract gives"""
    for name, (a, b, kw, expect) in cases.hand_cases().items():
        n_a, n_b = a[0].shape[1], b[0].shape[1]
        ua = Uploaded(eng, a)
        ub = Uploaded(eng, b) if n_b else None
        b_set = ub.set if ub else eng.poly_set(None, None, None, 0, 16)
        bad = bool(ref.bad_counts(a).any() or ref.bad_counts(b).any())
        got = ch.twice(eng, ua.set, b_set, n_a, name, expect_error=bad, **kw)
        ch.assert_same(got, ref.clearances(a, b, **kw), name)
        for f, v in expect.items():
            assert np.array_equal(got[f], np.array(v, got[f].dtype)), (name, f, got[f])
        ua.free()
        if ub:
            ub.free()
    eng.check_async()


def test_adversarial_bound_set_and_scales(eng, wl):
    """the adversarial set of the certified bound (box gap = true distance, coordinates 1, 1e3, 1e6) through the kernel, the nearest
    obstacle last and first; and a scene scaled from 1e30 down to 1e-42, inside and outside the bound's domain and through the band
    where a separated pair's d2 underflows to 0"""
    a, b = cases.adversarial_bound_sets()
    want = ref.clearances(a, b)
    n_b = b[0].shape[1]
    for name, order in (("as built", np.arange(n_b)), ("reversed", np.arange(n_b)[::-1])):
        ua, ub = Uploaded(eng, a), Uploaded(eng, ch.take(b, order))
        got = ch.call(eng, ua.set, ub.set, a[0].shape[1])
        ch.assert_same(got, ch.indexed_reference(a, np.arange(a[0].shape[1]), b, order), f"adversarial set {name}")
        ua.free()
        ub.free()
    assert (want["hit"] == 0).all()
    base_a = wl.random_convex_polygon_set(40, seed=9341, extent=30.0)
    base_b = wl.random_convex_polygon_set(130, seed=9342, extent=30.0)
    # 1e-22 .. 1e-23 is the band where d2 underflows to 0 while the exact test still separates: a lane stops at a separated pair with
    # dist = +0, and a hit and a separated pair tie (6, 6 and 12 such winners here, 1, 5 and 10 of them in front of a later hit)
    for scale in (1e30, 1e18, 1.0, 1e-18, 1e-22, 3e-23, 1e-23, 1e-30, 1e-36, 1e-42):
        sa, sb = (((s[0].astype(np.float64) * scale).astype(F), (s[1].astype(np.float64) * scale).astype(F), s[2]) for s in (base_a, base_b))
        D = ref.pair_records(sa, sb)
        want = ref.reduce(D, ref.bad_counts(sa), ref.bad_counts(sb))
        if 1e-23 <= scale <= 1e-22:
            zero_sep = np.flatnonzero((want["hit"] == 0) & (want["dist"] == 0))
            assert len(zero_sep) >= 6 and any((D["hit"][i, want["poly"][i] + 1:] == 1).any() for i in zero_sep), (scale, len(zero_sep))
        ua, ub = Uploaded(eng, sa), Uploaded(eng, sb)
        ch.assert_same(ch.twice(eng, ua.set, ub.set, 40, f"scale {scale}"), want, f"scale {scale}")
        ua.free()
        ub.free()
    eng.check_async()


def test_non_finite_and_bad_counts(eng, wl):
    """NaN / inf in queries and obstacles; vertex counts out of range in A and in the middle of B, the error reported once"""
    a = tuple(x.copy() for x in wl.random_convex_polygon_set(90, seed=9351, extent=10.0))
    b = tuple(x.copy() for x in wl.random_convex_polygon_set(200, seed=9352, extent=10.0))
    rng = np.random.default_rng(9353)
    for s in (a, b):
        for q in rng.choice(s[0].shape[1], s[0].shape[1] // 4, replace=False):
            s[int(rng.integers(2))][int(rng.integers(0, s[2][q])), q] = rng.choice(np.array([np.nan, np.inf, -np.inf, 3e38, -3e38], F))
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    ch.assert_same(ch.twice(eng, ua.set, ub.set, 90, "non-finite"), ref.clearances(a, b), "non-finite coordinates")
    eng.check_async()
    ua.free()
    ub.free()
    a[2][[3, 64, 89]] = [0, 17, 255]
    b[2][[0, 63, 64, 100, 199]] = [0, 17, 200, 0, 99]
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    want = ref.clearances(a, b)
    assert (want["flags"][[3, 64, 89]] == distance_ref.BAD_PAIR).all() and not np.isin(want["poly"], [0, 63, 64, 100, 199]).any()
    ch.assert_same(ch.call(eng, ua.set, ub.set, 90, expect_error=True), want, "bad counts in both sets")
    # bad counts in B alone, in A alone, and in A with no polygon in B at all: each is reported
    ch.call(eng, ua.sub(4, 60), ub.set, 56, expect_error=True)
    ch.call(eng, ua.set, ub.sub(1, 60), 90, expect_error=True)
    got = ch.call(eng, ua.set, eng.poly_set(None, None, None, 0, 16), 90, expect_error=True)
    ch.assert_same(got, ref.clearances(a, cases.empty()), "bad counts in A, no B")
    ua.free()
    ub.free()


def test_empty_sets_and_untouched_records(eng, sparse):
    """n_b == 0 writes the nothing-considered record; n_a == 0 is a no-op; records at or beyond n_a are never touched"""
    a, b, D = sparse
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    none = eng.poly_set(None, None, None, 0, 16)
    got = ch.call(eng, ua.set, none, 64)
    assert (got["poly"] == 0xFFFFFFFF).all() and np.isinf(got["dist"]).all() and (got["flags"] == ref.NONE_FLAG).all() and (got["edge"] == 0xFFFF).all()
    ch.assert_same(got, ref.clearances(a, cases.empty()), "n_b == 0")
    assert len(ch.call(eng, ua.sub(0, 0), ub.set, 0)) == 0                        # (unband: nothing written anywhere)
    got = ch.call(eng, ua.sub(0, 33), ub.sub(0, 200), 33, capacity=300)           # (unband: records 33 .. 299 untouched)
    ch.assert_same(got, ref.reduce(D[:33, :200], ref.bad_counts(a)[:33], ref.bad_counts(b)[:200]), "33 of 300 records")
    eng.check_async()
    ua.free()
    ub.free()


def test_cross_checks_against_existing_calls(eng, sparse, many_queries):
    """each record against c2d_poly_pair_distances on the pair (i, winner), and `hit` against the OR of the row of
    c2d_sat_poly_cross_mask, both run on the GPU"""
    for a, b in (sparse[:2], many_queries[:2]):
        n_a, n_b = a[0].shape[1], b[0].shape[1]
        ua, ub = Uploaded(eng, a), Uploaded(eng, b)
        got = ch.call(eng, ua.set, ub.set, n_a, col_base=11)
        pairs = np.stack([np.arange(n_a), got["poly"].astype(np.int64) - 11], axis=1).astype(np.uint32)
        d_pairs, d_out = eng.to_device(pairs), eng.empty(n_a, distance_ref.DISTANCE_DT)
        eng.poly_pair_distances(ua.set, ub.set, d_pairs, n_a, d_out)
        words = (n_b + 63) // 64
        d_mask = eng.zeros((n_a, words), np.uint64)
        eng.sat_poly_cross_mask(ua.set, ub.set, d_mask)
        eng.synchronize()
        dist, mask = d_out.get(), d_mask.get()
        for f in ref.COPIED:
            assert got[f].tobytes() == dist[f].tobytes(), f
        assert np.array_equal(got["hit"] == 1, (mask != 0).any(axis=1))
        # a hit record names the first set bit of its row
        first = np.array([next((64 * w + int(x & -x).bit_length() - 1 for w, x in enumerate(map(int, row)) if x), -1) for row in mask])
        assert np.array_equal(got["poly"][got["hit"] == 1].astype(np.int64) - 11, first[got["hit"] == 1])
        for x in (d_pairs, d_out, d_mask):
            x.free()
        ua.free()
        ub.free()
    eng.check_async()


def test_argument_errors(eng, pkg):
    """every refusal with a ctx: status -1, a message that names the call, nothing enqueued"""
    lib, B = eng.lib, pkg.binding
    d = eng.zeros(1024, np.float32)
    out = eng.empty(8, ref.CLEARANCE_DT)
    fn = lib.c2d_poly_set_clearances

    def status(a, b, rb, cb, flags, o):
        return fn(eng.h, None if a is None else C.byref(a), None if b is None else C.byref(b), rb, cb, flags, C.c_void_p(o), None)

    best.refused_set_arguments(status, B._PolySet, d.ptr, out.ptr, "c2d_poly_set_clearances", lambda: lib.c2d_last_error(eng.h))
    eng.synchronize()
    eng.check_async()
    d.free()
    out.free()


def test_graph_capture_in_a_fresh_process():
    """capture and six replays with changed buffers (tests/best_key_graph_check.py clearance: torch is loaded before the library there)"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "best_key_graph_check.py"), "clearance"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "clearance graph ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("idx", range(16))
def test_fixed_seed_fuzz(eng, wl, idx):
    """sixteen fixed-seed configurations of tests/tools/clearance_fuzz.py"""
    fuzz = best.load_tool("clearance_fuzz")
    ok, what = fuzz.one(eng, wl, np.random.default_rng([FUZZ_SEED, idx]), idx)
    assert ok, what
    if idx in FUZZ_UNDERFLOW_CONFIGS:      # scales 2^-73 .. 2^-75: winners that are separated at dist = +0 are really there
        assert fuzz.LAST["zero_separated"] >= 10, what
