"""GPU tests of the shape casts (c2d_poly_set_casts): every field of every record equals tests/cast_ref.py — the numpy restatement of
the contract of include/c2d.h, the reduction over tests/sweep_ref.py, pinned by tests/test_cast_ref_cpu.py — the three floats bit for
bit (+0 and -0 equal); each record also equals what c2d_poly_pair_sweeps gives for the pair (i, winner) on the GPU.  Every output
buffer handed to the library sits between guard bands that are checked afterwards.  No test case asks the numpy reference for more
than 1e5 pairs.

The finalise pass recomputes the winner's record, so a wrong `hit` or a wrong last bit of `toi` in the main kernel shows only in WHO
wins.  Three constructions make that visible (their inputs are proved on the reference alone in test_cast_cases_cpu.py):
test_every_pairs_hit_at_zero_through_a_witness   every pair of the hard batches beside a witness that starts in overlap with every query
test_near_ties_in_motion                         130 obstacles all touched at 1/2 in exact arithmetic, apart by rounding alone
test_grazes                                      t_in == t_out hits beside misses by one grid step"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import best_key_harness as best  # noqa: E402
import cast_cases as cases  # noqa: E402
import cast_harness as ch  # noqa: E402
import cast_ref as ref  # noqa: E402
import clearance_cases  # noqa: E402
import contact_cases  # noqa: E402
import pair_list_harness as h  # noqa: E402
import sweep_ref  # noqa: E402
from pair_list_harness import Motion, Uploaded  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
FUZZ_SEED = 20518
N_B_SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513]
HARD_NAMES = ["clockwise", "clockwise_both", "repeated_vertices", "k1_k2", "touching", "equal_shapes", "equal_boxes", "scale_1e30", "scale_1e-30",
              "scale_1e-42", "scale_1e18", "scale_1e-18", "non_finite_vertex0", "non_finite_later_vertex", "overflowing_len2"]


@pytest.fixture(scope="module")
def sparse(wl):
    """64 queries and 513 polygons of the sparse scene, both sets moving by up to +-6 per component, with the per-pair records of all
    32 832 pairs, computed once"""
    a, b, ma, mb = cases.scene(wl)
    S = ref.pair_records(a, b, ma, mb)
    S.setflags(write=False)
    full = ref.reduce(S, ref.bad_counts(a), ref.bad_counts(b))
    assert (full["hit"] == 0).mean() > 0.1 and ((full["hit"] == 1) & (full["toi"] > 0)).mean() > 0.2 and len(np.unique(full["poly"])) > 20
    return a, b, ma, mb, S


@pytest.fixture(scope="module")
def many_queries(wl):
    """4099 queries against 24 polygons: 98 376 reference pairs, once"""
    a = wl.random_convex_polygon_set(4099, seed=9511, extent=16.0)
    b = wl.random_convex_polygon_set(24, seed=9512, extent=16.0)
    ma, mb = h.motions(9513, 4099, 24, 5.0)
    want = ref.casts(a, b, ma, mb)
    want.setflags(write=False)
    assert (want["hit"] == 0).mean() > 0.1 and ((want["hit"] == 1) & (want["toi"] > 0)).mean() > 0.2 and (want["flags"] == cases.START_OVERLAP).mean() > 0.03
    return a, b, ma, mb, want


def bads(a, b):
    return ref.bad_counts(a), ref.bad_counts(b)


def test_every_number_of_queries(eng, many_queries):
    """0, 1, 63, 64, 65, 255, 256, 257, 1000 and 4099 queries against 24 polygons (one column tile, one strip)"""
    a, b, ma, mb, want = many_queries
    sc = ch.Scene(eng, a, b, ma, mb)
    for n in contact_cases.LIST_LENGTHS:
        got = ch.call(eng, sc.a.sub(0, n), sc.b.set, n, **sc.motions())
        ch.assert_same(got, want[:n], f"{n} queries")
        assert best.strips_of(eng.info()["compute_units"], max(n, 1), 24) == 1
    eng.check_async()
    sc.free()


def test_every_number_of_polygons(eng, sparse):
    """n_b from 1 to 513 on both sides of every power-of-two tile against 64 queries: one row tile against several column tiles takes
    several strips (the atomic minimum joins them), a B of one tile takes one; each run twice, the same bytes"""
    a, b, ma, mb, S = sparse
    sc = ch.Scene(eng, a, b, ma, mb)
    bad_a, bad_b = bads(a, b)
    for n_b in N_B_SIZES:
        want = ref.reduce(S[:, :n_b], bad_a, bad_b[:n_b])
        got = ch.twice(eng, sc.a.set, sc.b.sub(0, n_b), 64, f"{n_b} polygons", **sc.motions())
        ch.assert_same(got, want, f"{n_b} polygons")
        assert best.strips_of(eng.info()["compute_units"], 64, n_b) == -(-n_b // best.TILE_COLS)
    eng.check_async()
    sc.free()


def test_one_strip_walks_every_tile(eng, sparse):
    """2^19 + 5 queries from 64 distinct polygons against 64 obstacles: the row tiles alone fill the device, one strip per block"""
    a, b, ma, mb, S = sparse
    n = (1 << 19) + 5
    ia = np.random.default_rng(9521).integers(0, 64, n)
    ua, da = Uploaded(eng, ch.take(a, ia)), Motion(eng, ch.take_motion(ma, ia))
    ub, db = Uploaded(eng, b), Motion(eng, mb)
    bad_a, bad_b = bads(a, b)
    for n_b in (64, 130):
        assert best.strips_of(eng.info()["compute_units"], n, n_b) == 1
        want = ref.reduce(S[:, :n_b], bad_a, bad_b[:n_b])[ia]
        got = ch.call(eng, ua.set, ub.sub(0, n_b), n, a_motion=da.ptrs, b_motion=db.ptrs)
        ch.assert_same(got, want, f"2^19 + 5 queries against {n_b}")
    eng.check_async()
    for x in (ua, da, ub, db):
        x.free()


@pytest.mark.parametrize("s", [2, 4])
def test_between_one_strip_and_one_per_tile(eng, sparse, s):
    """8 * cus / s row tiles (the last one of 5 queries) against 513 polygons, 9 column tiles: 1 < strips < 9 and 9 is no multiple
    of it, so the strips hold unequal numbers of tiles, a lane's best is carried from tile to tile while the other strips race it
    through the atomic minimum.  The queries are drawn from 64 distinct polygons."""
    a, b, ma, mb, S = sparse
    cus = eng.info()["compute_units"]
    row_tiles = 8 * cus // s
    n = best.TILE_ROWS * row_tiles - 251
    strips = best.strips_of(eng.info()["compute_units"], n, 513) if n > 0 else 0
    if not (1 < strips < 9 and 9 % strips != 0):
        pytest.skip(f"{cus} compute units give {strips} strips for 8 * cus / {s} row tiles against 9 column tiles: not strictly between, unevenly split")
    ia = np.random.default_rng(9561 + s).integers(0, 64, n)
    ua, da = Uploaded(eng, ch.take(a, ia)), Motion(eng, ch.take_motion(ma, ia))
    ub, db = Uploaded(eng, b), Motion(eng, mb)
    got = ch.twice(eng, ua.set, ub.set, n, f"{strips} strips", a_motion=da.ptrs, b_motion=db.ptrs)
    ch.assert_same(got, ref.reduce(S, *bads(a, b))[ia], f"{n} queries against 513 in {strips} strips")
    eng.check_async()
    for x in (ua, da, ub, db):
        x.free()


@pytest.mark.parametrize("rows_a,rows_b", [(4, 4), (8, 16), (16, 8), (4, 16)])
def test_row_layouts_strides_and_offsets(eng, wl, rows_a, rows_b):
    """rows 4 / 8 / 16 on either side, d_k == NULL (every polygon has `rows` vertices), strides above n and plane offsets"""
    a = wl.random_convex_polygon_set(70, seed=9531, kmin=min(3, rows_a), kmax=rows_a, extent=8.0, rows=rows_a)
    b = wl.random_convex_polygon_set(90, seed=9532, kmin=min(3, rows_b), kmax=rows_b, extent=8.0, rows=rows_b)
    ma, mb = h.motions(9533, 70, 90, 3.0)
    want = ref.casts(a, b, ma, mb)
    for place_a, place_b in (((0, 0), (0, 0)), ((3, 5), (4, 10))):
        sc = ch.Scene(eng, a, b, ma, mb, place_a, place_b)
        ch.assert_same(ch.call(eng, sc.a.set, sc.b.set, 70, **sc.motions()), want, f"rows {rows_a} / {rows_b}, places {place_a} {place_b}")
        sc.free()
    full_a = (a[0], a[1], np.full(70, rows_a, np.uint8))
    full_b = (b[0], b[1], np.full(90, rows_b, np.uint8))     # (the padded slots are zeros: now they are vertices)
    sc = ch.Scene(eng, full_a, full_b, ma, mb, with_k=False)
    ch.assert_same(ch.call(eng, sc.a.set, sc.b.set, 70, **sc.motions()), ref.casts(full_a, full_b, ma, mb), "d_k == NULL")
    eng.check_async()
    sc.free()


def test_one_set_against_itself_and_shards(eng, sparse):
    """a and b the same memory under SKIP_SELF with both motions the same planes; shards of both sets with their bases, up to
    row_base + n_a = col_base + n_b = 2^32, the motion planes offset like the vertices"""
    a, b, ma, mb, _ = sparse
    s, ms = ch.take(b, np.arange(200)), ch.take_motion(mb, np.arange(200))
    Ss = ref.pair_records(s, s, ms, ms)
    bad = ref.bad_counts(s)
    sc = ch.Scene(eng, s, s, ms, ms, place_a=(2, 7), same=True)
    got = ch.twice(eng, sc.a.set, sc.a.set, 200, "self", flags=ref.SKIP_SELF, **sc.motions())
    ch.assert_same(got, ref.reduce(Ss, bad, bad, flags=ref.SKIP_SELF), "one set under SKIP_SELF")
    assert (got["poly"] != np.arange(200)).all() and 0.1 < (got["hit"] == 1).mean() < 1.0
    plain = ch.call(eng, sc.a.set, sc.a.set, 200, **sc.motions())
    assert (plain["flags"] == cases.START_OVERLAP).all() and (plain["poly"] <= np.arange(200)).all()      # without the flag every polygon overlaps itself
    top = 1 << 32
    for r0, r1, c0, c1 in ((0, 200, 0, 200), (100, 200, 0, 150), (37, 101, 90, 200)):
        for rb, cb in ((r0, c0), (top - 200 + r0, top - 200 + c0), (5 + r0, 1000 + c0)):
            want = ref.reduce(Ss[r0:r1, c0:c1], bad[r0:r1], bad[c0:c1], row_base=rb, col_base=cb, flags=ref.SKIP_SELF)
            got = ch.call(eng, sc.a.sub(r0, r1), sc.a.sub(c0, c1), r1 - r0, row_base=rb, col_base=cb, flags=ref.SKIP_SELF, **sc.motions(r0, c0))
            ch.assert_same(got, want, f"shard rows {r0}..{r1} x columns {c0}..{c1}, bases {rb} / {cb}")
    eng.check_async()
    sc.free()


def test_who_moves(eng, wl):
    """motion on A only, on B only, on both, none, and all-zero planes; with none or all-zero planes `hit` is the OR of the row of
    c2d_sat_poly_cross_mask on the GPU (bounded inputs)"""
    a = wl.random_convex_polygon_set(150, seed=9541, extent=40.0)
    b = wl.random_convex_polygon_set(140, seed=9542, extent=40.0)
    ma, mb = h.motions(9543, 150, 140, 3.0)
    zero = lambda n: (np.zeros(n, F), np.zeros(n, F))  # noqa: E731
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    d_mask = eng.zeros((150, 3), np.uint64)
    eng.sat_poly_cross_mask(ua.set, ub.set, d_mask)
    eng.synchronize()
    overlap = (d_mask.get() != 0).any(axis=1)
    assert 0.1 < overlap.mean() < 0.9
    for name, xa, xb in (("A only", ma, None), ("B only", None, mb), ("both", ma, mb), ("none", None, None), ("zero planes", zero(150), zero(140)),
                         ("zero on A", zero(150), None)):
        da, db = (None if m is None else Motion(eng, m) for m in (xa, xb))
        got = ch.twice(eng, ua.set, ub.set, 150, name, a_motion=None if da is None else da.ptrs, b_motion=None if db is None else db.ptrs)
        ch.assert_same(got, ref.casts(a, b, xa, xb), name)
        if name in ("none", "zero planes", "zero on A"):
            assert np.array_equal(got["hit"] == 1, overlap) and (got["flags"][overlap] == cases.START_OVERLAP).all(), name
        else:
            assert ((got["hit"] == 1) & ~overlap).sum() > 10, name
        for d in (da, db):
            if d is not None:
                d.free()
    eng.check_async()
    for x in (ua, ub, d_mask):
        x.free()


def test_order_independence_by_construction(eng, sparse):
    """One obstacle 1 025 times; the first-reached obstacle last of 1 025 (the abandon never has a best before it) and first of 1 025
    (the abandon fires for all the rest); two obstacles reached at the same instant in different tiles and strips, and in one tile.
    Each twice, the same bytes."""
    a, b, ma, mb, S = sparse
    bad_a, bad_b = bads(a, b)
    full = ref.reduce(S, bad_a, bad_b)
    never = np.flatnonzero((S["hit"] == 0).all(axis=0))[:8]      # obstacles that nobody reaches
    first = int(np.bincount(full["poly"][full["hit"] == 1], minlength=513).argmax())
    assert len(never) == 8
    ua, da = Uploaded(eng, a), Motion(eng, ma)
    layouts = {
        "one obstacle 1025 times": np.full(1025, first),
        "the first-reached last": np.concatenate([np.resize(never, 1024), [first]]),
        "the first-reached first": np.concatenate([[first], np.resize(never, 1024)]),
        "the whole set reversed": np.arange(513)[::-1],
        "the whole set twice": np.arange(1026) % 513,
        "the same instant in tiles 0 and 9": np.concatenate([np.resize(never, 5), [first], np.resize(never, 600), [first], np.resize(never, 418)]),
        "the same instant in one tile": np.concatenate([np.resize(never, 70), [first, first], np.resize(never, 953)]),
    }
    for name, ib in layouts.items():
        ub, db = Uploaded(eng, ch.take(b, ib)), Motion(eng, ch.take_motion(mb, ib))
        want = ref.reduce(S[:, ib], bad_a, bad_b[ib])
        got = ch.twice(eng, ua.set, ub.set, 64, name, a_motion=da.ptrs, b_motion=db.ptrs)
        ch.assert_same(got, want, name)
        assert best.strips_of(eng.info()["compute_units"], 64, len(ib)) == -(-len(ib) // best.TILE_COLS)
        ub.free()
        db.free()
    eng.check_async()
    ua.free()
    da.free()


def test_hand_cases(eng):
    """the hand cases of tests/cast_cases.py: the reference, and the values the contract gives"""
    for name, (a, b, ma, mb, kw, expect) in cases.hand_cases().items():
        n_a = a[0].shape[1]
        sc = ch.Scene(eng, a, b, ma, mb)
        bad = bool(ref.bad_counts(a).any() or ref.bad_counts(b).any())
        got = ch.twice(eng, sc.a.set, sc.b_set, n_a, name, expect_error=bad, **sc.motions(), **kw)
        ch.assert_same(got, ref.casts(a, b, ma, mb, **kw), name)
        for f, v in expect.items():
            assert np.array_equal(got[f], np.array(v, got[f].dtype)), (name, f, got[f])
        sc.free()
    eng.check_async()


@pytest.mark.parametrize("name", HARD_NAMES)
def test_hard_batches_whole(eng, wl, name):
    """one small batch per class of tests/contact_cases.py with motions of twice the batch's scale, the batch's queries against all of
    its obstacles, twice (the same bytes)"""
    assert sorted(contact_cases.hard_poly_batches(wl)) == sorted(HARD_NAMES), "a batch of hard_poly_batches is not run"
    a, b, _, _ = clearance_cases.witness_batches(wl)[name]
    S, _, (ma, mb) = ch.witness_records(wl, name)
    sc = ch.Scene(eng, a, b, ma, mb)
    got = ch.twice(eng, sc.a.set, sc.b.set, a[0].shape[1], name, **sc.motions())
    ch.assert_same(got, ref.reduce(S, *bads(a, b)), name)
    eng.check_async()
    sc.free()


@pytest.mark.parametrize("name", HARD_NAMES)
def test_every_pairs_hit_at_zero_through_a_witness(eng, wl, name):
    """Every obstacle j of a hard batch alone with a witness W that stands still and starts in overlap with every query: [B_j, W] in
    one staged tile, and [B_j x 64, W] with W alone in tile 1 (one row tile: another strip, so the atomic minimum decides).  One call
    per obstacle on a pointer shard, col_base the shard's offset.  The winner is the shard's index 0 exactly when the pair
    (A_i, B_j) is a hit at toi = +0, else W: that decision of the main kernel's walk is in `poly`, and must be what
    c2d_poly_pair_sweeps says of the pair, computed on the GPU here."""
    a, b, w, layouts = clearance_cases.witness_batches(wl)[name]
    S, _, (ma, mb) = ch.witness_records(wl, name)
    n_a, n_b = a[0].shape[1], b[0].shape[1]
    ua, da, ub0, db0 = Uploaded(eng, a), Motion(eng, ma), Uploaded(eng, b), Motion(eng, mb)
    pairs = contact_cases.all_pairs(n_a, n_b)
    d_pairs, d_sw = eng.to_device(pairs), eng.empty(len(pairs), sweep_ref.SWEEP_DT)
    eng.poly_pair_sweeps(ua.set, ub0.set, d_pairs, len(pairs), d_sw, a_motion=da.ptrs, b_motion=db0.ptrs)
    eng.synchronize()
    sw = d_sw.get().reshape(n_a, n_b)
    first = (sw["hit"] == 1) & (sw["toi"] == 0)
    band = h.banded(eng, n_a, ch.DT)
    for layout, (s, width) in layouts.items():
        is_w = np.tile(np.arange(width) == width - 1, n_b)
        idx = np.repeat(np.arange(n_b), width)
        ms = tuple(np.where(is_w, F(0), m[idx]).astype(F) for m in mb)
        ub, db = Uploaded(eng, s), Motion(eng, ms)
        assert best.strips_of(eng.info()["compute_units"], n_a, width) == -(-width // best.TILE_COLS)
        for j in range(n_b):
            what = f"{name}, {layout}, obstacle {j}"
            got = ch.call(eng, ua.set, ub.sub(width * j, width * (j + 1)), n_a, band=band, col_base=width * j, a_motion=da.ptrs, b_motion=db.sub(width * j))
            ch.assert_same(got, ch.witness_reference(wl, name, layout, j), what)
            wrong = np.flatnonzero((got["poly"] == width * j) != first[:, j])
            assert len(wrong) == 0, f"{what}: the main kernel and c2d_poly_pair_sweeps disagree on the pairs of queries {wrong[:8]}"
            assert np.isin(got["poly"], [width * j, width * j + width - 1]).all(), what
        ub.free()
        db.free()
    eng.check_async()
    for x in (band, ua, da, ub0, db0, d_pairs, d_sw):
        x.free()


def test_near_ties_in_motion(eng):
    """tests/cast_cases.py moving_near_ties: 64 slabs moving by 1.5 towards 130 pentagons that are all 0.75 away: every pair touches
    at 1/2 in exact arithmetic, and most queries have their best exactly tied with, or a few ulp ahead of, another obstacle.  The
    main kernel's t_in must be the contract's to the last bit, its comparison strict and its ties the smallest index: as built and
    reversed (each twice, the same bytes), and at the origin tiled to 1 025 obstacles, the near-tied ones in 17 different strips"""
    for theta in cases.NEAR_TIE_THETAS:
        for offset in cases.NEAR_TIE_OFFSETS:
            a, b, ma, S = ch.near_tie_records(theta, offset)
            ia = np.arange(64)
            orders = {"as built": np.arange(130), "reversed": np.arange(130)[::-1]}
            if offset == cases.NEAR_TIE_OFFSETS[0]:
                orders["tiled to 1025"] = np.resize(np.arange(130), 1025)
            ua, da = Uploaded(eng, a), Motion(eng, ma)
            for order, ib in orders.items():
                what = f"theta {theta}, offset {offset}, {order}"
                ub = Uploaded(eng, ch.take(b, ib))
                got = ch.twice(eng, ua.set, ub.set, 64, what, a_motion=da.ptrs)
                ch.assert_same(got, ch.indexed_reference(a, ia, b, ib, S=S), what)
                assert best.strips_of(eng.info()["compute_units"], 64, len(ib)) == -(-len(ib) // best.TILE_COLS)
                ub.free()
            ua.free()
            da.free()
    eng.check_async()


def test_grazes(eng):
    """tests/cast_cases.py grazes: per query a pass that misses by one grid step in front of the exact graze (t_in == t_out = 1/2, a
    hit) and a hit at the same 1/2 behind it: the winner is the graze; as built, and with each triple reversed (then the hit one
    step lower comes first and wins)"""
    a, b, ma, mb, graze, miss, S = ch.graze_records()
    n = a[0].shape[1]
    for name, ib in (("as built", np.arange(3 * n)), ("triples reversed", (3 * (np.arange(3 * n) // 3) + 2 - np.arange(3 * n) % 3))):
        sc = ch.Scene(eng, a, ch.take(b, ib), ma, ch.take_motion(mb, ib))
        got = ch.twice(eng, sc.a.set, sc.b.set, n, name, **sc.motions())
        ch.assert_same(got, ch.indexed_reference(a, np.arange(n), b, ib, S=S), name)
        assert (got["toi"] == 0.5).all() and np.array_equal(got["poly"], graze if name == "as built" else graze - 1)
        sc.free()
    eng.check_async()


def test_non_finite_and_bad_counts(eng, wl):
    """NaN / inf in queries, obstacles and motions; vertex counts out of range in A and in the middle of B, the error reported once"""
    a = tuple(x.copy() for x in wl.random_convex_polygon_set(90, seed=9551, extent=10.0))
    b = tuple(x.copy() for x in wl.random_convex_polygon_set(200, seed=9552, extent=10.0))
    ma, mb = (tuple(p.copy() for p in m) for m in h.motions(9554, 90, 200, 4.0))
    rng = np.random.default_rng(9553)
    odd = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38], F)
    for s, m in ((a, ma), (b, mb)):
        n = s[0].shape[1]
        for q in rng.choice(n, n // 4, replace=False):
            s[int(rng.integers(2))][int(rng.integers(0, s[2][q])), q] = rng.choice(odd)
        for q in rng.choice(n, n // 8, replace=False):
            m[int(rng.integers(2))][q] = rng.choice(odd)
    with np.errstate(all="ignore"):
        want = ref.casts(a, b, ma, mb)
    sc = ch.Scene(eng, a, b, ma, mb)
    ch.assert_same(ch.twice(eng, sc.a.set, sc.b.set, 90, "non-finite", **sc.motions()), want, "non-finite coordinates and motions")
    eng.check_async()
    sc.free()
    a[2][[3, 64, 89]] = [0, 17, 255]
    b[2][[0, 63, 64, 100, 199]] = [0, 17, 200, 0, 99]
    sc = ch.Scene(eng, a, b, ma, mb)
    with np.errstate(all="ignore"):
        want = ref.casts(a, b, ma, mb)
    assert (want["flags"][[3, 64, 89]] == sweep_ref.BAD_PAIR).all() and not np.isin(want["poly"], [0, 63, 64, 100, 199]).any()
    ch.assert_same(ch.call(eng, sc.a.set, sc.b.set, 90, expect_error=True, **sc.motions()), want, "bad counts in both sets")
    # bad counts in B alone, in A alone, and in A with no polygon in B at all: each is reported
    ch.call(eng, sc.a.sub(4, 60), sc.b.set, 56, expect_error=True, a_motion=sc.ma.sub(4), b_motion=sc.mb.ptrs)
    ch.call(eng, sc.a.set, sc.b.sub(1, 60), 90, expect_error=True, a_motion=sc.ma.ptrs, b_motion=sc.mb.sub(1))
    got = ch.call(eng, sc.a.set, eng.poly_set(None, None, None, 0, 16), 90, expect_error=True, a_motion=sc.ma.ptrs)
    ch.assert_same(got, ref.casts(a, cases.empty(), ma, None), "bad counts in A, no B")
    sc.free()


def test_empty_sets_and_untouched_records(eng, sparse):
    """n_b == 0 writes the miss record; n_a == 0 is a no-op; records at or beyond n_a are never touched"""
    a, b, ma, mb, S = sparse
    sc = ch.Scene(eng, a, b, ma, mb)
    none = eng.poly_set(None, None, None, 0, 16)
    got = ch.call(eng, sc.a.set, none, 64, a_motion=sc.ma.ptrs)
    assert (got["poly"] == 0xFFFFFFFF).all() and np.isinf(got["toi"]).all() and (got["flags"] == 0).all() and (got["axis"] == 0xFFFF).all()
    ch.assert_same(got, ref.casts(a, cases.empty(), ma, None), "n_b == 0")
    assert len(ch.call(eng, sc.a.sub(0, 0), sc.b.set, 0, **sc.motions())) == 0          # (unband: nothing written anywhere)
    got = ch.call(eng, sc.a.sub(0, 33), sc.b.sub(0, 200), 33, capacity=300, **sc.motions())           # (unband: records 33 .. 299 untouched)
    ch.assert_same(got, ref.reduce(S[:33, :200], ref.bad_counts(a)[:33], ref.bad_counts(b)[:200]), "33 of 300 records")
    eng.check_async()
    sc.free()


def test_each_record_against_the_pair_sweeps(eng, sparse, many_queries):
    """each record against c2d_poly_pair_sweeps on the pair (i, winner), run on the GPU; a query without a winner is a miss against
    every obstacle there"""
    for a, b, ma, mb in (sparse[:4], many_queries[:4]):
        n_a, n_b = a[0].shape[1], b[0].shape[1]
        sc = ch.Scene(eng, a, b, ma, mb)
        got = ch.call(eng, sc.a.set, sc.b.set, n_a, col_base=11, **sc.motions())
        won = got["poly"] != ref.NO_POLY
        pairs = np.stack([np.arange(n_a), np.where(won, got["poly"].astype(np.int64) - 11, 0)], axis=1).astype(np.uint32)
        d_pairs, d_out = eng.to_device(pairs), eng.empty(n_a, sweep_ref.SWEEP_DT)
        eng.poly_pair_sweeps(sc.a.set, sc.b.set, d_pairs, n_a, d_out, **sc.motions())
        eng.synchronize()
        sw = d_out.get()
        for f in ref.COPIED:
            assert got[f][won].tobytes() == sw[f][won].tobytes(), f
        assert (got["hit"][won] == 1).all() and (got["hit"][~won] == 0).all() and won.sum() > 10 and (~won).sum() > 5
        for x in (d_pairs, d_out):
            x.free()
        sc.free()
    eng.check_async()


def test_argument_errors(eng, pkg):
    """every refusal with a ctx: status -1, a message that names the call, nothing enqueued"""
    lib, B = eng.lib, pkg.binding
    d = eng.zeros(1024, np.float32)
    out = eng.empty(9, ref.CAST_DT)                # (the last call below writes eight records eight bytes in)
    good = B._PolySet(16, 8, 0, d.ptr, d.ptr, 0)
    fn = lib.c2d_poly_set_casts
    P = C.c_void_p

    def status(a, b, rb=0, cb=0, flags=0, o=out.ptr, m=(None, None, None, None)):
        return fn(eng.h, None if a is None else C.byref(a), None if b is None else C.byref(b), *[None if x is None else P(x) for x in m], rb, cb, flags, P(o), None)

    def refused(a, b, m):
        assert status(a, b, m=m) == -1 and b"c2d_poly_set_casts" in lib.c2d_last_error(eng.h)

    best.refused_set_arguments(status, B._PolySet, d.ptr, out.ptr, "c2d_poly_set_casts", lambda: lib.c2d_last_error(eng.h), off=4)
    for half in ((d.ptr, None, None, None), (None, d.ptr, None, None), (None, None, d.ptr, None), (d.ptr, d.ptr, None, d.ptr)):
        refused(good, good, m=half)                                    # half a motion
    for k in range(4):                                                 # a misaligned motion plane
        refused(good, good, m=tuple(d.ptr + (2 if q == k else 0) for q in range(4)))
    assert status(good, good, (1 << 32) - 8, (1 << 32) - 8, 1, out.ptr + 8, (d.ptr, d.ptr, None, None)) == 0      # exactly 2^32 with a motion, 8-byte aligned
    eng.synchronize()
    eng.check_async()
    d.free()
    out.free()


def test_graph_capture_in_a_fresh_process():
    """capture and six replays with changed buffers (tests/best_key_graph_check.py cast: torch is loaded before the library there)"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "best_key_graph_check.py"), "cast"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "cast graph ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.parametrize("idx", range(16))
def test_fixed_seed_fuzz(eng, wl, idx):
    """sixteen fixed-seed configurations of tests/tools/cast_fuzz.py"""
    fuzz = best.load_tool("cast_fuzz")
    ok, what = fuzz.one(eng, wl, np.random.default_rng([FUZZ_SEED, idx]), idx)
    assert ok, what
