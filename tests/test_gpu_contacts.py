"""GPU tests of the contact queries (c2d_poly_pair_contacts / c2d_rect_pair_contacts): every field of every contact equals
tests/contact_ref.py — the numpy restatement of the contract of include/c2d.h, pinned by tests/test_contact_ref_cpu.py — floats
bit for bit (+0 and -0 equal), and `hit` also equals the pairwise GPU path and the oracle.  Every output buffer handed to the
library sits between guard bands that are checked afterwards."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import contact_cases as cases  # noqa: E402
import contact_ref as ref  # noqa: E402
import pair_list_harness as h  # noqa: E402
from pair_list_harness import RectsOnDevice, Uploaded, local, oracle_hits, pairwise_gpu  # noqa: E402

pytestmark = pytest.mark.gpu
Q = h.CONTACTS
run, poly_call, rect_call, assert_same = Q.run, Q.poly_call, Q.rect_call, Q.assert_same


@pytest.fixture(scope="module")
def dense(wl, oracle):
    """two sets of about 300 polygons in a small box with the reference contacts of ALL their pairs, computed once"""
    a, b, pairs, want = h.dense(wl, Q)
    assert np.array_equal(want["hit"], oracle_hits(oracle, a, b, pairs))
    return a, b, pairs, want


def test_values_for_every_list_length(eng, dense):
    """Lists of 0, 1, 63, 64, 65, 255, 256, 257, 1000 and 4099 entries cut from the all-pairs enumeration: the colliding pairs only
    (what a list call emits) and every 17th pair (separated pairs mixed in)."""
    a, b, pairs, want = dense
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    hits = np.flatnonzero(want["hit"] == 1)
    mixed = np.arange(0, len(pairs), 17)
    assert len(hits) >= 4099 and len(mixed) >= 4099 and 0.1 < want["hit"][mixed].mean() < 0.5
    for length in cases.LIST_LENGTHS:
        for name, sel in (("colliding", hits[-length:] if length else hits[:0]), ("mixed", mixed[:length])):
            got = run(eng, poly_call(eng, ua.set, ub.set), pairs[sel])
            assert_same(got, want[sel], f"{name} list of {length}")
    got = run(eng, poly_call(eng, ua.set, ub.set), pairs)     # all 93 300 pairs: long runs of one row per wave
    assert_same(got, want, "all pairs")
    assert np.array_equal(got["hit"], pairwise_gpu(eng, a, b, pairs)), "hit differs from c2d_sat_poly_pairs_rows"
    eng.check_async()
    ua.free()
    ub.free()


def test_layout_variants(eng, wl):
    """rows 4, 8 and 16 on either side (different rows for A and B), d_k == NULL, stride > n with the planes shifted by one float, A
    and B the same memory, and shards with row_base / col_base."""
    for ra, rb in ((4, 4), (4, 16), (8, 4), (16, 8), (8, 8)):
        a, b = cases.dense_poly_sets(wl, n=90, extent=3.0, rows_a=ra, rows_b=rb, seeds=(7500 + ra, 7600 + rb))
        pairs = cases.all_pairs(90, 101)[::3]
        want = ref.poly_contacts(a, b, *local(pairs))
        ua, ub = Uploaded(eng, a, offset=1, stride=90 + 7), Uploaded(eng, b, offset=1, stride=101 + 3)
        assert_same(run(eng, poly_call(eng, ua.set, ub.set), pairs), want, f"rows {ra} x {rb}")
        ua.free()
        ub.free()
    # every polygon has exactly `rows` vertices: no count plane on A, on B, on both
    a = wl.random_convex_polygon_set(80, seed=7701, kmin=8, kmax=8, extent=3.0, rows=8)
    b = wl.random_convex_polygon_set(90, seed=7702, kmin=4, kmax=4, extent=3.0, rows=4)
    c = wl.random_convex_polygon_set(90, seed=7703, extent=3.0)
    for x, y in ((a, c), (c, b), (a, b)):
        pairs = cases.all_pairs(x[0].shape[1], y[0].shape[1])[::2]
        want = ref.poly_contacts(x, y, *local(pairs))
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
    want = ref.poly_contacts(s, s, *local(pairs))
    assert_same(run(eng, poly_call(eng, us.set, us.set), pairs), want, "the same memory")
    diag = want[pairs[:, 0] == pairs[:, 1]]
    assert len(diag) > 10 and (diag["hit"] == 1).all() and (diag["depth"] > 0).all()
    r0, r1, c0, c1, rb, cb = 37, 111, 20, 150, 1000, 4_000_000_000
    block = cases.all_pairs(r1 - r0, c1 - c0)[::3]
    sub = (tuple(x[..., r0:r1] for x in s), tuple(x[..., c0:c1] for x in s))
    want = ref.poly_contacts(*sub, *local(block))
    listed = (block.astype(np.int64) + (rb, cb)).astype(np.uint32)
    assert_same(run(eng, poly_call(eng, us.sub(r0, r1), us.sub(c0, c1), row_base=rb, col_base=cb), listed), want, "shards with bases")
    eng.check_async()
    us.free()


@pytest.mark.parametrize("name", ["clockwise", "clockwise_both", "repeated_vertices", "k1_k2", "touching", "equal_shapes", "equal_boxes", "scale_1e30",
                                  "scale_1e-30", "scale_1e-42", "scale_1e18", "scale_1e-18", "non_finite_vertex0", "non_finite_later_vertex",
                                  "overflowing_len2"])
def test_hard_inputs(eng, oracle, wl, name):
    """one small batch per class; on the finite, non-overflowing ones hit == (depth >= 0) wherever an axis was usable"""
    a, b, pairs, finite = h.hard_batches(wl)[name]
    want = ref.poly_contacts(a, b, *local(pairs))
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    got = run(eng, poly_call(eng, ua.set, ub.set), pairs)
    ua.free()
    ub.free()
    assert_same(got, want, name)
    assert np.array_equal(got["hit"], oracle_hits(oracle, a, b, pairs))
    assert np.array_equal(got["hit"], pairwise_gpu(eng, a, b, pairs))
    if finite:
        live = got["flags"] == 0
        assert live.any() and np.array_equal(got["hit"][live] == 1, got["depth"][live] >= 0)
    if name == "touching":
        assert (got["depth"][:100] == 0).all() and (got["hit"][:100] == 1).all()
    if name == "k1_k2":
        assert (got["flags"] == ref.NO_AXIS).any() and (got["depth"][got["flags"] == ref.NO_AXIS] == np.inf).all()
    if name == "equal_boxes":
        assert (got["axis"] == 0).all() and (got["depth"] == 1).all()
    eng.check_async()


def test_moving_b_out_along_the_normal_separates(eng, wl):
    """The well-conditioned batch (coordinates in [-8, 8], no degenerate polygon): for every hit pair with depth > 1e-3, B moved by
    (depth + 1e-3 * 8) * normal no longer collides with A in the pairwise test.  The batch keeps at least 90 % of its hit pairs
    under those filters (a condition on the input, checked on the CPU as well: test_contact_ref_cpu.py)."""
    a, b = cases.well_conditioned_poly_sets(wl)
    n = a[0].shape[1]
    pairs = cases.all_pairs(n, n)
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    got = run(eng, poly_call(eng, ua.set, ub.set), pairs)
    ua.free()
    ub.free()
    live = got["flags"] == 0
    assert live.all() and np.array_equal(got["hit"] == 1, got["depth"] >= 0)
    hits = got["hit"] == 1
    keep = hits & (got["depth"] > 1e-3)
    assert hits.sum() > 500 and keep.sum() >= 0.9 * hits.sum(), (hits.sum(), keep.sum())
    norm = np.hypot(got["nx"][keep].astype(np.float64), got["ny"][keep].astype(np.float64))
    assert np.abs(norm - 1).max() < 1e-6
    i, j = local(pairs[keep])
    step = got["depth"][keep] + np.float32(1e-3 * 8)
    moved = cases.translated(b, j, step * got["nx"][keep], step * got["ny"][keep])
    m = len(i)
    after = pairwise_gpu(eng, (a[0][:, i], a[1][:, i], a[2][i]), moved, np.stack([np.arange(m), np.arange(m)], axis=1))
    assert not after.any(), f"{int(after.sum())} of {m} pairs still collide"


def test_rectangles(eng, oracle, wl):
    """About 500 rectangles per set: the lists of rect_cross_pairs_host and rect_broad_pairs_host, a list with separated pairs, quads
    that are no rectangles, and a batch with non-finite vertices."""
    ra, rb = cases.rect_sets(oracle, wl)
    da, db = RectsOnDevice(eng, ra), RectsOnDevice(eng, rb)
    cross = eng.rect_cross_pairs_host(ra, rb)
    broad = eng.rect_broad_pairs_host(ra, rb)
    assert np.array_equal(cross, broad) and len(cross) > 4099
    want = ref.rect_contacts(ra, rb, *local(cross))
    assert (want["hit"] == 1).all() and (want["depth"] >= 0).all()
    got = run(eng, rect_call(eng, da, db), cross)
    assert_same(got, want, "the cross list")
    for length in cases.LIST_LENGTHS:
        assert_same(run(eng, rect_call(eng, da, db), cross[:length]), want[:length], f"list of {length}")
    self_list = eng.rect_broad_pairs_host(ra, upper=True)
    assert len(self_list) > 500
    assert_same(run(eng, rect_call(eng, da, da), self_list), ref.rect_contacts(ra, ra, *local(self_list)), "the broad self list")
    mixed = cases.all_pairs(500, 500)[::41]
    want = ref.rect_contacts(ra, rb, *local(mixed))
    got = run(eng, rect_call(eng, da, db), mixed)
    assert_same(got, want, "mixed list")
    i, j = local(mixed)
    assert np.array_equal(got["hit"], oracle.sat_rect_pairs_verts(np.concatenate([ra[:, i], rb[:, j]]))[0])
    assert 0.02 < got["hit"].mean() < 0.5 and np.array_equal(got["hit"] == 1, got["depth"] >= 0)
    rb0, cb0 = 70_000, 12
    shard = cases.all_pairs(100, 80)[::3]
    d_sa, d_sb = RectsOnDevice(eng, ra[:, 200:300]), RectsOnDevice(eng, rb[:, 40:120])
    listed = (shard.astype(np.int64) + (rb0, cb0)).astype(np.uint32)
    assert_same(run(eng, rect_call(eng, d_sa, d_sb, row_base=rb0, col_base=cb0), listed), ref.rect_contacts(ra[:, 200:300], rb[:, 40:120], *local(shard)),
                "shards with bases")
    qa, qb = cases.quad_sets()
    nf = wl.inject_non_finite(ra[:, :200], seed=7801, frac=0.3)
    grid = cases.all_pairs(200, 200)[::3]
    i, j = local(grid)
    for name, (sa, sb) in {"quads": (qa, qb), "non-finite": (nf, qb)}.items():
        d_x, d_y = RectsOnDevice(eng, sa), RectsOnDevice(eng, sb)
        got = run(eng, rect_call(eng, d_x, d_y), grid)
        assert_same(got, ref.rect_contacts(sa, sb, i, j), name)
        assert np.array_equal(got["hit"], oracle.sat_rect_pairs_verts(np.concatenate([sa[:, i], sb[:, j]]))[0]), name
        d_x.free()
        d_y.free()
    for x in (da, db, d_sa, d_sb):
        x.free()
    eng.check_async()


def test_pipeline_through_the_broad_phase(eng, wl, oracle):
    """poly_contacts_host and rect_contacts_host (broad phase -> list -> contacts on the list's device count) on a sparse scene of
    4099 objects give the pairs and contacts of the cross list followed by the contacts call."""
    n = 4099
    a = wl.random_convex_polygon_set(n, seed=7901, extent=70.0)
    b = wl.random_convex_polygon_set(n, seed=7902, extent=70.0)
    for sets, upper in (((a, b), False), ((a, None), True)):
        sb = sets[0] if sets[1] is None else sets[1]
        pairs, contacts = eng.poly_contacts_host(*sets[0], *((None, None, None) if sets[1] is None else sets[1]), upper=upper)
        cross = eng.poly_cross_pairs_host(*sets[0], *sb, upper=upper)
        assert np.array_equal(pairs, cross) and len(cross) > 1000
        ua, ub = Uploaded(eng, sets[0]), Uploaded(eng, sb)
        direct = run(eng, poly_call(eng, ua.set, ub.set), cross)
        ua.free()
        ub.free()
        assert contacts.dtype == ref.CONTACT_DT and contacts.tobytes() == direct.tobytes()
        assert_same(contacts, ref.poly_contacts(sets[0], sb, *local(cross)), "pipeline")
        assert (contacts["hit"] == 1).all()
        p2, c2 = eng.poly_contacts_host(*sets[0], *((None, None, None) if sets[1] is None else sets[1]), upper=upper, broad=False)
        assert np.array_equal(p2, pairs) and c2.tobytes() == contacts.tobytes()
    poses = wl.random_obb_pose_planes(n, seed=7903, extent=120.0)
    ra, rb = oracle.rects_from_poses(*poses[:5]), oracle.rects_from_poses(*poses[5:])
    for sets, upper in (((ra, rb), False), ((ra, None), True)):
        sb = ra if sets[1] is None else rb
        pairs, contacts = eng.rect_contacts_host(sets[0], sets[1], upper=upper)
        cross = eng.rect_cross_pairs_host(ra, sb, upper=upper)
        assert np.array_equal(pairs, cross) and len(cross) > 1000
        da, db = RectsOnDevice(eng, ra), RectsOnDevice(eng, sb)
        direct = run(eng, rect_call(eng, da, db), cross)
        da.free()
        db.free()
        assert contacts.tobytes() == direct.tobytes()
        assert_same(contacts, ref.rect_contacts(ra, sb, *local(cross)), "rectangle pipeline")
    eng.check_async()
