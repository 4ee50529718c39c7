"""GPU tests of c2d_poly_pair_manifolds: every field of both outputs equals tests/manifold_ref.py / tests/contact_ref.py — the numpy
restatements of the contracts of include/c2d.h, pinned by tests/test_manifold_ref_cpu.py and tests/test_contact_ref_cpu.py — floats
bit for bit (+0 and -0 equal, NaN equal to NaN), and the contact output equals c2d_poly_pair_contacts' on the same list byte for
byte.  Both output buffers sit between guard bands that are checked afterwards."""
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import contact_cases  # noqa: E402
import contact_ref  # noqa: E402
import manifold_cases as cases  # noqa: E402
import manifold_ref as ref  # noqa: E402
import pair_list_harness as h  # noqa: E402
from pair_list_harness import Uploaded, diag, local  # noqa: E402

pytestmark = pytest.mark.gpu
FUZZ_SEED = 2026
LIST_LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 4099]
Q = h.MANIFOLDS
assert_same = Q.assert_same


def manifolds_of(eng, a, b, pairs, **bases):
    """-> (CONTACT_DT[len(pairs)], MANIFOLD_DT[len(pairs)]) of one c2d_poly_pair_manifolds call on the list, between guard bands; the
    contact output is also compared, byte for byte, with what c2d_poly_pair_contacts writes for the same arguments (h.MANIFOLDS)."""
    return Q.run(eng, Q.poly_call(eng, a, b, **bases), pairs)


@pytest.fixture(scope="module")
def dense(wl):
    """two sets of about 300 polygons in a small box and every 17th of their pairs (colliding and separated), with the reference"""
    return h.dense(wl, Q)


@pytest.fixture(scope="module")
def batch(wl):
    """the random batch of tests/test_manifold_ref_cpu.py (every case of the contract at its measured share) with the reference"""
    a, b = cases.random_colliding_batch(wl)
    want = ref.poly_manifolds(a, b, np.arange(cases.BATCH), np.arange(cases.BATCH))
    for w in want:
        w.setflags(write=False)
    return a, b, want


def test_values_for_every_list_length(eng, dense):
    a, b, pairs, want = dense
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    for length in LIST_LENGTHS:
        got = manifolds_of(eng, ua.set, ub.set, pairs[:length])
        assert_same(got, (want[0][:length], want[1][:length]), f"list of {length}")
    assert_same(manifolds_of(eng, ua.set, ub.set, pairs), want, "the whole list")
    eng.check_async()
    ua.free()
    ub.free()


def test_layout_variants(eng, wl):
    """rows 4, 8 and 16 on either side, k == rows at 4 and at 16 with d_k == NULL (the wrap of "next of k - 1" without padding and,
    in the 16-slot registers, with it), stride > n with shifted planes, the same memory for a and b, and shards with bases."""
    for ra, rb in ((4, 4), (4, 16), (8, 4), (16, 8)):
        a, b = contact_cases.dense_poly_sets(wl, n=90, extent=3.0, rows_a=ra, rows_b=rb, seeds=(7500 + ra, 7600 + rb))
        pairs = contact_cases.all_pairs(90, 101)[::3]
        ua, ub = Uploaded(eng, a, offset=1, stride=90 + 7), Uploaded(eng, b, offset=1, stride=101 + 3)
        assert_same(manifolds_of(eng, ua.set, ub.set, pairs), ref.poly_manifolds(a, b, *local(pairs)), f"rows {ra} x {rb}")
        ua.free()
        ub.free()
    full16 = wl.random_convex_polygon_set(80, seed=9201, kmin=16, kmax=16, extent=3.0, rows=16)
    full4 = wl.random_convex_polygon_set(90, seed=9202, kmin=4, kmax=4, extent=3.0, rows=4)
    mixed = wl.random_convex_polygon_set(90, seed=9203, extent=3.0)
    for x, y in ((full16, mixed), (mixed, full4), (full16, full4), (full4, full16), (full16, full16)):
        pairs = contact_cases.all_pairs(x[0].shape[1], y[0].shape[1])[::2]
        want = ref.poly_manifolds(x, y, *local(pairs))
        last = (want[1]["count"] == 2) & (want[1]["feature"] == 15)
        assert x is not full16 or y is not full16 or last.sum() > 20          # the incident edge from vertex 15 back to vertex 0
        ux, uy = Uploaded(eng, x, with_k=x is mixed), Uploaded(eng, y, with_k=y is mixed)
        assert_same(manifolds_of(eng, ux.set, uy.set, pairs), want, "k == rows, d_k == NULL")
        ux.free()
        uy.free()
    n = 150
    s = wl.random_convex_polygon_set(n, seed=9204, extent=3.0)
    us = Uploaded(eng, s, offset=1, stride=n + 5)
    pairs = contact_cases.all_pairs(n, n)[::5]
    assert_same(manifolds_of(eng, us.set, us.set, pairs), ref.poly_manifolds(s, s, *local(pairs)), "the same memory")
    r0, r1, c0, c1, rb, cb = 37, 111, 20, 150, 1000, 4_000_000_000
    block = contact_cases.all_pairs(r1 - r0, c1 - c0)[::3]
    sub = (tuple(x[..., r0:r1] for x in s), tuple(x[..., c0:c1] for x in s))
    listed = (block.astype(np.int64) + (rb, cb)).astype(np.uint32)
    assert_same(manifolds_of(eng, us.sub(r0, r1), us.sub(c0, c1), listed, row_base=rb, col_base=cb), ref.poly_manifolds(*sub, *local(block)), "shards with bases")
    eng.check_async()
    us.free()


@pytest.mark.parametrize("name", ["clockwise", "clockwise_both", "repeated_vertices", "k1_k2", "touching", "equal_shapes", "equal_boxes",
                                  "non_finite_vertex0", "non_finite_later_vertex", "scale_1e30", "scale_1e-42"])
def test_hard_inputs(eng, wl, name):
    """one small batch per class of tests/contact_cases.py"""
    a, b, pairs, _ = h.hard_batches(wl)[name]
    want = ref.poly_manifolds(a, b, *local(pairs))
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    got = manifolds_of(eng, ua.set, ub.set, pairs)
    ua.free()
    ub.free()
    assert_same(got, want, name)
    m = got[1]
    if name == "k1_k2":
        assert (m["count"] == 0).any() and ((m["count"] == 1) & (m["flags"] & ref.OUTSIDE_SLAB == 0)).any()      # NO_AXIS; an incident point
    if name == "touching":
        assert (m["d0"][:100] == 0).all() and (m["count"][:100] == 2).all()
    if name == "equal_boxes":
        assert (m["count"] == 2).all() and (m["d0"] == 1).all() and (m["d1"] == 1).all() and (m["flags"] == 0).all()
    if name.startswith("non_finite"):
        assert np.isnan(m["x0"]).any() or np.isnan(m["d0"]).any() or np.isinf(m["x0"]).any()
    eng.check_async()


def test_random_batch_in_order_and_shuffled(eng, batch):
    """the diagonal list (one row per lane) and the same pairs in a fixed shuffled order: every wave mixes reference sides, signs,
    clip cases and vertex counts"""
    a, b, want = batch
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    assert_same(manifolds_of(eng, ua.set, ub.set, diag(cases.BATCH)), want, "the diagonal")
    order = cases.shuffled()
    assert_same(manifolds_of(eng, ua.set, ub.set, diag(cases.BATCH)[order]), (want[0][order], want[1][order]), "shuffled")
    eng.check_async()
    ua.free()
    ub.free()


def test_scale_sweep_across_the_fast_pick_window(eng, wl):
    """the 2^k sweep of tests/test_gpu_contact_ties.py (contact_cases.WINDOW_EDGE_K), every fifth pair: lanes the first pass decides
    and lanes that take the second pass both reach the manifold code"""
    a, b, pairs, k_of_pair = contact_cases.window_edge_poly_batch(wl)
    pairs, k_of_pair = pairs[::5], k_of_pair[::5]
    terms = contact_ref.poly_axis_terms(a, b, *local(pairs))
    len2_out, o_out = contact_cases.outside_window(terms)
    hard = len2_out | o_out
    assert 0.05 < hard.mean() < 0.95, hard.mean()           # (0.84 on this batch)
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    assert_same(manifolds_of(eng, ua.set, ub.set, pairs), ref.poly_manifolds(a, b, *local(pairs)), "scale sweep")
    eng.check_async()
    ua.free()
    ub.free()


def test_pipeline_through_the_broad_phase(eng, wl):
    """poly_manifolds_host (broad phase -> list -> manifolds on the list's device count) on a sparse scene of 4099 polygons"""
    n = 4099
    a = wl.random_convex_polygon_set(n, seed=7901, extent=70.0)
    b = wl.random_convex_polygon_set(n, seed=7902, extent=70.0)
    for sets, upper in (((a, b), False), ((a, None), True)):
        sb = sets[0] if sets[1] is None else sets[1]
        second = (None, None, None) if sets[1] is None else sets[1]
        pairs, contacts, manifolds = eng.poly_manifolds_host(*sets[0], *second, upper=upper)
        p2, c2 = eng.poly_contacts_host(*sets[0], *second, upper=upper)
        assert np.array_equal(pairs, p2) and len(pairs) > 1000 and contacts.tobytes() == c2.tobytes()
        assert contacts.dtype == contact_ref.CONTACT_DT and manifolds.dtype == ref.MANIFOLD_DT
        assert_same((contacts, manifolds), ref.poly_manifolds(sets[0], sb, *local(pairs)), "pipeline")
        assert (manifolds["count"] >= 1).all() and (contacts["hit"] == 1).all()
        p3, c3, m3 = eng.poly_manifolds_host(*sets[0], *second, upper=upper, broad=False)
        assert np.array_equal(p3, pairs) and c3.tobytes() == contacts.tobytes() and m3.tobytes() == manifolds.tobytes()
    eng.check_async()


@pytest.mark.parametrize("n_dev", [None, (1 << 24) + 70], ids=["whole", "device_count"])
def test_grid_stride_second_trip(eng, batch, n_dev):
    """2^24 + 197 entries — one more than a full grid of 65536 blocks can take in one trip — repeating the 4096-pair batch.  The
    first repetition is compared with the reference, every later one (the 197 of the second trip included) with the first, byte
    for byte; with a device count of 2^24 + 70 the last 127 records of both outputs stay untouched."""
    a, b, want = batch
    n = (1 << 24) + 197
    bound = n if n_dev is None else n_dev
    reps, tail = bound // cases.BATCH, bound % cases.BATCH
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    listed = np.tile(diag(cases.BATCH), (n // cases.BATCH + 1, 1))[:n]
    # (the manifolds call alone: at this length no second contacts call next to it)
    queue = lambda d_pairs, cap, outs, d_n: eng.poly_pair_manifolds(ua.set, ub.set, d_pairs, cap, *outs, n_pairs_dev=d_n)  # noqa: E731
    try:
        outs = h.run(eng, queue, listed, Q.dts, n_dev=n_dev)
        eng.check_async()
    finally:
        ua.free()
        ub.free()
    assert_same((outs[0][:cases.BATCH], outs[1][:cases.BATCH]), want, "the first repetition")
    for got in outs:
        raw = got.view(np.uint8).reshape(len(got), -1)
        first = raw[:cases.BATCH]
        tiles = raw[:reps * cases.BATCH].reshape(reps, cases.BATCH, -1)
        assert all((tiles[q] == first).all() for q in range(reps)), "a later repetition differs from the first"
        assert (raw[reps * cases.BATCH: bound] == first[:tail]).all(), "the last, partial repetition differs"


def test_fuzzer_configurations_at_a_fixed_seed(eng):
    """tests/tools/manifold_fuzz.py at a fixed seed, each configuration from its own stream (seed, index): sixteen configurations,
    near-tied polygons among them"""
    spec = importlib.util.spec_from_file_location("manifold_fuzz", os.path.join(HERE, "tools", "manifold_fuzz.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    seen, compared = [], 0
    for i in range(16):
        ok, (desc, n) = fz.one(eng, np.random.default_rng([FUZZ_SEED, i]), i)
        assert ok, desc
        seen.append(desc)
        compared += n
    assert any("near-ties, polygons" in d for d in seen) and any("B = A" in d for d in seen), seen
    assert compared > 1000
    eng.check_async()
