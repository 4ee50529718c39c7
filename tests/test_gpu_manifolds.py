"""GPU tests of c2d_poly_pair_manifolds: every field of both outputs equals tests/manifold_ref.py / tests/contact_ref.py — the numpy
restatements of the contracts of include/c2d.h, pinned by tests/test_manifold_ref_cpu.py and tests/test_contact_ref_cpu.py — floats
bit for bit (+0 and -0 equal, NaN equal to NaN), and the contact output equals c2d_poly_pair_contacts' on the same list byte for
byte.  Both output buffers sit between guard bands that are checked afterwards."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import contact_cases  # noqa: E402
import contact_ref  # noqa: E402
import manifold_cases as cases  # noqa: E402
import manifold_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 4            # guard records in front of and behind every output
BAND = 0xA5
LIST_LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 4099]


class Uploaded:
    """A polygon set on the device: every plane row shifted by `offset` floats, `stride` >= n elements between vertex rows, NaN in
    the gaps.  .set is the c2d_poly_set; .sub(r0, r1) the shard of polygons [r0, r1) (pointer offset, the same stride)."""

    def __init__(self, eng, s, offset=0, stride=None, with_k=True):
        vx, vy, k = s
        self.eng, self.rows, self.n = eng, vx.shape[0], vx.shape[1]
        self.stride = self.n if stride is None else stride
        host = np.full((2, self.rows * self.stride + offset), np.nan, np.float32)
        for p, v in enumerate((vx, vy)):
            for r in range(self.rows):
                host[p, offset + r * self.stride: offset + r * self.stride + self.n] = v[r]
        self.d = eng.to_device(host)
        self.px, self.py = self.d.row(0) + 4 * offset, self.d.row(1) + 4 * offset
        self.dk = eng.to_device(k) if (k is not None and with_k) else None
        self.set = self.sub(0, self.n)

    def sub(self, r0, r1):
        return self.eng.poly_set(self.px + 4 * r0, self.py + 4 * r0, None if self.dk is None else self.dk.ptr + r0, r1 - r0, self.rows, self.stride)

    def free(self):
        self.d.free()
        if self.dk is not None:
            self.dk.free()


def banded(eng, cap, dt):
    d = eng.empty(cap + 2 * GUARD, dt)
    eng.memset(d, BAND, d.nbytes)
    return d


def unband(d, cap, bound, dt):
    """the records between the guard bands; the bands and every record at or beyond `bound` must read as BAND bytes"""
    out = d.get()
    raw = out.view(np.uint8).reshape(-1, dt.itemsize)
    assert (raw[:GUARD] == BAND).all() and (raw[GUARD + cap:] == BAND).all(), "written outside the output"
    assert (raw[GUARD + bound: GUARD + cap] == BAND).all(), "written at or beyond min(n_pairs, *d_n_pairs)"
    return out[GUARD: GUARD + cap]


def run(eng, a, b, pairs, capacity=None, n_dev=None, row_base=0, col_base=0, expect_error=False):
    """-> (CONTACT_DT[capacity], MANIFOLD_DT[capacity]) of one c2d_poly_pair_manifolds call on the list; the contact output is
    also compared, byte for byte, with what c2d_poly_pair_contacts writes for the same arguments."""
    cap = len(pairs) if capacity is None else capacity
    host_pairs = np.full((max(cap, 1), 2), 0xFFFFFFFF, np.uint32)   # entries beyond the list: indices no set has
    host_pairs[:len(pairs)] = pairs
    d_pairs = eng.to_device(host_pairs)
    d_c, d_m, d_c2 = banded(eng, cap, contact_ref.CONTACT_DT), banded(eng, cap, ref.MANIFOLD_DT), banded(eng, cap, contact_ref.CONTACT_DT)
    d_n = None if n_dev is None else eng.to_device(np.array([n_dev], np.uint64))
    try:
        eng.poly_pair_manifolds(a, b, d_pairs, cap, d_c.ptr + 16 * GUARD, d_m.ptr + 32 * GUARD, n_pairs_dev=d_n, row_base=row_base, col_base=col_base)
        eng.poly_pair_contacts(a, b, d_pairs, cap, d_c2.ptr + 16 * GUARD, n_pairs_dev=d_n, row_base=row_base, col_base=col_base)
        if expect_error:
            with pytest.raises(Exception) as e:
                eng.synchronize()
            assert getattr(e.value, "status", None) == -1
            eng.synchronize()
            eng.check_async()      # reported once, then clear
        else:
            eng.synchronize()
        bound = cap if n_dev is None else min(cap, n_dev)
        got_c, got_m, alone = unband(d_c, cap, bound, contact_ref.CONTACT_DT), unband(d_m, cap, bound, ref.MANIFOLD_DT), unband(d_c2, cap, bound, contact_ref.CONTACT_DT)
    finally:
        for x in (d_pairs, d_c, d_m, d_c2, d_n):
            if x is not None:
                x.free()
    assert got_c.tobytes() == alone.tobytes(), "the contact output differs from c2d_poly_pair_contacts'"
    return got_c, got_m


def assert_same(got, want, what):
    for g, w, same, name in ((got[0], want[0], contact_ref.same, "contacts"), (got[1], want[1], ref.same, "manifolds")):
        ok = same(g, w)
        if not ok.all():
            q = int(np.flatnonzero(~ok)[0])
            raise AssertionError(f"{what}: {int((~ok).sum())} of {len(w)} {name} differ; first at {q}: got {g[q]}, want {w[q]}")
    assert (got[1]["reserved"] == 0).all()


def local(pairs):
    return pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)


def diag(n):
    return np.stack([np.arange(n), np.arange(n)], axis=1).astype(np.uint32)


@pytest.fixture(scope="module")
def dense(wl):
    """two sets of about 300 polygons in a small box and every 17th of their pairs (colliding and separated), with the reference"""
    a, b = contact_cases.dense_poly_sets(wl)
    pairs = contact_cases.all_pairs(a[0].shape[1], b[0].shape[1])[::17]
    want = ref.poly_manifolds(a, b, *local(pairs))
    for w in want:
        w.setflags(write=False)
    assert len(pairs) >= 4099 and 0.1 < want[0]["hit"].mean() < 0.5
    return a, b, pairs, want


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
        got = run(eng, ua.set, ub.set, pairs[:length])
        assert_same(got, (want[0][:length], want[1][:length]), f"list of {length}")
    assert_same(run(eng, ua.set, ub.set, pairs), want, "the whole list")
    eng.check_async()
    ua.free()
    ub.free()


def test_device_count_bounds_the_work(eng, dense):
    """n_pairs = capacity with the count on the device; run() checks the guard bands and every record of both outputs beyond the bound"""
    a, b, pairs, want = dense
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    for n_dev in (0, 1, 63, 64, 137, 299, 300, 301, (1 << 64) - 1):
        got = run(eng, ua.set, ub.set, pairs[:300], capacity=300, n_dev=n_dev)
        bound = min(300, n_dev)
        assert_same((got[0][:bound], got[1][:bound]), (want[0][:bound], want[1][:bound]), f"device count {n_dev}")
    got = run(eng, ua.set, ub.set, pairs[:300], capacity=1000, n_dev=300)
    assert_same((got[0][:300], got[1][:300]), (want[0][:300], want[1][:300]), "capacity 1000, count 300")
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
        assert_same(run(eng, ua.set, ub.set, pairs), ref.poly_manifolds(a, b, *local(pairs)), f"rows {ra} x {rb}")
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
        assert_same(run(eng, ux.set, uy.set, pairs), want, "k == rows, d_k == NULL")
        ux.free()
        uy.free()
    n = 150
    s = wl.random_convex_polygon_set(n, seed=9204, extent=3.0)
    us = Uploaded(eng, s, offset=1, stride=n + 5)
    pairs = contact_cases.all_pairs(n, n)[::5]
    assert_same(run(eng, us.set, us.set, pairs), ref.poly_manifolds(s, s, *local(pairs)), "the same memory")
    r0, r1, c0, c1, rb, cb = 37, 111, 20, 150, 1000, 4_000_000_000
    block = contact_cases.all_pairs(r1 - r0, c1 - c0)[::3]
    sub = (tuple(x[..., r0:r1] for x in s), tuple(x[..., c0:c1] for x in s))
    listed = (block.astype(np.int64) + (rb, cb)).astype(np.uint32)
    assert_same(run(eng, us.sub(r0, r1), us.sub(c0, c1), listed, row_base=rb, col_base=cb), ref.poly_manifolds(*sub, *local(block)), "shards with bases")
    eng.check_async()
    us.free()


HARD = None


@pytest.mark.parametrize("name", ["clockwise", "clockwise_both", "repeated_vertices", "k1_k2", "touching", "equal_shapes", "equal_boxes",
                                  "non_finite_vertex0", "non_finite_later_vertex", "scale_1e30", "scale_1e-42"])
def test_hard_inputs(eng, wl, name):
    """one small batch per class of tests/contact_cases.py"""
    global HARD
    if HARD is None:
        HARD = contact_cases.hard_poly_batches(wl)
    a, b, pairs, _ = HARD[name]
    want = ref.poly_manifolds(a, b, *local(pairs))
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    got = run(eng, ua.set, ub.set, pairs)
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
    assert_same(run(eng, ua.set, ub.set, diag(cases.BATCH)), want, "the diagonal")
    order = cases.shuffled()
    assert_same(run(eng, ua.set, ub.set, diag(cases.BATCH)[order]), (want[0][order], want[1][order]), "shuffled")
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
    assert_same(run(eng, ua.set, ub.set, pairs), ref.poly_manifolds(a, b, *local(pairs)), "scale sweep")
    eng.check_async()
    ua.free()
    ub.free()


def test_bad_pairs_read_nothing_and_are_reported_once(eng, wl):
    """indices outside their set in either column and polygons with a vertex count of 0 and 17: BAD_PAIR contacts with empty
    manifolds, every other entry correct, the error reported once; the planes end where their allocations end"""
    n_a, n_b, rb, cb = 50, 64, 1000, 5
    a = wl.random_convex_polygon_set(n_a, seed=8001, extent=2.5)
    b = wl.random_convex_polygon_set(n_b, seed=8002, kmax=8, extent=2.5, rows=8)
    kb = b[2].copy()
    kb[[3, 40]] = [0, 17]
    b = (b[0], b[1], kb)
    d = [eng.to_device(x) for x in (*a, *b)]
    sa, sb = eng.poly_set(d[0], d[1], d[2], n_a, 16), eng.poly_set(d[3], d[4], d[5], n_b, 8)
    good = contact_cases.all_pairs(n_a, n_b)[::7].astype(np.int64) + (rb, cb)
    bad = np.array([[rb + n_a, cb], [0xFFFFFFFF, cb + 1], [rb - 1, cb + 2], [rb + 1, cb + n_b], [rb + 2, 0xFFFFFFFF], [rb + 3, cb - 1],
                    [0, 0], [0xFFFFFFFF, 0xFFFFFFFF], [rb + n_a + 70, cb + 3]], np.int64)
    listed = good.copy()
    at = np.array([0, 1, 63, 64, 65, 200, 255, 256, len(good) - 1])
    listed[at] = bad
    want = ref.poly_manifolds(a, b, listed[:, 0] - rb, listed[:, 1] - cb)
    is_bad = want[0]["flags"] == contact_ref.BAD_PAIR
    assert is_bad[at].all() and is_bad.sum() > len(at) and (~is_bad).sum() > 300
    assert want[1][is_bad].tobytes() == ref.empty(int(is_bad.sum())).tobytes()
    eng.check_async()
    got = run(eng, sa, sb, listed.astype(np.uint32), row_base=rb, col_base=cb, expect_error=True)
    assert_same(got, want, "list with bad pairs")
    assert got[1][is_bad].tobytes() == ref.empty(int(is_bad.sum())).tobytes()
    sound = good[(kb[good[:, 1] - cb] >= 1) & (kb[good[:, 1] - cb] <= 8)][:10]
    run(eng, sa, sb, sound.astype(np.uint32), row_base=rb, col_base=cb)
    eng.check_async()
    for x in d:
        x.free()


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


def test_argument_errors(eng, pkg, wl):
    a = wl.random_convex_polygon_set(100, seed=5, extent=3.0)
    ua = Uploaded(eng, a)
    S = ua.set
    d_pairs = eng.zeros((16, 2), np.uint32)
    d_c = eng.zeros(16, contact_ref.CONTACT_DT)
    d_m = eng.zeros(16, ref.MANIFOLD_DT)
    d_n = eng.zeros(1, np.uint64)
    mk = lambda **kw: eng.poly_set(kw.get("vx", ua.px), kw.get("vy", ua.py), ua.dk, kw.get("n", 100), kw.get("rows", 16), kw.get("stride", 0))  # noqa: E731
    raw = eng.lib.c2d_poly_pair_manifolds
    assert raw(eng.h, None, C.byref(S), d_pairs.ptr, 16, None, 0, 0, d_c.ptr, d_m.ptr, None) == -1
    assert raw(eng.h, C.byref(S), None, d_pairs.ptr, 16, None, 0, 0, d_c.ptr, d_m.ptr, None) == -1
    call = eng.poly_pair_manifolds
    bad = [
        lambda: call(mk(vx=0), S, d_pairs, 16, d_c, d_m),                           # a NULL plane
        lambda: call(S, mk(vy=0), d_pairs, 16, d_c, d_m),
        lambda: call(mk(rows=0), S, d_pairs, 16, d_c, d_m),                         # rows 0 or 17
        lambda: call(S, mk(rows=17), d_pairs, 16, d_c, d_m),
        lambda: call(mk(stride=99), S, d_pairs, 16, d_c, d_m),                      # stride < n
        lambda: call(mk(vx=ua.px + 2), S, d_pairs, 16, d_c, d_m),                   # a misaligned plane
        lambda: call(S, S, None, 16, d_c, d_m),                                     # no list
        lambda: call(S, S, d_pairs, 16, None, d_m),                                 # either output missing
        lambda: call(S, S, d_pairs, 16, d_c, None),
        lambda: call(S, S, d_pairs, 15, d_c.ptr + 8, d_m),                          # either output not 16-byte aligned
        lambda: call(S, S, d_pairs, 15, d_c, d_m.ptr + 8),
        lambda: call(S, S, d_pairs.ptr + 2, 15, d_c, d_m),                          # list not 4-byte aligned
        lambda: call(S, S, d_pairs, 16, d_c, d_m, n_pairs_dev=d_n.ptr + 4),         # count not 8-byte aligned
        lambda: call(S, S, d_pairs, 16, d_c, d_m, row_base=1 << 62),                # bases beyond 2^62
        lambda: call(S, S, d_pairs, 16, d_c, d_m, col_base=1 << 62),
    ]
    for q, f in enumerate(bad):
        with pytest.raises(pkg.C2DError) as e:
            f()
        assert e.value.status == -1, q
    call(S, S, None, 0, None, None)                      # n_pairs == 0: a no-op
    eng.synchronize()
    assert (d_c.get().view(np.uint8) == 0).all() and (d_m.get().view(np.uint8) == 0).all(), "a refused call wrote something"
    for x in (d_pairs, d_c, d_m, d_n, ua):
        x.free()


def test_graph_capture_follows_the_device_count():
    """One capture of a manifolds call with d_n_pairs, replayed with different counts written to the device in between
    (tests/manifold_graph_check.py, its own process: torch has to be imported before libc2d.so)."""
    out = subprocess.run([sys.executable, os.path.join(HERE, "manifold_graph_check.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "manifold graph ok" in out.stdout


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
    host_pairs = np.tile(diag(cases.BATCH), (n // cases.BATCH + 1, 1))[:n]
    d_pairs = eng.to_device(host_pairs)
    del host_pairs
    d_c, d_m = banded(eng, n, contact_ref.CONTACT_DT), banded(eng, n, ref.MANIFOLD_DT)
    d_n = None if n_dev is None else eng.to_device(np.array([n_dev], np.uint64))
    try:
        eng.poly_pair_manifolds(ua.set, ub.set, d_pairs, n, d_c.ptr + 16 * GUARD, d_m.ptr + 32 * GUARD, n_pairs_dev=d_n)
        eng.synchronize()
        eng.check_async()
        outs = [unband(d_c, n, bound, contact_ref.CONTACT_DT), unband(d_m, n, bound, ref.MANIFOLD_DT)]
    finally:
        for x in (d_pairs, d_c, d_m, d_n, ua, ub):
            if x is not None:
                x.free()
    assert_same((outs[0][:cases.BATCH], outs[1][:cases.BATCH]), want, "the first repetition")
    for got in outs:
        raw = got.view(np.uint8).reshape(len(got), -1)
        first = raw[:cases.BATCH]
        tiles = raw[:reps * cases.BATCH].reshape(reps, cases.BATCH, -1)
        assert all((tiles[q] == first).all() for q in range(reps)), "a later repetition differs from the first"
        assert (raw[reps * cases.BATCH: bound] == first[:tail]).all(), "the last, partial repetition differs"
