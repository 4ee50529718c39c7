"""GPU tests of the swept queries (c2d_poly_pair_sweeps / c2d_rect_pair_sweeps): every field of every record equals
tests/sweep_ref.py — the numpy restatement of the contract of include/c2d.h, pinned by tests/test_sweep_ref_cpu.py — floats bit for
bit (+0 and -0 equal).  Every output buffer handed to the library sits between guard bands that are checked afterwards
(pair_list_harness.run).  What every list-driven query promises of its list is tests/test_gpu_pair_list_contract.py's, for the sweeps
as for the others; the last test here is what the sweeps alone refuse: half a motion, a misaligned plane."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import contact_cases as cases  # noqa: E402
import sweep_ref as ref  # noqa: E402
import pair_list_harness as h  # noqa: E402
from pair_list_harness import BAND, Motion, RectsOnDevice, Uploaded, local, motions, pairwise_gpu, rect_pairwise_gpu  # noqa: E402

pytestmark = pytest.mark.gpu
FUZZ_SEED = 20264
F = np.float32
LIST_LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 4099]
Q = h.SWEEPS
run, poly_call, rect_call, assert_same, classes = Q.run, Q.poly_call, Q.rect_call, Q.assert_same, h.sweep_classes


@pytest.fixture(scope="module")
def dense(wl):
    """the dense sets (300 x 311 polygons), both moving by up to +-4 per component, with the reference records of ALL their pairs,
    computed once and read-only (pair_list_harness.dense: every class of record has its share) -> a, b, pairs, ma, mb, want"""
    a, b, pairs, want = h.dense(wl, Q)
    return (a, b, pairs, *h.dense_extras(Q), want)


def test_values_for_every_list_length(eng, dense):
    """Lists of 0, 1, 63, 64, 65, 255, 256, 257 and 4099 entries cut from the all-pairs enumeration: start-overlap pairs only (every
    wave skips the axis walk), pairs without start overlap only, and every 17th pair (mixed waves)."""
    a, b, pairs, ma, mb, want = dense
    ua, ub, da, db = Uploaded(eng, a), Uploaded(eng, b), Motion(eng, ma), Motion(eng, mb)
    start = (want["flags"] & ref.START_OVERLAP) != 0
    starts, others = np.flatnonzero(start), np.flatnonzero(~start)
    mixed = np.arange(0, len(pairs), 17)
    assert len(starts) >= 4099 and len(others) >= 4099 and len(mixed) >= 4099 and 0.1 < start[mixed].mean() < 0.5
    assert (want["hit"][others[:4099]] == 1).sum() > 100
    call = poly_call(eng, ua.set, ub.set, a_motion=da.ptrs, b_motion=db.ptrs)
    for length in LIST_LENGTHS:
        for name, sel in (("start overlap", starts[-length:] if length else starts[:0]), ("no start overlap", others[:length]), ("mixed", mixed[:length])):
            assert_same(run(eng, call, pairs[sel]), want[sel], f"{name} list of {length}")
    eng.check_async()
    for x in (ua, ub, da, db):
        x.free()


def test_dense_batch_in_order_and_shuffled(eng, dense):
    """All 93 300 pairs row-major (long runs of one row per wave), and the same list in a fixed shuffle: a wave then mixes rows, axes,
    signs and the three classes.  Twice: the call is deterministic."""
    a, b, pairs, ma, mb, want = dense
    ua, ub, da, db = Uploaded(eng, a), Uploaded(eng, b), Motion(eng, ma), Motion(eng, mb)
    call = poly_call(eng, ua.set, ub.set, a_motion=da.ptrs, b_motion=db.ptrs)
    got = run(eng, call, pairs)
    assert_same(got, want, "all pairs")
    assert run(eng, call, pairs).tobytes() == got.tobytes(), "two runs differ"
    assert np.array_equal((got["flags"] & ref.START_OVERLAP) != 0, pairwise_gpu(eng, a, b, pairs) == 1), "START_OVERLAP differs from c2d_sat_poly_pairs_rows"
    order = np.random.default_rng(8301).permutation(len(pairs))
    assert_same(run(eng, call, pairs[order]), want[order], "all pairs, shuffled")
    eng.check_async()
    for x in (ua, ub, da, db):
        x.free()


def test_motion_on_one_side_only_and_none_at_all(eng, dense):
    """b_motion None, a_motion None, both None, and planes that are all zero (the walk is skipped where nothing moves: the answer is
    hit0 or a miss).  With nothing moving, hit equals the pairwise GPU boolean."""
    a, b, pairs, ma, mb, _ = dense
    pairs = pairs[::7]
    ua, ub, da, db = Uploaded(eng, a), Uploaded(eng, b), Motion(eng, ma), Motion(eng, mb)
    zero_a, zero_b = (np.zeros(300, F),) * 2, (np.zeros(311, F),) * 2
    dza, dzb = Motion(eng, zero_a), Motion(eng, zero_b)
    boolean = pairwise_gpu(eng, a, b, pairs)
    for name, (ha, hb), (pa, pb) in (("only A moves", (ma, None), (da.ptrs, None)), ("only B moves", (None, mb), (None, db.ptrs)),
                                     ("no planes", (None, None), (None, None)), ("zero planes", (zero_a, zero_b), (dza.ptrs, dzb.ptrs)),
                                     ("A zero planes, B none", (zero_a, None), (dza.ptrs, None)), ("A moves, B zero planes", (ma, zero_b), (da.ptrs, dzb.ptrs))):
        want = ref.poly_sweeps(a, b, *local(pairs), ha, hb)
        got = run(eng, poly_call(eng, ua.set, ub.set, a_motion=pa, b_motion=pb), pairs)
        assert_same(got, want, name)
        if "moves" not in name:
            assert np.array_equal(got["hit"], boolean), name
            assert np.array_equal(got["flags"] == ref.START_OVERLAP, boolean == 1) and np.isinf(got["toi"][boolean == 0]).all(), name
        else:
            assert all(c.mean() > 0.03 for c in classes(want)), name
    eng.check_async()
    for x in (ua, ub, da, db, dza, dzb):
        x.free()


def test_layout_variants(eng, wl):
    """rows 4, 8 and 16 on either side (different rows for A and B), k == rows with d_k == NULL, stride > n with the planes shifted by
    one float (the motion planes by three), A and B the same memory, and shards with row_base / col_base whose motion planes are
    offset with them."""
    for ra, rb in ((4, 4), (4, 16), (8, 4), (16, 8), (8, 8)):
        a, b = cases.dense_poly_sets(wl, n=90, extent=3.0, rows_a=ra, rows_b=rb, seeds=(7500 + ra, 7600 + rb))
        pairs = cases.all_pairs(90, 101)[::3]
        ma, mb = motions(9300 + ra + rb, 90, 101, 3.0)
        want = ref.poly_sweeps(a, b, *local(pairs), ma, mb)
        assert all(c.mean() > 0.03 for c in classes(want))
        ua, ub = Uploaded(eng, a, offset=1, stride=90 + 7), Uploaded(eng, b, offset=1, stride=101 + 3)
        da, db = Motion(eng, ma, offset=3), Motion(eng, mb, offset=3)
        assert_same(run(eng, poly_call(eng, ua.set, ub.set, a_motion=da.ptrs, b_motion=db.ptrs), pairs), want, f"rows {ra} x {rb}")
        for x in (ua, ub, da, db):
            x.free()
    # every polygon has exactly `rows` vertices (the closing edge is slot 16 = slot 0 at rows = 16): no count plane on A, on B, on both
    a = wl.random_convex_polygon_set(80, seed=7701, kmin=16, kmax=16, extent=3.0, rows=16)
    b = wl.random_convex_polygon_set(90, seed=7702, kmin=4, kmax=4, extent=3.0, rows=4)
    c = wl.random_convex_polygon_set(90, seed=7703, extent=3.0)
    d = wl.random_convex_polygon_set(80, seed=7705, kmin=8, kmax=8, extent=3.0, rows=8)
    for x, y in ((a, c), (c, b), (a, b), (d, a)):
        pairs = cases.all_pairs(x[0].shape[1], y[0].shape[1])[::2]
        mx, my = motions(9400, x[0].shape[1], y[0].shape[1], 3.0)
        want = ref.poly_sweeps(x, y, *local(pairs), mx, my)
        assert all(cl.mean() > 0.02 for cl in classes(want))
        ux, uy = Uploaded(eng, x, with_k=x is c), Uploaded(eng, y, with_k=y is c)
        dx, dy = Motion(eng, mx), Motion(eng, my)
        assert (ux.dk is None) or (uy.dk is None)
        assert_same(run(eng, poly_call(eng, ux.set, uy.set, a_motion=dx.ptrs, b_motion=dy.ptrs), pairs), want, "d_k == NULL")
        for z in (ux, uy, dx, dy):
            z.free()
    # one set against itself (the same vertex memory and the same motion planes: r = 0 on the diagonal), and shards of it with their bases
    n = 150
    s = wl.random_convex_polygon_set(n, seed=7704, extent=3.0)
    ms, _ = motions(9401, n, 1, 3.0)
    us, ds = Uploaded(eng, s, offset=1, stride=n + 5), Motion(eng, ms, offset=1)
    pairs = cases.all_pairs(n, n)[::5]
    want = ref.poly_sweeps(s, s, *local(pairs), ms, ms)
    assert_same(run(eng, poly_call(eng, us.set, us.set, a_motion=ds.ptrs, b_motion=ds.ptrs), pairs), want, "the same memory")
    diag = want[pairs[:, 0] == pairs[:, 1]]
    assert len(diag) > 10 and (diag["flags"] == ref.START_OVERLAP).all()
    r0, r1, c0, c1, rb, cb = 37, 111, 20, 150, 1000, 4_000_000_000
    block = cases.all_pairs(r1 - r0, c1 - c0)[::3]
    sub = (tuple(x[..., r0:r1] for x in s), tuple(x[..., c0:c1] for x in s))
    want = ref.poly_sweeps(*sub, *local(block), tuple(m[r0:r1] for m in ms), tuple(m[c0:c1] for m in ms))
    assert all(cl.mean() > 0.02 for cl in classes(want))
    listed = (block.astype(np.int64) + (rb, cb)).astype(np.uint32)
    call = poly_call(eng, us.sub(r0, r1), us.sub(c0, c1), a_motion=ds.sub(r0), b_motion=ds.sub(c0), row_base=rb, col_base=cb)
    assert_same(run(eng, call, listed), want, "shards with bases")
    eng.check_async()
    us.free()
    ds.free()


HARD_NAMES = ["clockwise", "clockwise_both", "repeated_vertices", "k1_k2", "touching", "equal_shapes", "equal_boxes", "scale_1e30", "scale_1e-30",
              "scale_1e-42", "scale_1e18", "scale_1e-18", "non_finite_vertex0", "non_finite_later_vertex", "overflowing_len2"]


def batch_scale(a, b):
    """the size of a batch's own coordinates: the median magnitude of its finite, non-zero vertex coordinates"""
    c = np.abs(np.concatenate([x.ravel() for x in (a[0], a[1], b[0], b[1])]).astype(np.float64))
    c = c[np.isfinite(c) & (c > 0)]
    return float(np.median(c))


@pytest.mark.parametrize("name", HARD_NAMES)
def test_hard_inputs(eng, wl, name):
    """one small batch per class of tests/contact_cases.py, both sets moving by up to twice the batch's own coordinate scale: where
    masking the padding, the closing edge, k = 1 / 2, exact ties, overflow, underflow and non-finite input go wrong"""
    a, b, pairs, finite = h.hard_batches(wl)[name]
    assert sorted(h.hard_batches(wl)) == sorted(HARD_NAMES), "a batch of hard_poly_batches is not run"
    scale = batch_scale(a, b)
    ma, mb = motions(9500 + HARD_NAMES.index(name), a[0].shape[1], b[0].shape[1], 2.0 * scale)
    want = ref.poly_sweeps(a, b, *local(pairs), ma, mb)
    ua, ub, da, db = Uploaded(eng, a), Uploaded(eng, b), Motion(eng, ma), Motion(eng, mb)
    got = run(eng, poly_call(eng, ua.set, ub.set, a_motion=da.ptrs, b_motion=db.ptrs), pairs)
    for x in (ua, ub, da, db):
        x.free()
    assert_same(got, want, name)
    start, moving, miss = classes(got)
    assert np.array_equal(start, pairwise_gpu(eng, a, b, pairs) == 1)
    assert (got["flags"] & ref.BAD_PAIR == 0).all()
    # (at 1e-30 and 1e-42 every product underflows and no axis separates: all start overlap; at 1e30 the overlaps overflow and no
    # moving pair misses, 416 of them hitting at +0 with no axis)
    if name not in ("touching", "equal_boxes", "scale_1e30", "scale_1e-30", "scale_1e-42"):
        assert moving.sum() > 20 and miss.sum() > 20, (name, int(moving.sum()), int(miss.sum()))
    if name == "scale_1e30":
        assert (moving & (got["axis"] == 0xFFFF) & (got["toi"] == 0)).sum() > 100
    if finite:
        assert (got["axis"][moving] != 0xFFFF).all() and (got["toi"][moving] > 0).all() and (got["toi"][moving] <= 1).all()
    if name in ("touching", "equal_boxes"):
        assert start[:100].all()
    eng.check_async()


def grid_boxes(n=2048, seed=8303):
    """boxes on a 1/64 grid, each starting at a random vertex, B at an exact gap beside, above or diagonal to A; the motions are
    multiples of 1/16 up to 4: every quotient of the rule is a ratio of small integers, parallel faces tie exactly and diagonal
    passes graze -> (a, b) as 4-gon sets, (a, b) as planes f32[8][n], (ma, mb)"""
    rng = np.random.default_rng(seed)
    g = lambda lo, hi: rng.integers(int(lo * 64), int(hi * 64) + 1, n) / 64.0  # noqa: E731
    x0, y0, wa, ha, wb, hb = g(-4, 4), g(-4, 4), g(0.25, 2), g(0.25, 2), g(0.25, 2), g(0.25, 2)
    gx, gy = g(1 / 64, 1) * rng.choice([-1, 0, 1], n), g(1 / 64, 1) * rng.choice([-1, 0, 1], n)
    bx = np.where(gx > 0, x0 + wa + gx, np.where(gx < 0, x0 + gx - wb, x0 + g(-1, 1)))
    by = np.where(gy > 0, y0 + ha + gy, np.where(gy < 0, y0 + gy - hb, y0 + g(-1, 1)))
    corner = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float64)
    out = []
    for px, py, w, hh in ((x0, y0, wa, ha), (bx, by, wb, hb)):
        first = rng.integers(0, 4, n)
        c = corner[(first[:, None] + np.arange(4)[None, :]) % 4]
        out.append(np.stack([px[:, None] + w[:, None] * c[..., 0], py[:, None] + hh[:, None] * c[..., 1]], axis=-1))
    m = lambda: (rng.integers(-64, 65, n) / 16.0).astype(F)  # noqa: E731
    four = np.full(n, 4)
    return ((cases._as_poly_set(out[0], four, rows=4), cases._as_poly_set(out[1], four, rows=4)), (cases._as_planes(out[0]), cases._as_planes(out[1])),
            ((m(), m()), (m(), m())))


def test_boxes_on_a_grid_with_motions_on_a_binary_grid(eng):
    """grid_boxes as 4-gons through the polygon call and as planes through the rectangle call: exact ties among the axes, the winner
    among them the rule's first.  The two calls walk different axes (normals against edge vectors) and agree on hit and toi."""
    (pa, pb), (ra, rb), (ma, mb) = grid_boxes()
    n = pa[0].shape[1]
    pairs = h.diag(n)
    want = ref.poly_sweeps(pa, pb, *local(pairs), ma, mb)
    want_r = ref.rect_sweeps(ra, rb, *local(pairs), ma, mb)
    assert all(c.mean() > 0.05 for c in classes(want))
    assert np.array_equal(want["hit"], want_r["hit"]) and np.array_equal(want["toi"], want_r["toi"]) and np.array_equal(want["flags"], want_r["flags"])
    da, db = Motion(eng, ma), Motion(eng, mb)
    ua, ub = Uploaded(eng, pa), Uploaded(eng, pb)
    assert_same(run(eng, poly_call(eng, ua.set, ub.set, a_motion=da.ptrs, b_motion=db.ptrs), pairs), want, "boxes as 4-gons")
    ua.free()
    ub.free()
    xa, xb = RectsOnDevice(eng, ra), RectsOnDevice(eng, rb)
    assert_same(run(eng, rect_call(eng, xa, xb, a_motion=da.ptrs, b_motion=db.ptrs), pairs), want_r, "boxes as planes")
    for x in (xa, xb, da, db):
        x.free()
    eng.check_async()


def test_rectangles(eng, oracle, wl):
    """About 500 rectangles per set: every list length of a mixed list, motion on one side only and none, shards with bases (the
    motion planes offset with them), quads that are no rectangles, and a batch with non-finite vertices."""
    ra, rb = cases.rect_sets(oracle, wl)
    ma, mb = motions(9601, 500, 500, 6.0)
    xa, xb, da, db = RectsOnDevice(eng, ra), RectsOnDevice(eng, rb), Motion(eng, ma), Motion(eng, mb, offset=1)
    mixed = cases.all_pairs(500, 500)[::41]
    want = ref.rect_sweeps(ra, rb, *local(mixed), ma, mb)
    assert len(mixed) >= 4099 and all(c.mean() > 0.02 for c in classes(want))
    call = rect_call(eng, xa, xb, a_motion=da.ptrs, b_motion=db.ptrs)
    for length in LIST_LENGTHS:
        assert_same(run(eng, call, mixed[:length]), want[:length], f"list of {length}")
    boolean = rect_pairwise_gpu(eng, ra, rb, mixed)
    assert np.array_equal(want["flags"] == ref.START_OVERLAP, boolean == 1)
    for name, (ha, hb), (pa, pb) in (("only A moves", (ma, None), (da.ptrs, None)), ("only B moves", (None, mb), (None, db.ptrs)),
                                     ("no planes", (None, None), (None, None))):
        got = run(eng, rect_call(eng, xa, xb, a_motion=pa, b_motion=pb), mixed)
        assert_same(got, ref.rect_sweeps(ra, rb, *local(mixed), ha, hb), name)
        if ha is None and hb is None:
            assert np.array_equal(got["hit"], boolean)
    rb0, cb0 = 70_000, 12
    shard = cases.all_pairs(100, 80)[::3]
    d_sa, d_sb = RectsOnDevice(eng, ra[:, 200:300]), RectsOnDevice(eng, rb[:, 40:120])
    listed = (shard.astype(np.int64) + (rb0, cb0)).astype(np.uint32)
    want = ref.rect_sweeps(ra[:, 200:300], rb[:, 40:120], *local(shard), tuple(m[200:300] for m in ma), tuple(m[40:120] for m in mb))
    assert_same(run(eng, rect_call(eng, d_sa, d_sb, a_motion=da.sub(200), b_motion=db.sub(40), row_base=rb0, col_base=cb0), listed), want, "shards with bases")
    qa, qb = cases.quad_sets()
    nf = wl.inject_non_finite(ra[:, :200], seed=7801, frac=0.3)
    grid = cases.all_pairs(200, 200)[::3]
    i, j = local(grid)
    qm = motions(9602, 200, 200, 5.0)
    dqa, dqb = Motion(eng, qm[0]), Motion(eng, qm[1])
    for name, (sa, sb) in {"quads": (qa, qb), "non-finite": (nf, qb)}.items():
        d_x, d_y = RectsOnDevice(eng, sa), RectsOnDevice(eng, sb)
        got = run(eng, rect_call(eng, d_x, d_y, a_motion=dqa.ptrs, b_motion=dqb.ptrs), grid)
        assert_same(got, ref.rect_sweeps(sa, sb, i, j, *qm), name)
        assert np.array_equal(got["flags"] == ref.START_OVERLAP, rect_pairwise_gpu(eng, sa, sb, grid) == 1), name
        d_x.free()
        d_y.free()
    for x in (xa, xb, d_sa, d_sb, da, db, dqa, dqb):
        x.free()
    eng.check_async()


def test_pipeline_from_the_list_calls(eng, wl):
    """Broad list -> sweeps on one stream with the list's device count and no read-back in between: every listed pair starts in
    overlap.  And the full cross enumeration of two small sets (a caller's own list: all pairs) -> sweeps: what a planner asks."""
    n = 4099
    a = wl.random_convex_polygon_set(n, seed=7901, extent=70.0)
    ma, _ = motions(9701, n, 1, 2.0)
    ua, da = Uploaded(eng, a), Motion(eng, ma)
    cross = eng.poly_cross_pairs_host(*a, *a, upper=True)
    cap = len(cross) + 100
    assert len(cross) > 1000
    d_pairs, d_cnt = eng.empty((cap, 2), np.uint32), eng.zeros(1, np.uint64)
    d_out = eng.empty(cap, ref.SWEEP_DT)
    eng.memset(d_out, BAND, d_out.nbytes)
    eng.sat_poly_broad_pairs(ua.set, ua.set, d_pairs, cap, d_cnt, upper=True)
    eng.poly_pair_sweeps(ua.set, ua.set, d_pairs, cap, d_out, a_motion=da.ptrs, b_motion=da.ptrs, n_pairs_dev=d_cnt)
    eng.synchronize()
    out, listed = d_out.get(), d_pairs.get()[:len(cross)]
    assert int(d_cnt.get()[0]) == len(cross) and np.array_equal(listed, cross)
    assert_same(out[:len(cross)], ref.poly_sweeps(a, a, *local(cross), ma, ma), "broad list -> sweeps")
    assert (out["flags"][:len(cross)] == ref.START_OVERLAP).all() and (out[len(cross):].view(np.uint8) == BAND).all()
    for x in (d_pairs, d_cnt, d_out, ua, da):
        x.free()
    s, t = cases.dense_poly_sets(wl, n=40, extent=6.0, seeds=(7905, 7906))
    pairs = cases.all_pairs(40, 51)
    ms, mt = motions(9702, 40, 51, 6.0)
    us, ut, ds, dtm = Uploaded(eng, s), Uploaded(eng, t), Motion(eng, ms), Motion(eng, mt)
    got = run(eng, poly_call(eng, us.set, ut.set, a_motion=ds.ptrs, b_motion=dtm.ptrs), pairs)
    assert_same(got, ref.poly_sweeps(s, t, *local(pairs), ms, mt), "all pairs of two small sets")
    first = got["toi"].reshape(40, 51).min(axis=1)        # each A's first touch with any B during the step
    assert (first >= 0).all() and np.isinf(first).any() and (first == 0).any() and classes(got)[1].sum() > 50
    for x in (us, ut, ds, dtm):
        x.free()
    eng.check_async()


def test_list_longer_than_one_grid(eng, oracle, wl):
    """2^24 + 197 entries (a 4099-entry mixed list of the rectangle batch, tiled): the launch is capped at 65 536 blocks of 256, so
    the last 197 entries are the second trip of the grid-stride loop.  Once without a device count, once with 2^24 + 70: the
    127 records beyond it keep the band bytes (run() checks them).  The whole output is compared."""
    ra, rb = cases.rect_sets(oracle, wl)
    ma, mb = motions(9601, 500, 500, 6.0)
    mixed = cases.all_pairs(500, 500)[::41][:4099]
    want = ref.rect_sweeps(ra, rb, *local(mixed), ma, mb)
    assert len(mixed) == 4099 and all(c.mean() > 0.02 for c in classes(want))
    total = (1 << 24) + 197
    tile = np.arange(total) % 4099
    listed = mixed[tile]
    want32 = np.ascontiguousarray(want).view(np.uint32).reshape(-1, 4)
    xa, xb, da, db = RectsOnDevice(eng, ra), RectsOnDevice(eng, rb), Motion(eng, ma), Motion(eng, mb)
    for n_dev in (None, (1 << 24) + 70):
        bound = total if n_dev is None else n_dev
        got = run(eng, rect_call(eng, xa, xb, a_motion=da.ptrs, b_motion=db.ptrs), listed, n_dev=n_dev)[:bound]
        got32 = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 4)
        whole = bound // 4099 * 4099
        differs = np.concatenate([(got32[:whole].reshape(-1, 4099, 4) != want32[None]).any(axis=2).ravel(),
                                  (got32[whole:] != want32[:bound - whole]).any(axis=1)])
        at = np.flatnonzero(differs)        # not the same bytes: +0 against -0 is still the same record
        if len(at):
            ok = ref.same(got[at], want[tile[at]])
            assert ok.all(), (f"device count {n_dev}: {int((~ok).sum())} of {bound} records differ; first at entry {int(at[~ok][0])}: "
                              f"got {got[at[~ok][0]]}, want {want[tile[at[~ok][0]]]}")
    for x in (xa, xb, da, db):
        x.free()
    eng.check_async()


def test_fuzzer_configurations_at_a_fixed_seed(eng):
    """tests/tools/sweep_fuzz.py at a fixed seed, each configuration from its own stream (seed, index): sixteen configurations,
    polygons and rectangles and every kind of motion among them"""
    spec = importlib.util.spec_from_file_location("sweep_fuzz", os.path.join(HERE, "tools", "sweep_fuzz.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    seen, compared, moving = [], 0, 0
    for i in range(16):
        ok, (desc, bound) = fz.one(eng, np.random.default_rng([FUZZ_SEED, i]), i)
        assert ok, desc
        seen.append(desc)
        compared += bound
        moving += fz.LAST["moving_hits"]
    assert any("polygons" in d for d in seen) and any("rectangles" in d for d in seen), seen
    assert all(any(f"motion A {k}" in d or f"B {k}" in d for d in seen) for k in fz.MOTIONS), seen
    assert compared > 1000 and moving > 50
    eng.check_async()


def test_motion_argument_errors(eng, wl):
    """What the sweeps refuse beyond the forms of every list-driven query (tests/test_gpu_pair_list_contract.py): a set's motion with
    exactly one plane, or a misaligned one — on the C calls (the Python mirror refuses a half motion itself), with -1, nothing
    written, and in front of the n_pairs == 0 no-op, which a sound motion on one set alone passes."""
    ua = Uploaded(eng, wl.random_convex_polygon_set(100, seed=5, extent=3.0))
    S = ua.set
    d_pairs = eng.zeros((16, 2), np.uint32)
    d_out = eng.zeros(16, ref.SWEEP_DT)
    dm = Motion(eng, (np.ones(100, F), np.ones(100, F)))
    M = dm.ptrs
    planes = [ua.px] * 8
    cplanes = (C.c_void_p * 8)(*planes)
    raw_poly, raw_rect = eng.lib.c2d_poly_pair_sweeps, eng.lib.c2d_rect_pair_sweeps
    for m4 in ((M[0], None, None, None), (None, M[1], None, None), (M[0], M[1], M[0], None), (None, None, None, M[1]),      # one NULL plane of a set
               (M[0] + 2, M[1], None, None), (None, None, M[0], M[1] + 1)):                                                  # a misaligned plane
        assert raw_poly(eng.h, C.byref(S), C.byref(S), *m4, d_pairs.ptr, 16, None, 0, 0, d_out.ptr, None) == -1, m4
        assert raw_rect(eng.h, cplanes, 100, cplanes, 100, *m4, d_pairs.ptr, 16, None, 0, 0, d_out.ptr, None) == -1, m4
        assert raw_poly(eng.h, C.byref(S), C.byref(S), *m4, None, 0, None, 0, 0, None, None) == -1, m4        # refused in front of the n_pairs == 0 no-op
    eng.poly_pair_sweeps(S, S, None, 0, None, M, None)                      # n_pairs == 0: a no-op
    eng.rect_pair_sweeps(planes, 100, planes, 100, None, 0, None)
    eng.synchronize()
    assert (d_out.get().view(np.uint8) == 0).all(), "a refused call wrote something"
    for x in (d_pairs, ua, d_out, dm):
        x.free()
