"""GPU tests of the contact queries (c2d_poly_pair_contacts / c2d_rect_pair_contacts): every field of every contact equals
tests/contact_ref.py — the numpy restatement of the contract of include/c2d.h, pinned by tests/test_contact_ref_cpu.py — floats
bit for bit (+0 and -0 equal), and `hit` also equals the pairwise GPU path and the oracle.  Every output buffer handed to the
library sits between guard bands that are checked afterwards."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import contact_cases as cases  # noqa: E402
import contact_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 4            # guard records in front of and behind every output
BAND = 0xA5


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


class RectsOnDevice:
    def __init__(self, eng, planes):
        self.n = planes.shape[1]
        self.d = eng.to_device(planes)
        self.ptrs = [self.d.row(k) for k in range(8)]

    def free(self):
        self.d.free()


def run(eng, call, pairs, capacity=None, n_dev=None, expect_error=False):
    """call(d_pairs, capacity, d_out, d_n) queues the contacts call.  -> CONTACT_DT[capacity]: the output, taken from between two guard
    bands that must be intact; every record at or beyond min(capacity, n_dev) must be untouched as well (it reads as BAND bytes)."""
    cap = len(pairs) if capacity is None else capacity
    host_pairs = np.full((max(cap, 1), 2), 0xFFFFFFFF, np.uint32)   # entries beyond the list: indices no set has
    host_pairs[:len(pairs)] = pairs
    d_pairs = eng.to_device(host_pairs)
    d_out = eng.empty(cap + 2 * GUARD, ref.CONTACT_DT)
    eng.memset(d_out, BAND, d_out.nbytes)
    d_n = None if n_dev is None else eng.to_device(np.array([n_dev], np.uint64))
    try:
        call(d_pairs, cap, d_out.ptr + 16 * GUARD, d_n)
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
    raw = out.view(np.uint8).reshape(-1, 16)
    assert (raw[:GUARD] == BAND).all() and (raw[GUARD + cap:] == BAND).all(), "written outside the output"
    bound = cap if n_dev is None else min(cap, n_dev)
    assert (raw[GUARD + bound: GUARD + cap] == BAND).all(), "written at or beyond min(n_pairs, *d_n_pairs)"
    return out[GUARD: GUARD + cap]


def poly_call(eng, a, b, row_base=0, col_base=0):
    return lambda d_pairs, cap, out, d_n: eng.poly_pair_contacts(a, b, d_pairs, cap, out, n_pairs_dev=d_n, row_base=row_base, col_base=col_base)


def rect_call(eng, a, b, row_base=0, col_base=0):
    return lambda d_pairs, cap, out, d_n: eng.rect_pair_contacts(a.ptrs, a.n, b.ptrs, b.n, d_pairs, cap, out, n_pairs_dev=d_n, row_base=row_base,
                                                                 col_base=col_base)


def assert_same(got, want, what):
    ok = ref.same(got, want)
    if not ok.all():
        q = int(np.flatnonzero(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {len(want)} contacts differ; first at {q}: got {got[q]}, want {want[q]}")


def local(pairs):
    return pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)


def pairwise_gpu(eng, a, b, pairs):
    """the boolean of c2d_sat_poly_pairs_rows on the listed pairs (both sets in 16 rows)"""
    i, j = local(pairs)
    vx, vy = np.stack([a[0][:, i], b[0][:, j]]), np.stack([a[1][:, i], b[1][:, j]])
    k = np.stack([a[2][i], b[2][j]])
    d = [eng.to_device(x) for x in (vx, vy, k)]
    d_out = eng.zeros(len(pairs), np.uint8)
    eng.sat_poly_pairs_rows(*d, len(pairs), vx.shape[1], d_out)
    out = d_out.get()
    for x in d + [d_out]:
        x.free()
    return out


def oracle_hits(oracle, a, b, pairs):
    i, j = local(pairs)
    return oracle.sat_poly_pairs(np.stack([a[0][:, i], b[0][:, j]]), np.stack([a[1][:, i], b[1][:, j]]), np.stack([a[2][i], b[2][j]]))[0]


@pytest.fixture(scope="module")
def dense(wl, oracle):
    """two sets of about 300 polygons in a small box with the reference contacts of ALL their pairs, computed once"""
    a, b = cases.dense_poly_sets(wl)
    pairs = cases.all_pairs(a[0].shape[1], b[0].shape[1])
    want = ref.poly_contacts(a, b, *local(pairs))
    want.setflags(write=False)
    share = want["hit"].mean()
    assert 0.1 < share < 0.5, share
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


HARD = None


def hard_batches(wl):
    global HARD
    if HARD is None:
        HARD = cases.hard_poly_batches(wl)
    return HARD


@pytest.mark.parametrize("name", ["clockwise", "clockwise_both", "repeated_vertices", "k1_k2", "touching", "equal_shapes", "equal_boxes", "scale_1e30",
                                  "scale_1e-30", "scale_1e-42", "scale_1e18", "scale_1e-18", "non_finite_vertex0", "non_finite_later_vertex",
                                  "overflowing_len2"])
def test_hard_inputs(eng, oracle, wl, name):
    """one small batch per class; on the finite, non-overflowing ones hit == (depth >= 0) wherever an axis was usable"""
    a, b, pairs, finite = hard_batches(wl)[name]
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


def test_device_count_bounds_the_work(eng, dense):
    """n_pairs = capacity with the count on the device: smaller (only that many records are written), equal, larger (clamped to
    n_pairs), and no count at all.  run() checks the guard bands and every record beyond the bound."""
    a, b, pairs, want = dense
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    sel = np.arange(5, len(pairs), 311)[:300]
    for n_dev in (0, 1, 63, 64, 137, 299, 300, 301, 1 << 40, (1 << 64) - 1, None):
        got = run(eng, poly_call(eng, ua.set, ub.set), pairs[sel], capacity=300, n_dev=n_dev)
        bound = 300 if n_dev is None else min(300, n_dev)
        assert_same(got[:bound], want[sel][:bound], f"device count {n_dev}")
    # a capacity above the list, as a caller passes it: the count says where the list ends
    got = run(eng, poly_call(eng, ua.set, ub.set), pairs[sel], capacity=1000, n_dev=300)
    assert_same(got[:300], want[sel], "capacity 1000, count 300")
    eng.check_async()
    ua.free()
    ub.free()


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


def test_argument_errors(eng, pkg, wl):
    a = wl.random_convex_polygon_set(100, seed=5, extent=3.0)
    ua = Uploaded(eng, a)
    S = ua.set
    d_pairs = eng.zeros((16, 2), np.uint32)
    d_out = eng.zeros(16, ref.CONTACT_DT)
    d_n = eng.zeros(1, np.uint64)
    mk = lambda **kw: eng.poly_set(kw.get("vx", ua.px), kw.get("vy", ua.py), ua.dk, kw.get("n", 100), kw.get("rows", 16), kw.get("stride", 0))  # noqa: E731
    planes = [ua.px] * 8
    raw = eng.lib.c2d_poly_pair_contacts
    assert raw(eng.h, None, C.byref(S), d_pairs.ptr, 16, None, 0, 0, d_out.ptr, None) == -1
    assert raw(eng.h, C.byref(S), None, d_pairs.ptr, 16, None, 0, 0, d_out.ptr, None) == -1
    bad = [
        lambda: eng.poly_pair_contacts(mk(vx=0), S, d_pairs, 16, d_out),                       # a NULL plane
        lambda: eng.poly_pair_contacts(S, mk(vy=0), d_pairs, 16, d_out),
        lambda: eng.poly_pair_contacts(mk(rows=0), S, d_pairs, 16, d_out),                     # rows 0 or 17
        lambda: eng.poly_pair_contacts(S, mk(rows=17), d_pairs, 16, d_out),
        lambda: eng.poly_pair_contacts(mk(stride=99), S, d_pairs, 16, d_out),                  # stride < n
        lambda: eng.poly_pair_contacts(mk(vx=ua.px + 2), S, d_pairs, 16, d_out),               # a misaligned plane
        lambda: eng.poly_pair_contacts(S, S, None, 16, d_out),                                 # no list
        lambda: eng.poly_pair_contacts(S, S, d_pairs, 16, None),                               # no output
        lambda: eng.poly_pair_contacts(S, S, d_pairs, 15, d_out.ptr + 8),                      # output not 16-byte aligned
        lambda: eng.poly_pair_contacts(S, S, d_pairs.ptr + 2, 15, d_out),                      # list not 4-byte aligned
        lambda: eng.poly_pair_contacts(S, S, d_pairs, 16, d_out, n_pairs_dev=d_n.ptr + 4),     # count not 8-byte aligned
        lambda: eng.poly_pair_contacts(S, S, d_pairs, 16, d_out, row_base=1 << 62),            # bases beyond 2^62
        lambda: eng.poly_pair_contacts(S, S, d_pairs, 16, d_out, col_base=1 << 62),
        lambda: eng.rect_pair_contacts(planes[:7] + [0], 100, planes, 100, d_pairs, 16, d_out),
        lambda: eng.rect_pair_contacts(planes, 100, planes[:7] + [0], 100, d_pairs, 16, d_out),
        lambda: eng.rect_pair_contacts(planes, 100, planes, 100, None, 16, d_out),
        lambda: eng.rect_pair_contacts(planes, 100, planes, 100, d_pairs, 16, None),
        lambda: eng.rect_pair_contacts(planes, 100, planes, 100, d_pairs, 15, d_out.ptr + 4),
        lambda: eng.rect_pair_contacts(planes, 100, planes, 100, d_pairs, 16, d_out, col_base=1 << 62),
    ]
    for q, call in enumerate(bad):
        with pytest.raises(pkg.C2DError) as e:
            call()
        assert e.value.status == -1, q
    eng.poly_pair_contacts(S, S, None, 0, None)                      # n_pairs == 0: a no-op
    eng.rect_pair_contacts(planes, 100, planes, 100, None, 0, None)
    eng.synchronize()
    assert (d_out.get().view(np.uint8) == 0).all(), "a refused call wrote something"
    for x in (d_pairs, d_out, d_n, ua):
        x.free()


def test_graph_capture_follows_the_device_count():
    """One capture of a contacts call with d_n_pairs, replayed with different counts written to the device in between
    (tests/contact_graph_check.py, its own process: torch has to be imported before libc2d.so)."""
    out = subprocess.run([sys.executable, os.path.join(HERE, "contact_graph_check.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "contact graph ok" in out.stdout


def test_bad_pairs_read_nothing_and_are_reported_once(eng, wl):
    """Indices equal to n, 0xFFFFFFFF and below the base, in either column, and polygons with a vertex count of 0 and 17: those
    entries carry BAD_PAIR, every other entry is correct, and the error is reported once by the next synchronise.  The planes end
    where their allocations end; the guard (contact_kernel: `ranged`, `valid`) lets no such index reach a load."""
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
    want = ref.poly_contacts(a, b, listed[:, 0] - rb, listed[:, 1] - cb)
    assert (want["flags"][at] == ref.BAD_PAIR).all() and (want["flags"] == ref.BAD_PAIR).sum() > len(at)   # (the bad counts as well)
    assert (want["flags"] != ref.BAD_PAIR).sum() > 300
    eng.check_async()
    got = run(eng, poly_call(eng, sa, sb, row_base=rb, col_base=cb), listed.astype(np.uint32), expect_error=True)
    assert_same(got, want, "list with bad pairs")
    # the same with rectangles (no absent objects there: only the indices)
    ra = np.ascontiguousarray(np.concatenate([a[0][:4], a[1][:4]])[[0, 4, 1, 5, 2, 6, 3, 7]])
    da = RectsOnDevice(eng, ra)
    want = ref.rect_contacts(ra, ra, listed[:, 0] - rb, listed[:, 1] - cb)
    got = run(eng, rect_call(eng, da, da, row_base=rb, col_base=cb), listed.astype(np.uint32), expect_error=True)
    assert_same(got, want, "rectangle list with bad pairs")
    # a clean call afterwards reports nothing
    sound = good[(kb[good[:, 1] - cb] >= 1) & (kb[good[:, 1] - cb] <= 8)][:10]
    clean = run(eng, poly_call(eng, sa, sb, row_base=rb, col_base=cb), sound.astype(np.uint32))
    assert (clean["flags"] & ref.BAD_PAIR == 0).all()
    eng.check_async()
    for x in d + [da]:
        x.free()
