"""The one frame of the tests of the list-driven queries (contacts, manifolds, distances, sweeps), as csrc/c2d_pair_list.hpp is the one
frame of their kernels: the uploads, the pairwise GPU paths, run() with its guard bands, and the table QUERIES of what each query
states of its own.  A plain module (pytest does not collect it) on numpy, pytest and the numpy references only: it never loads
libc2d.so, so tests/pair_list_graph_check.py can import it after torch.  tests/test_pair_list_harness_cpu.py drives run() without a
device."""
import functools

import numpy as np
import pytest

import contact_cases
import contact_ref
import distance_ref
import manifold_ref
import sweep_ref

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


class Motion:
    """The motion of a set on the device: two planes f32[n], each behind `offset` floats of NaN.  .ptrs = (dx, dy), the a_motion /
    b_motion of the Engine methods; .sub(r0) the planes of the shard that starts at object r0.  apart: each plane is an exact
    allocation of its own (nothing behind its last element)."""

    def __init__(self, eng, m, offset=0, apart=False):
        host = np.full((2, len(m[0]) + offset), np.nan, np.float32)
        host[0, offset:], host[1, offset:] = m[0], m[1]
        self.d = [eng.to_device(host[0]), eng.to_device(host[1])] if apart else [eng.to_device(host)]
        self.ptrs = tuple(p + 4 * offset for p in ((self.d[0].ptr, self.d[1].ptr) if apart else (self.d[0].row(0), self.d[0].row(1))))

    def sub(self, r0):
        return self.ptrs[0] + 4 * r0, self.ptrs[1] + 4 * r0

    def free(self):
        for d in self.d:
            d.free()


def motions(seed, n_a, n_b, scale=4.0):
    """-> (ma, mb), each (dx, dy) f32[n] of up to +-scale per component"""
    rng = np.random.default_rng(seed)
    return tuple(tuple((rng.uniform(-1, 1, n) * scale).astype(np.float32) for _ in range(2)) for n in (n_a, n_b))


class Extras:
    """What the two sets of one call carry besides their vertices, on the device, from its host form x = Query.extras(...): nothing
    for most queries, each set's motion for the sweeps (None: that set stands still).  .kw: the keywords of poly_call / rect_call;
    .raw: the same pointers as the C call takes them behind the two sets."""

    def __init__(self, eng, x, apart=False):
        self.d = [None if m is None else Motion(eng, m, apart=apart) for m in x]
        self.kw = {name: d.ptrs for name, d in zip(("a_motion", "b_motion"), self.d) if d is not None}
        self.raw = [p for d in self.d for p in (d.ptrs if d is not None else (None, None))]

    def free(self):
        for d in self.d:
            if d is not None:
                d.free()


def local(pairs):
    return pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)


def diag(n):
    return np.stack([np.arange(n), np.arange(n)], axis=1).astype(np.uint32)


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


def oracle_hits(oracle, a, b, pairs):
    i, j = local(pairs)
    return oracle.sat_poly_pairs(np.stack([a[0][:, i], b[0][:, j]]), np.stack([a[1][:, i], b[1][:, j]]), np.stack([a[2][i], b[2][j]]))[0]


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


def synchronize(eng, expect_error=False):
    """the synchronise behind the call(s) under test; under expect_error it reports status -1, once"""
    if expect_error:
        with pytest.raises(Exception) as e:
            eng.synchronize()
        assert getattr(e.value, "status", None) == -1
        eng.synchronize()
        eng.check_async()      # reported once, then clear
    else:
        eng.synchronize()


def banded_call(eng, dt, n, launch, capacity=None, expect_error=False, band=None):
    """launch(ptr) queues a call that writes n records of dt at ptr, the start of `capacity` records (default n) between two guard
    bands -> dt[capacity]: the bands and every record at or beyond n must be untouched (unband); under expect_error the next
    synchronise reports status -1, once.  band: a buffer of banded(eng, capacity, dt) to use again (many small calls: it is filled
    with the band's byte first and stays the caller's)."""
    cap = n if capacity is None else capacity
    d = banded(eng, cap, dt) if band is None else band
    try:
        if band is not None:
            assert d.nbytes == (cap + 2 * GUARD) * dt.itemsize
            eng.memset(d, BAND, d.nbytes)
        launch(d.ptr + dt.itemsize * GUARD)
        synchronize(eng, expect_error)
        return unband(d, cap, n, dt)
    finally:
        if band is None:
            d.free()


def run(eng, queue, pairs, dts, capacity=None, n_dev=None, expect_error=False):
    """queue(d_pairs, capacity, out_ptrs, d_n) queues the call(s) under test; out_ptrs[q] is where output q (dts[q][capacity]) begins,
    between two guard bands.  -> [dts[q][capacity]]: the bands must be intact and every record at or beyond min(capacity, n_dev)
    untouched (unband); under expect_error the next synchronise reports status -1, once."""
    cap = len(pairs) if capacity is None else capacity
    host_pairs = np.full((max(cap, 1), 2), 0xFFFFFFFF, np.uint32)   # entries beyond the list: indices no set has
    host_pairs[:len(pairs)] = pairs
    d_pairs = eng.to_device(host_pairs)
    d_outs = [banded(eng, cap, dt) for dt in dts]
    d_n = None if n_dev is None else eng.to_device(np.array([n_dev], np.uint64))
    try:
        queue(d_pairs, cap, [d.ptr + dt.itemsize * GUARD for d, dt in zip(d_outs, dts)], d_n)
        synchronize(eng, expect_error)
        bound = cap if n_dev is None else min(cap, n_dev)
        return [unband(d, cap, bound, dt) for d, dt in zip(d_outs, dts)]
    finally:
        for x in [d_pairs, d_n] + d_outs:
            if x is not None:
                x.free()


def outputs(records):
    """the records of one call as a tuple, one element per output (a query with one output hands its records around bare)"""
    return records if isinstance(records, tuple) else (records,)


def hit_or_miss(want):
    return want["hit"] == 1, want["hit"] == 0


def sweep_classes(want):
    """start overlap, moving hit, miss"""
    start = (want["flags"] & sweep_ref.START_OVERLAP) != 0
    return start, (want["hit"] == 1) & ~start, want["hit"] == 0


class Query:
    """What one list-driven query states of its own.  dts / sames / nouns: per output, the record, its comparison and its word in a
    message; poly / rect: the Engine method of the polygon / rectangle call (the C symbol is "c2d_" + that), taking the outputs in
    order behind n_pairs; poly_ref / rect_ref(a, b, i, j, *x): the numpy reference on local indices; bad_pair: the flag a refused
    entry carries in the first output; every / count_cut: which of the dense sets' pairs dense() takes, and which 300 of those
    test_device_count_bounds_the_work lists; with_contacts: every polygon run() also queues c2d_poly_pair_contacts on the same
    arguments and compares it, byte for byte, with the first output; extras(seed, n_a, n_b, scale) -> x: what the two sets carry
    besides their vertices, as the reference takes it (Extras uploads it for the call); classes(first output) -> the kinds of record a
    list has to mix, and mix = (dense, graph): the share of each that dense() and the graph check ask for at least."""

    def __init__(self, name, dts, sames, nouns, bad_pair, poly, poly_ref, rect=None, rect_ref=None, every=1, count_cut=slice(5, None, 311), with_contacts=False,
                 extras=lambda *a, **kw: (), classes=hit_or_miss, mix=((0.1, 0.5), (0.1, 0.1))):
        self.name, self.dts, self.sames, self.nouns, self.bad_pair = name, dts, sames, nouns, bad_pair
        self.poly, self.poly_ref, self.rect, self.rect_ref = poly, poly_ref, rect, rect_ref
        self.every, self.count_cut, self.with_contacts = every, count_cut, with_contacts
        self.extras, self.classes, self.mix = extras, classes, mix

    def mixed(self, want, where):
        """whether the records `want` of a list mix this query's classes as `where` (0: dense(), 1: the graph check) asks"""
        return all(c.mean() > least for c, least in zip(self.classes(outputs(want)[0]), self.mix[where]))

    def __repr__(self):
        return self.name

    def poly_call(self, eng, a, b, **bases):
        """a, b: c2d_poly_set; bases: row_base, col_base and Extras.kw -> the queue of run(); .dts: the outputs it wants banded"""
        def queue(d_pairs, cap, outs, d_n):
            getattr(eng, self.poly)(a, b, d_pairs, cap, *outs[:len(self.dts)], n_pairs_dev=d_n, **bases)
            if self.with_contacts:
                eng.poly_pair_contacts(a, b, d_pairs, cap, outs[-1], n_pairs_dev=d_n, **bases)
        queue.dts = self.dts + ((contact_ref.CONTACT_DT,) if self.with_contacts else ())
        return queue

    def rect_call(self, eng, a, b, **bases):
        """a, b: RectsOnDevice"""
        return lambda d_pairs, cap, outs, d_n: getattr(eng, self.rect)(a.ptrs, a.n, b.ptrs, b.n, d_pairs, cap, *outs, n_pairs_dev=d_n, **bases)

    def run(self, eng, queue, pairs, **kw):
        """run() with the outputs of this query's call -> its records (a tuple where the query has two outputs)"""
        got = run(eng, queue, pairs, getattr(queue, "dts", self.dts), **kw)
        if len(got) > len(self.dts):
            assert got[0].tobytes() == got.pop().tobytes(), "the contact output differs from c2d_poly_pair_contacts'"
        return got[0] if len(got) == 1 else tuple(got)

    def cut(self, records, sel):
        """records[sel] of every output"""
        got = tuple(r[sel] for r in outputs(records))
        return got[0] if len(got) == 1 else got

    def assert_same(self, got, want, what):
        for g, w, same, noun in zip(outputs(got), outputs(want), self.sames, self.nouns):
            ok = same(g, w)
            if not ok.all():
                q = int(np.flatnonzero(~ok)[0])
                raise AssertionError(f"{what}: {int((~ok).sum())} of {len(w)} {noun} differ; first at {q}: got {g[q]}, want {w[q]}")
            assert "reserved" not in g.dtype.names or (g["reserved"] == 0).all()


CONTACTS = Query("contacts", (contact_ref.CONTACT_DT,), (contact_ref.same,), ("contacts",), contact_ref.BAD_PAIR, "poly_pair_contacts",
                 contact_ref.poly_contacts, "rect_pair_contacts", contact_ref.rect_contacts)
MANIFOLDS = Query("manifolds", (contact_ref.CONTACT_DT, manifold_ref.MANIFOLD_DT), (contact_ref.same, manifold_ref.same), ("contacts", "manifolds"),
                  contact_ref.BAD_PAIR, "poly_pair_manifolds", manifold_ref.poly_manifolds, every=17, count_cut=slice(None), with_contacts=True)
DISTANCES = Query("distances", (distance_ref.DISTANCE_DT,), (distance_ref.same,), ("records",), distance_ref.BAD_PAIR, "poly_pair_distances",
                  distance_ref.poly_distances, "rect_pair_distances", distance_ref.rect_distances)
SWEEPS = Query("sweeps", (sweep_ref.SWEEP_DT,), (sweep_ref.same,), ("records",), sweep_ref.BAD_PAIR, "poly_pair_sweeps", sweep_ref.poly_sweeps,
               "rect_pair_sweeps", sweep_ref.rect_sweeps, extras=motions, classes=sweep_classes, mix=((0.1, 0.05, 0.3), (0.1, 0.05, 0.05)))
QUERIES = (CONTACTS, MANIFOLDS, DISTANCES, SWEEPS)


# ---- shared inputs, computed once per process ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense(wl, query):
    """The dense sets (300 x 311 polygons in a small box) and every `query.every`-th of their pairs, in every class of the query, with
    the query's reference of those pairs (read-only), the sets carrying dense_extras(query) -> a, b, pairs, want"""
    a, b = contact_cases.dense_poly_sets(wl)
    pairs = contact_cases.all_pairs(a[0].shape[1], b[0].shape[1])[::query.every]
    want = query.poly_ref(a, b, *local(pairs), *dense_extras(query))
    for w in outputs(want):
        w.setflags(write=False)
    assert len(pairs) >= 4099 and query.mixed(want, 0), [c.mean() for c in query.classes(outputs(want)[0])]
    return a, b, pairs, want


@functools.lru_cache(maxsize=None)
def dense_extras(query):
    """the sweeps: both dense sets move by up to +-4 per component"""
    return query.extras(9101, 300, 311)


@functools.lru_cache(maxsize=None)
def hard_batches(wl):
    return contact_cases.hard_poly_batches(wl)
