"""CPU test of tests/pair_list_harness.py itself: run(), banded() and unband() carry the guard-band coverage of all four list-driven
queries, and banded_call() that of the N x M reductions, their grid forms and the ray queries, so a silent mistake there would remove
it everywhere at once.  The stand-in engine's device arrays are numpy buffers, the stand-in query a Python function that writes
records through the pointers it is handed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_list_harness as h  # noqa: E402


class Status(Exception):
    status = -1


class HostArray:
    def __init__(self, eng, a):
        self.a, self.ptr, self.nbytes = a, a.ctypes.data, a.nbytes
        eng.live.append(self)

    def get(self):
        return self.a.copy()

    def free(self):
        self.freed = True


class HostEngine:
    """reports: how many of the following synchronise / check_async calls raise status -1 (a real engine: one after a bad entry)"""

    def __init__(self, reports=0):
        self.reports, self.live = reports, []

    def empty(self, shape, dtype):
        return HostArray(self, np.zeros(shape, dtype))

    def to_device(self, host):
        return HostArray(self, np.array(host))

    def memset(self, d, value, nbytes):
        d.a.view(np.uint8).reshape(-1)[:nbytes] = value

    def synchronize(self):
        if self.reports:
            self.reports -= 1
            raise Status()

    check_async = synchronize


def bytes_at(ptr, n):
    return np.frombuffer((C.c_ubyte * n).from_address(ptr), np.uint8)


def record(p, q, size):
    return (np.arange(size) + 7 * p + q) % 251


def writer(dts, stray=None):
    """the stand-in query: record p of output q = record(p, q, size) for p < min(capacity, *d_n); stray = (output, byte offset from
    the output's begin): one more byte written there"""
    def queue(d_pairs, cap, outs, d_n):
        assert d_pairs.a.shape == (max(cap, 1), 2) and d_pairs.a.dtype == np.uint32
        n = cap if d_n is None else min(cap, int(d_n.a[0]))
        for q, (ptr, dt) in enumerate(zip(outs, dts)):
            for p in range(n):
                bytes_at(ptr + p * dt.itemsize, dt.itemsize)[:] = record(p, q, dt.itemsize)
        if stray:
            bytes_at(outs[stray[0]] + stray[1], 1)[:] = 0
    return queue


@pytest.mark.parametrize("q", h.QUERIES, ids=repr)
def test_the_table_has_the_bindings_records(pkg, q):
    assert [dt.itemsize for dt in q.dts] == {"contacts": [16], "manifolds": [16, 32], "distances": [32], "sweeps": [16]}[q.name]
    assert q.dts == {"contacts": (pkg.CONTACT_DT,), "manifolds": (pkg.CONTACT_DT, pkg.MANIFOLD_DT), "distances": (pkg.DISTANCE_DT,),
                     "sweeps": (pkg.SWEEP_DT,)}[q.name]
    assert pkg.CONTACT_DT.itemsize == 16 and pkg.MANIFOLD_DT.itemsize == 32 and pkg.DISTANCE_DT.itemsize == 32 and pkg.SWEEP_DT.itemsize == 16


@pytest.mark.parametrize("q", h.QUERIES, ids=repr)
@pytest.mark.parametrize("cap, n_dev", [(9, None), (9, 4), (9, 0), (9, 9), (9, 1 << 40), (0, None)])
def test_a_correct_writer_returns_the_records_between_the_bands(q, cap, n_dev):
    eng = HostEngine()
    pairs = np.arange(2 * min(cap, 5), dtype=np.uint32).reshape(-1, 2)
    got = h.run(eng, writer(q.dts), pairs, q.dts, capacity=cap, n_dev=n_dev)
    bound = cap if n_dev is None else min(cap, n_dev)
    assert len(got) == len(q.dts)
    for k, (g, dt) in enumerate(zip(got, q.dts)):
        assert g.dtype == dt and g.shape == (cap,)
        raw = g.view(np.uint8).reshape(cap, dt.itemsize)
        assert all((raw[p] == record(p, k, dt.itemsize)).all() for p in range(bound)) and (raw[bound:] == h.BAND).all()
    assert len(eng.live) == 1 + len(q.dts) + (n_dev is not None) and all(getattr(x, "freed", False) for x in eng.live)
    assert (eng.live[0].a[len(pairs):] == 0xFFFFFFFF).all() and np.array_equal(eng.live[0].a[:len(pairs)], pairs)


@pytest.mark.parametrize("q", h.QUERIES, ids=repr)
def test_one_stray_byte_raises_the_matching_assertion(q):
    cap, n_dev = 9, 4
    for k, dt in enumerate(q.dts):
        for where, message in ((-1, "written outside the output"), (-dt.itemsize * h.GUARD, "written outside the output"),
                               (cap * dt.itemsize, "written outside the output"), ((cap + h.GUARD) * dt.itemsize - 1, "written outside the output"),
                               (n_dev * dt.itemsize, "written at or beyond min(n_pairs, *d_n_pairs)"),
                               (cap * dt.itemsize - 1, "written at or beyond min(n_pairs, *d_n_pairs)")):
            with pytest.raises(AssertionError) as e:
                h.run(HostEngine(), writer(q.dts, stray=(k, where)), np.zeros((cap, 2), np.uint32), q.dts, n_dev=n_dev)
            assert str(e.value).startswith(message), (k, where, str(e.value))
    h.run(HostEngine(), writer(q.dts, stray=(0, 0)), np.zeros((cap, 2), np.uint32), q.dts, n_dev=n_dev)        # (a byte inside the bound is none)


def test_banded_and_unband():
    eng, dt = HostEngine(), h.DISTANCES.dts[0]
    d = h.banded(eng, 5, dt)
    assert d.a.shape == (5 + 2 * h.GUARD,) and (d.a.view(np.uint8) == h.BAND).all()
    assert h.unband(d, 5, 0, dt).shape == (5,)
    d.a.view(np.uint8)[dt.itemsize * (h.GUARD + 2)] ^= 1
    assert h.unband(d, 5, 3, dt).shape == (5,)
    with pytest.raises(AssertionError, match="at or beyond"):
        h.unband(d, 5, 2, dt)


def test_expect_error_wants_one_report():
    dts, pairs = h.CONTACTS.dts, np.zeros((3, 2), np.uint32)
    assert len(h.run(HostEngine(reports=1), writer(dts), pairs, dts, expect_error=True)[0]) == 3
    with pytest.raises(pytest.fail.Exception, match="DID NOT RAISE"):            # a stand-in that reports nothing
        h.run(HostEngine(reports=0), writer(dts), pairs, dts, expect_error=True)
    for reports in (2, 3):                                                       # one that goes on reporting
        with pytest.raises(Status):
            h.run(HostEngine(reports=reports), writer(dts), pairs, dts, expect_error=True)
    with pytest.raises(Status):                                                  # and without expect_error a report is an error
        h.run(HostEngine(reports=1), writer(dts), pairs, dts)


def test_banded_call_asserts_what_the_per_query_calls_asserted():
    """banded_call carries the guard bands of the N x M reductions and the ray queries (the call / cast wrappers of clearance_harness,
    cast_harness, clearance_grid_harness, cast_grid_harness and ray_harness): a stand-in kernel that writes (a) exactly n records
    passes, (b) one byte into the lower band, (c) one record beyond n raise."""
    dt, n, cap = h.DISTANCES.dts[0], 5, 8

    def kernel(records, stray=None):
        def launch(ptr):
            for p in range(records):
                bytes_at(ptr + p * dt.itemsize, dt.itemsize)[:] = record(p, 0, dt.itemsize)
            if stray is not None:
                bytes_at(ptr + stray, 1)[:] = 0
        return launch

    eng = HostEngine()
    got = h.banded_call(eng, dt, n, kernel(n), capacity=cap)                     # (a)
    raw = got.view(np.uint8).reshape(cap, dt.itemsize)
    assert got.dtype == dt and got.shape == (cap,) and (raw[n:] == h.BAND).all()
    assert all((raw[p] == record(p, 0, dt.itemsize)).all() for p in range(n))
    assert len(eng.live) == 1 and eng.live[0].freed
    assert h.banded_call(HostEngine(), dt, n, kernel(n)).shape == (n,)           # capacity defaults to n
    with pytest.raises(AssertionError, match="written outside the output"):      # (b)
        h.banded_call(HostEngine(), dt, n, kernel(n, stray=-1), capacity=cap)
    with pytest.raises(AssertionError, match="written at or beyond"):            # (c)
        h.banded_call(HostEngine(), dt, n, kernel(n + 1), capacity=cap)
    with pytest.raises(AssertionError, match="written outside the output"):      # (c) with no room behind n: the upper band
        h.banded_call(HostEngine(), dt, n, kernel(n + 1))

    # a band of the caller's: refilled before the call, checked for its size, and left to the caller
    eng = HostEngine()
    band = h.banded(eng, cap, dt)
    band.a.view(np.uint8)[:] = 0
    assert (h.banded_call(eng, dt, n, kernel(n), capacity=cap, band=band).view(np.uint8).reshape(cap, -1)[n:] == h.BAND).all()
    assert not getattr(band, "freed", False)
    with pytest.raises(AssertionError):
        h.banded_call(eng, dt, n, kernel(n), capacity=cap + 1, band=band)

    # expect_error: status -1, once, then clear
    assert len(h.banded_call(HostEngine(reports=1), dt, n, kernel(n), expect_error=True)) == n
    with pytest.raises(pytest.fail.Exception, match="DID NOT RAISE"):
        h.banded_call(HostEngine(reports=0), dt, n, kernel(n), expect_error=True)
    with pytest.raises(Status):
        h.banded_call(HostEngine(reports=2), dt, n, kernel(n), expect_error=True)
    with pytest.raises(Status):
        h.banded_call(HostEngine(reports=1), dt, n, kernel(n))


def test_the_manifolds_entry_compares_its_contacts_with_the_contacts_call():
    q = h.MANIFOLDS

    class Both(HostEngine):
        stray = None

        def poly_pair_manifolds(self, a, b, d_pairs, cap, contacts, manifolds, n_pairs_dev=None):
            writer(q.dts)(d_pairs, cap, [contacts, manifolds], n_pairs_dev)

        def poly_pair_contacts(self, a, b, d_pairs, cap, contacts, n_pairs_dev=None):
            writer(q.dts[:1], stray=self.stray)(d_pairs, cap, [contacts], n_pairs_dev)

    eng, pairs = Both(), np.zeros((6, 2), np.uint32)
    got = q.run(eng, q.poly_call(eng, None, None), pairs)
    assert isinstance(got, tuple) and [g.dtype for g in got] == list(q.dts) and len(eng.live) == 4
    eng.stray = (0, 16 * 5 + 3)
    with pytest.raises(AssertionError, match="the contact output differs from c2d_poly_pair_contacts'"):
        q.run(eng, q.poly_call(eng, None, None), pairs)
