"""What the GPU tests of the clearance query share (test_gpu_clearances.py, tools/clearance_fuzz.py): the call between guard bands, the
reference of a scene whose polygons repeat (computed on the distinct polygons and indexed), and the comparison with its message.
A plain module on numpy and the numpy references: it never loads libc2d.so."""
import numpy as np
import pytest

import clearance_ref as ref
import pair_list_harness as h

DT = ref.CLEARANCE_DT


def call(eng, a_set, b_set, n_a, capacity=None, expect_error=False, **kw):
    """c2d_poly_set_clearances into a buffer between guard bands -> the n_a records; the bands and every record at or beyond n_a
    must be untouched; under expect_error the next synchronise reports status -1, once"""
    cap = max(n_a, 4) if capacity is None else capacity
    d = h.banded(eng, cap, DT)
    try:
        eng.poly_set_clearances(a_set, b_set, d.ptr + DT.itemsize * h.GUARD, **kw)
        if expect_error:
            with pytest.raises(Exception) as e:
                eng.synchronize()
            assert getattr(e.value, "status", None) == -1
            eng.synchronize()
            eng.check_async()      # reported once, then clear
        else:
            eng.synchronize()
        return h.unband(d, cap, n_a, DT)[:n_a].copy()
    finally:
        d.free()


def twice(eng, a_set, b_set, n_a, what, **kw):
    """the call, run twice: the two outputs must be the same bytes"""
    got, again = call(eng, a_set, b_set, n_a, **kw), call(eng, a_set, b_set, n_a, **kw)
    assert got.tobytes() == again.tobytes(), f"{what}: two runs differ"
    return got


def take(s, idx):
    """the set of polygons s[idx[0]], s[idx[1]], ..."""
    idx = np.asarray(idx, np.int64)
    return np.ascontiguousarray(s[0][:, idx]), np.ascontiguousarray(s[1][:, idx]), None if s[2] is None else np.ascontiguousarray(s[2][idx])


def indexed_reference(a, ia, b, ib, **kw):
    """the reference of (take(a, ia), take(b, ib)): the per-pair records are computed for the distinct polygons once and indexed"""
    ia, ib = np.asarray(ia, np.int64), np.asarray(ib, np.int64)
    if len(ia) == 0:
        return np.zeros(0, DT)
    D = ref.pair_records(a, b) if b[0].shape[1] else np.zeros((a[0].shape[1], 0), ref.dref.DISTANCE_DT)
    return ref.reduce(D[np.ix_(ia, ib)], ref.bad_counts(a)[ia], ref.bad_counts(b)[ib], **kw)


def assert_same(got, want, what):
    ok = ref.same(got, want)
    if not ok.all():
        q = int(np.flatnonzero(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {len(want)} records differ; first at {q}: got {got[q]}, want {want[q]}")
