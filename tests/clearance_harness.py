"""What the GPU tests of the clearance query share (test_gpu_clearances.py, tools/clearance_fuzz.py): the frame's call between guard
bands and its comparison (tests/best_key_harness.py) bound to c2d_poly_set_clearances, and the reference of a scene whose polygons
repeat (computed on the distinct polygons and indexed).
The per-pair records of the constructions of clearance_cases.py (witness_batches, slid_near_ties) are computed once per process here, for
test_clearance_cases_cpu.py and the GPU tests alike.  A plain module on numpy and the numpy references: it never loads libc2d.so."""
import functools

import numpy as np

import best_key_harness as best
import clearance_cases as cases
import clearance_ref as ref

DT = ref.CLEARANCE_DT


call = functools.partial(best.call, best.CLEARANCES)                # call(eng, a_set, b_set, n_a, capacity=None, expect_error=False, band=None, **kw) -> DT[n_a]
twice = functools.partial(best.twice, best.CLEARANCES)              # twice(eng, a_set, b_set, n_a, what, **kw): the call, run twice: the same bytes
assert_same = functools.partial(best.assert_same, best.CLEARANCES)  # assert_same(got, want, what)


def take(s, idx):
    """the set of polygons s[idx[0]], s[idx[1]], ..."""
    idx = np.asarray(idx, np.int64)
    return np.ascontiguousarray(s[0][:, idx]), np.ascontiguousarray(s[1][:, idx]), None if s[2] is None else np.ascontiguousarray(s[2][idx])


def indexed_reference(a, ia, b, ib, D=None, by_query=None, **kw):
    """the reference of (take(a, ia), take(b, ib)): the per-pair records are computed for the distinct polygons once (or handed in
    as D) and indexed.  by_query (the default beyond 2^22 pairs): the pick is made once per DISTINCT query against take(b, ib) and
    indexed by ia (best_key_harness.reduce_by_query)."""
    ia, ib = np.asarray(ia, np.int64), np.asarray(ib, np.int64)
    if len(ia) == 0:
        return np.zeros(0, DT)
    if D is None:
        D = ref.pair_records(a, b) if b[0].shape[1] else np.zeros((a[0].shape[1], 0), ref.dref.DISTANCE_DT)
    bad_a, bad_b = ref.bad_counts(a), ref.bad_counts(b)[ib]
    if by_query is None:
        by_query = len(ia) * len(ib) > 1 << 22
    if not by_query:
        return ref.reduce(D[np.ix_(ia, ib)], bad_a[ia], bad_b, **kw)
    return best.reduce_by_query(ref, D, ia, ib, bad_a, bad_b, **kw)


@functools.lru_cache(maxsize=None)
def witness_records(wl, name):
    """-> D [n_a][n_b], DW [n_a][1]: the per-pair records of batch `name` of cases.witness_batches and of its queries against the
    witness (read-only)"""
    a, b, w, _ = cases.witness_batches(wl)[name]
    D, DW = ref.pair_records(a, b), ref.pair_records(a, w)
    D.setflags(write=False)
    DW.setflags(write=False)
    return D, DW


def witness_reference(wl, name, layout, j):
    """the reference of batch `name`'s queries against the shard of obstacle j in `layout`, col_base being the shard's offset"""
    a, b, w, layouts = cases.witness_batches(wl)[name]
    D, DW = witness_records(wl, name)
    width = layouts[layout][1]
    records = np.concatenate([np.repeat(D[:, j:j + 1], width - 1, axis=1), DW], axis=1)
    bad_b = np.concatenate([np.repeat(ref.bad_counts(b)[j:j + 1], width - 1), ref.bad_counts(w)])
    return ref.reduce(records, ref.bad_counts(a), bad_b, col_base=width * j)


@functools.lru_cache(maxsize=None)
def near_tie_records(theta, offset):
    """-> a, b, D: cases.slid_near_ties(theta, offset) and its per-pair records [64][130] (read-only)"""
    a, b = cases.slid_near_ties(theta, offset)
    D = ref.pair_records(a, b)
    D.setflags(write=False)
    return a, b, D
