"""What the harnesses of the best-key queries share (clearance_harness.py, cast_harness.py, the ray tests): the call run twice, the
comparison with its message, and the reference of a scene whose polygons repeat, made once per distinct query.  Each takes the
query's own `call` or numpy reference module `ref` first; the harnesses bind it (functools.partial).  A plain module on numpy."""
import numpy as np


def twice(call, eng, x, y, z, what, **kw):
    """call(eng, x, y, z, **kw), run twice: the two outputs must be the same bytes"""
    got, again = call(eng, x, y, z, **kw), call(eng, x, y, z, **kw)
    assert got.tobytes() == again.tobytes(), f"{what}: two runs differ"
    return got


def assert_same(ref, got, want, what):
    ok = ref.same(got, want)
    if not ok.all():
        q = int(np.flatnonzero(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {len(want)} records differ; first at {q}: got {got[q]}, want {want[q]}")


def reduce_by_query(ref, R, ia, ib, bad_a, bad_b, **kw):
    """the reference of the queries ia against the polygons ib from R, the per-pair records of the DISTINCT polygons [n_a][n_b]
    (bad_a of the distinct queries, bad_b of ib): the pick is made once per distinct query against R[:, ib] and indexed by ia, so
    that the cost does not grow with len(ia); the self pair of SKIP_SELF depends on the query's own place, and matters only where it
    is the winner: those queries are reduced one by one."""
    rb, cb, flags = kw.get("row_base", 0), kw.get("col_base", 0), kw.get("flags", 0)
    Rb = R[:, ib]
    out = ref.reduce(Rb, bad_a, bad_b, col_base=cb)[ia]
    if flags & ref.SKIP_SELF:
        j_self = rb + np.arange(len(ia), dtype=np.int64) - cb
        own = (j_self >= 0) & (j_self < len(ib)) & (out["poly"].astype(np.int64) == cb + j_self)
        for q in np.flatnonzero(own):
            out[q] = ref.reduce(Rb[ia[q]:ia[q] + 1], bad_a[ia[q]:ia[q] + 1], bad_b, row_base=rb + int(q), col_base=cb, flags=flags)[0]
    return out
