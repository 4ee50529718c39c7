"""What the GPU tests of the shape casts share (test_gpu_casts.py, tools/cast_fuzz.py), after clearance_harness.py: the frame's
call between guard bands and its comparison (tests/best_key_harness.py) bound to c2d_poly_set_casts, and the reference of a scene whose
polygons repeat (computed on the distinct polygons and indexed).  The per-pair records of the constructions of cast_cases.py are computed once per process here, for
test_cast_cases_cpu.py and the GPU tests alike.  A plain module on numpy and the numpy references: it never loads libc2d.so."""
import functools

import numpy as np

import best_key_harness as best
import cast_cases as cases
import cast_ref as ref
import clearance_cases
import pair_list_harness as h
from clearance_harness import take  # noqa: F401  (the set of polygons s[idx[0]], s[idx[1]], ...)

DT = ref.CAST_DT


call = functools.partial(best.call, best.CASTS)                # call(eng, a_set, b_set, n_a, a_motion=None, b_motion=None, capacity=None, expect_error=False, band=None, **kw)
twice = functools.partial(best.twice, best.CASTS)              # twice(eng, a_set, b_set, n_a, what, **kw): the call, run twice: the same bytes
assert_same = functools.partial(best.assert_same, best.CASTS)  # assert_same(got, want, what)


def take_motion(m, idx):
    return None if m is None else (np.ascontiguousarray(m[0][idx]), np.ascontiguousarray(m[1][idx]))


def indexed_reference(a, ia, b, ib, ma=None, mb=None, S=None, **kw):
    """the reference of (take(a, ia), take(b, ib)) with the motions indexed alike: the per-pair records are computed for the distinct
    polygons once (or handed in as S) and indexed.  Beyond 2^22 pairs the pick is made once per DISTINCT query and indexed by ia
    (best_key_harness.reduce_by_query)."""
    ia, ib = np.asarray(ia, np.int64), np.asarray(ib, np.int64)
    if len(ia) == 0:
        return np.zeros(0, DT)
    if S is None:
        S = ref.pair_records(a, b, ma, mb) if b[0].shape[1] else np.zeros((a[0].shape[1], 0), ref.sref.SWEEP_DT)
    bad_a, bad_b = ref.bad_counts(a), ref.bad_counts(b)[ib]
    if len(ia) * len(ib) <= 1 << 22:
        return ref.reduce(S[np.ix_(ia, ib)], bad_a[ia], bad_b, **kw)
    return best.reduce_by_query(ref, S, ia, ib, bad_a, bad_b, **kw)


class Scene:
    """two sets with their motions on the device: .a, .b (pair_list_harness.Uploaded), .ma, .mb (Motion or None)"""

    def __init__(self, eng, a, b, ma=None, mb=None, place_a=(0, 0), place_b=(0, 0), with_k=True, same=False):
        n_a, n_b = a[0].shape[1], b[0].shape[1]
        self.a = h.Uploaded(eng, a, offset=place_a[0], stride=n_a + place_a[1], with_k=with_k)
        self.ma = None if ma is None else h.Motion(eng, ma, offset=place_a[0])
        self.same = same
        if same:
            self.b, self.mb = self.a, self.ma
        else:
            self.b = h.Uploaded(eng, b, offset=place_b[0], stride=n_b + place_b[1], with_k=with_k) if n_b else None
            self.mb = None if (mb is None or not n_b) else h.Motion(eng, mb, offset=place_b[0])
        self.b_set = self.b.set if self.b is not None else eng.poly_set(None, None, None, 0, b[0].shape[0])

    def motions(self, r0=0, c0=0):
        return dict(a_motion=None if self.ma is None else self.ma.sub(r0), b_motion=None if self.mb is None else self.mb.sub(c0))

    def free(self):
        for x in (self.a, self.ma) + (() if self.same else (self.b, self.mb)):
            if x is not None:
                x.free()


@functools.lru_cache(maxsize=None)
def witness_records(wl, name):
    """-> S [n_a][n_b], SW [n_a][1], (ma, mb, mw): the per-pair sweep records of batch `name` of clearance_cases.witness_batches with
    motions of twice the batch's scale, and of its queries against the witness, which stands still (read-only)"""
    a, b, w, _ = clearance_cases.witness_batches(wl)[name]
    ma, mb = witness_motions(a, b, name)
    S, SW = ref.pair_records(a, b, ma, mb), ref.pair_records(a, w, ma, None)
    S.setflags(write=False)
    SW.setflags(write=False)
    return S, SW, (ma, mb)


def witness_motions(a, b, name):
    """motions of up to twice the batch's scale (the median finite |coordinate|), drawn from the batch's name"""
    c = np.abs(np.concatenate([x.ravel() for x in (a[0], a[1], b[0], b[1])]).astype(np.float64))
    c = c[np.isfinite(c) & (c > 0)]
    scale = float(np.median(c)) if c.size else 1.0
    rng = np.random.default_rng([9701] + [ord(ch) for ch in name])
    with np.errstate(over="ignore"):
        return tuple(tuple((rng.uniform(-2, 2, s[0].shape[1]) * scale).astype(np.float32) for _ in range(2)) for s in (a, b))


def witness_reference(wl, name, layout, j):
    """the reference of batch `name`'s queries against the shard of obstacle j in `layout`, col_base being the shard's offset"""
    a, b, w, layouts = clearance_cases.witness_batches(wl)[name]
    S, SW, _ = witness_records(wl, name)
    width = layouts[layout][1]
    records = np.concatenate([np.repeat(S[:, j:j + 1], width - 1, axis=1), SW], axis=1)
    bad_b = np.concatenate([np.repeat(ref.bad_counts(b)[j:j + 1], width - 1), ref.bad_counts(w)])
    return ref.reduce(records, ref.bad_counts(a), bad_b, col_base=width * j)


@functools.lru_cache(maxsize=None)
def near_tie_records(theta, offset):
    """-> a, b, ma, S: cases.moving_near_ties(theta, offset) and its per-pair records [64][130] (read-only)"""
    a, b, ma = cases.moving_near_ties(theta, offset)
    S = ref.pair_records(a, b, ma, None)
    S.setflags(write=False)
    return a, b, ma, S


@functools.lru_cache(maxsize=None)
def graze_records():
    """-> a, b, ma, mb, graze, miss, S: cases.grazes() and its per-pair records (read-only)"""
    a, b, ma, mb, graze, miss = cases.grazes()
    S = ref.pair_records(a, b, ma, mb)
    S.setflags(write=False)
    return a, b, ma, mb, graze, miss, S
