"""CPU restatement of the shape-cast contract of include/c2d.h (c2d_poly_set_casts), written from the contract: the reduction over
tests/sweep_ref.py's poly_sweeps and nothing else.  For query i, S(i, j) is the sweep record of the pair (A_i, B_j) with the call's
motions; polygon j is considered when its vertex count is within 1..rows and it is not the self pair (under SKIP_SELF the pair with
row_base + i == col_base + j); among the considered j with S(i, j).hit == 1 the winner is the one with the smallest key
(bits of S(i, j).toi, col_base + j).

casts(a, b, a_motion, b_motion, ...) -> CAST_DT[n_a].  pair_records(a, b, a_motion, b_motion) -> the S(i, j) of all pairs
[n_a][n_b], for callers that want the same scene reduced more than once (reduce())."""
import numpy as np

import sweep_ref as sref

CAST_DT = np.dtype([("poly", "<u4"), ("toi", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("axis", "<u2"), ("hit", "u1"), ("flags", "u1"), ("reserved0", "<u4")])
SKIP_SELF = 1
NO_POLY, NONE16 = 0xFFFFFFFF, 0xFFFF
FLOATS = sref.FLOATS
COPIED = FLOATS + ("axis", "hit", "flags")


def bad_counts(s):
    """per polygon: its vertex count is outside 1..rows"""
    k = sref._counts(s)
    return (k < 1) | (k > s[0].shape[0])


def pair_records(a, b, a_motion=None, b_motion=None):
    """S(i, j) of every pair -> SWEEP_DT[n_a][n_b] (BAD_PAIR entries where either count is out of range)"""
    n_a, n_b = a[0].shape[1], b[0].shape[1]
    i, j = np.repeat(np.arange(n_a), n_b), np.tile(np.arange(n_b), n_a)
    return sref.poly_sweeps(a, b, i, j, a_motion, b_motion).reshape(n_a, n_b)


def reduce(S, bad_a, bad_b, row_base=0, col_base=0, flags=0):
    """the pick and the two special records, from the per-pair records S [n_a][n_b]"""
    n_a, n_b = S.shape
    out = np.zeros(n_a, CAST_DT)
    considered = np.broadcast_to(~bad_b[None, :], (n_a, n_b)).copy()
    if flags & SKIP_SELF:
        considered &= (row_base + np.arange(n_a))[:, None] != (col_base + np.arange(n_b))[None, :]
    candidate = considered & (S["hit"] == 1)
    toi = np.ascontiguousarray(S["toi"])
    assert not (candidate & (np.isnan(toi) | (np.signbit(toi) & (toi == 0)) | (toi > 1))).any()   # a hit's toi: never NaN, never -0, at most 1
    bits = toi.view(np.uint32).astype(np.uint64)
    key = (bits << np.uint64(32)) | (np.uint64(col_base) + np.arange(n_b, dtype=np.uint64))[None, :]
    key = np.where(candidate, key, np.uint64(0xFFFFFFFFFFFFFFFF))
    any_hit = candidate.any(axis=1) if n_b else np.zeros(n_a, bool)
    win = key.argmin(axis=1) if n_b else np.zeros(n_a, np.int64)   # (argmin: the first of equal keys; keys differ in j anyway)
    rows = np.arange(n_a)
    for f in COPIED:
        out[f] = S[f][rows, win] if n_b else 0
    out["poly"] = (col_base + win).astype(np.uint32)
    out[~any_hit] = (NO_POLY, np.inf, 0.0, 0.0, NONE16, 0, 0, 0)
    out[bad_a] = (NO_POLY, 0.0, 0.0, 0.0, NONE16, 0, sref.BAD_PAIR, 0)
    return out


def casts(a, b, a_motion=None, b_motion=None, row_base=0, col_base=0, flags=0):
    """a, b: (vx f32[rows][n], vy, k u8[n] or None); a motion: None or (dx, dy) f32[n] -> CAST_DT[n_a]"""
    n_a, n_b = a[0].shape[1], b[0].shape[1]
    if n_a == 0:
        return np.zeros(0, CAST_DT)
    bad_a, bad_b = bad_counts(a), bad_counts(b)
    S = pair_records(a, b, a_motion, b_motion) if n_b else np.zeros((n_a, 0), sref.SWEEP_DT)
    return reduce(S, bad_a, bad_b, row_base, col_base, flags)


def same(got, want):
    """every field equal; the three floats bit for bit, except that +0 and -0 are equal"""
    ok = np.ones(len(want), bool)
    for f in FLOATS:
        g, w = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        ok &= (g.view(np.uint32) == w.view(np.uint32)) | ((g == 0) & (w == 0))
    for f in ("poly", "axis", "hit", "flags", "reserved0"):
        ok &= got[f] == want[f]
    return ok
