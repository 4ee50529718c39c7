"""CPU restatement of the clearance contract of include/c2d.h (c2d_poly_set_clearances), written from the contract: the reduction over
tests/distance_ref.py's poly_distances and nothing else.  For query i, D(i, j) is the distance record of the pair (A_i, B_j); polygon
j is considered when its vertex count is within 1..rows and it is not the self pair (under SKIP_SELF the pair with
row_base + i == col_base + j); the winner is the considered polygon with the smallest key (bits of D(i, j).dist, col_base + j).

clearances(a, b, ...) -> CLEARANCE_DT[n_a].  pair_records(a, b) -> the D(i, j) of all pairs [n_a][n_b], for callers that want the
same scene reduced more than once (reduce())."""
import numpy as np

import contact_ref as cref
import distance_ref as dref

CLEARANCE_DT = np.dtype([("poly", "<u4"), ("dist", "<f4"), ("ax", "<f4"), ("ay", "<f4"), ("bx", "<f4"), ("by", "<f4"), ("edge", "<u2"), ("vert", "<u2"),
                         ("hit", "u1"), ("flags", "u1"), ("reserved0", "<u2")])
SKIP_SELF, NONE_FLAG = 1, 16
NO_POLY, NONE16 = 0xFFFFFFFF, 0xFFFF
FLOATS = dref.FLOATS
COPIED = FLOATS + ("edge", "vert", "hit", "flags")


def bad_counts(s):
    """per polygon: its vertex count is outside 1..rows"""
    k = cref._counts(s)
    return (k < 1) | (k > s[0].shape[0])


def pair_records(a, b):
    """D(i, j) of every pair -> DISTANCE_DT[n_a][n_b] (BAD_PAIR entries where either count is out of range)"""
    n_a, n_b = a[0].shape[1], b[0].shape[1]
    i, j = np.repeat(np.arange(n_a), n_b), np.tile(np.arange(n_b), n_a)
    return dref.poly_distances(a, b, i, j).reshape(n_a, n_b)


def reduce(D, bad_a, bad_b, row_base=0, col_base=0, flags=0):
    """the pick and the three special records, from the per-pair records D [n_a][n_b]"""
    n_a, n_b = D.shape
    out = np.zeros(n_a, CLEARANCE_DT)
    considered = np.broadcast_to(~bad_b[None, :], (n_a, n_b)).copy()
    if flags & SKIP_SELF:
        considered &= (row_base + np.arange(n_a))[:, None] != (col_base + np.arange(n_b))[None, :]
    bits = np.ascontiguousarray(D["dist"]).view(np.uint32).astype(np.uint64)
    assert not np.isnan(D["dist"]).any() and not (np.signbit(D["dist"]) & (D["dist"] == 0)).any()   # never NaN, never -0
    key = (bits << np.uint64(32)) | (np.uint64(col_base) + np.arange(n_b, dtype=np.uint64))[None, :]
    key = np.where(considered, key, np.uint64(0xFFFFFFFFFFFFFFFF))
    any_considered = considered.any(axis=1) if n_b else np.zeros(n_a, bool)
    win = key.argmin(axis=1) if n_b else np.zeros(n_a, np.int64)   # (argmin: the first of equal keys; keys differ in j anyway)
    rows = np.arange(n_a)
    for f in COPIED:
        out[f] = D[f][rows, win] if n_b else 0
    out["poly"] = (col_base + win).astype(np.uint32)
    none = ~any_considered
    out[none] = (NO_POLY, np.inf, 0.0, 0.0, 0.0, 0.0, NONE16, NONE16, 0, NONE_FLAG, 0)
    out[bad_a] = (NO_POLY, 0.0, 0.0, 0.0, 0.0, 0.0, NONE16, NONE16, 0, dref.BAD_PAIR, 0)
    return out


def clearances(a, b, row_base=0, col_base=0, flags=0):
    """a, b: (vx f32[rows][n], vy, k u8[n] or None) -> CLEARANCE_DT[n_a]"""
    n_a, n_b = a[0].shape[1], b[0].shape[1]
    if n_a == 0:
        return np.zeros(0, CLEARANCE_DT)
    bad_a, bad_b = bad_counts(a), bad_counts(b)
    D = pair_records(a, b) if n_b else np.zeros((n_a, 0), dref.DISTANCE_DT)
    return reduce(D, bad_a, bad_b, row_base, col_base, flags)


def same(got, want):
    """every field equal; the five floats bit for bit, except that +0 and -0 are equal"""
    ok = np.ones(len(want), bool)
    for f in FLOATS:
        g, w = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        ok &= (g.view(np.uint32) == w.view(np.uint32)) | ((g == 0) & (w == 0))
    for f in ("poly", "edge", "vert", "hit", "flags", "reserved0"):
        ok &= got[f] == want[f]
    return ok
