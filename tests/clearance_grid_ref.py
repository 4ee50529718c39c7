"""The reference of c2d_poly_set_clearances_grid (include/c2d.h, "clearance queries through a grid"), built from parts that exist and
nothing else: near_broad_ref.pairs for the considered pairs (hit | dist <= max_dist on the record's own dist, absent polygons removed),
distance_ref.poly_distances on exactly those pairs, a per-row minimum of (bits of dist, col_base + j), and the three special records
as clearance_ref.reduce writes them.  It knows nothing of boxes, grids or bounds.

clearances(a, b, max_dist, ...) -> CLEARANCE_DT[n_a];  considered(a, b, max_dist, ...) -> (ii, jj, records) of the considered pairs,
row-major, for callers that want the distances themselves (the margins of the GPU tests are taken from them)."""
import numpy as np

import clearance_ref as cref
import distance_ref as dref
import near_broad_ref as nref

CLEARANCE_DT = cref.CLEARANCE_DT
SKIP_SELF, NONE_FLAG = cref.SKIP_SELF, cref.NONE_FLAG
NONE_RECORD = (cref.NO_POLY, np.inf, 0.0, 0.0, 0.0, 0.0, cref.NONE16, cref.NONE16, 0, NONE_FLAG, 0)
BAD_RECORD = (cref.NO_POLY, 0.0, 0.0, 0.0, 0.0, 0.0, cref.NONE16, cref.NONE16, 0, dref.BAD_PAIR, 0)


def considered(a, b, max_dist, row_base=0, col_base=0, flags=0, step=1 << 12):
    """-> ii, jj (int64, row-major), rec DISTANCE_DT[len(ii)]: the pairs the contract considers, with their records"""
    p = nref.pairs(a, b, max_dist).astype(np.int64)
    ii, jj = p[:, 0], p[:, 1]
    if flags & SKIP_SELF:
        keep = row_base + ii != col_base + jj
        ii, jj = ii[keep], jj[keep]
    if len(ii) == 0:
        return ii, jj, np.zeros(0, dref.DISTANCE_DT)
    rec = np.concatenate([dref.poly_distances(a, b, ii[s:s + step], jj[s:s + step]) for s in range(0, len(ii), step)])
    return ii, jj, rec


def reduce_pairs(n_a, bad_a, ii, jj, rec, col_base=0):
    """the pick over the considered pairs (ii, jj) with records rec, and the three special records"""
    out = np.zeros(n_a, CLEARANCE_DT)
    out[:] = NONE_RECORD
    if len(ii):
        dist = np.ascontiguousarray(rec["dist"])
        assert not np.isnan(dist).any() and not (np.signbit(dist) & (dist == 0)).any()   # never NaN, never -0
        key = (dist.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(col_base) + jj.astype(np.uint64))
        order = np.lexsort((key, ii))                                   # by row, then by key
        first = order[np.concatenate([[True], ii[order][1:] != ii[order][:-1]])]   # the smallest key of each row that has a pair
        rows = ii[first]
        for f in cref.COPIED:
            out[f][rows] = rec[f][first]
        out["poly"][rows] = (col_base + jj[first]).astype(np.uint32)
        out["reserved0"][rows] = 0
    out[bad_a] = BAD_RECORD
    return out


def clearances(a, b, max_dist, row_base=0, col_base=0, flags=0):
    """a, b: (vx f32[rows][n], vy, k u8[n] or None) -> CLEARANCE_DT[n_a]"""
    n_a = a[0].shape[1]
    if n_a == 0:
        return np.zeros(0, CLEARANCE_DT)
    ii, jj, rec = considered(a, b, max_dist, row_base, col_base, flags)
    return reduce_pairs(n_a, cref.bad_counts(a), ii, jj, rec, col_base)


same = cref.same
