"""The reference of c2d_poly_near_broad_pairs (include/c2d.h): tests/distance_ref.py's poly_distances over all pairs of the two sets,
keeping hit | (dist <= max_dist) — a float32 compare on the record's own dist — in row-major order, with the upper-triangle predicate
and absent polygons (a vertex count outside 1..rows) removed.  It is the judge of every test of the call; it knows nothing of the
kernel's boxes, grid or constants.

pairs(...) is that statement, literally, while the all-pairs list stays small.  Above `direct_limit` pairs it decides, before the judge
sees them, the pairs whose answer is plain; every other pair still goes through poly_distances.
  not hit   the judge's OWN pairwise test already separates on one of six single axes (edges 0, 1, 2 of A and of B): contact_ref's
            _interval and the compare of its _Rule.add, the same float32 operations in the same order (for the first axis, which sees
            every pair, B's projections are made as one rows x columns matrix per vertex slot).  An axis that separates makes the pair
            a miss whatever the other axes say.  Only pairs that are not near are asked.
  not near  both polygons are tame (live coordinates finite, largest magnitude C within 2^-40 .. 2^50) and one lies beyond the other
            along some direction by G > 1.02 max_dist + 2^-8 (C_A + C_B), in float64: along x or y for the whole rows x columns
            matrix (_plainly_far), along five directions of the pair's own for what is left (_bounds, which gives the argument).
  near      one candidate of the pair, computed as distance_ref computes it, already has sqrt(d2) <= max_dist (_bounds): listed,
            hit or not.
test_near_broad_ref_cpu.py pins the two routes to each other, the bounds to the judge and candidate_d2 to distance_ref."""
import numpy as np

import contact_ref as cref
import distance_ref

F32 = np.float32


def present(s):
    """bool[n]: the vertex count of each polygon is inside 1..rows"""
    k = cref._counts(s)
    return (k >= 1) & (k <= s[0].shape[0])


def listed(rec, max_dist):
    """the contract's predicate on DISTANCE_DT records"""
    return (rec["hit"] == 1) | (rec["dist"] <= F32(max_dist))


def _extent(s):
    """(xlo, xhi, ylo, yhi, C f64[n], tame bool[n]) of the live vertices"""
    k = np.clip(cref._counts(s), 0, s[0].shape[0])
    live = np.arange(s[0].shape[0])[:, None] < k[None, :]
    x, y = np.asarray(s[0], np.float64), np.asarray(s[1], np.float64)
    with np.errstate(all="ignore"):
        finite = ~(live & ~(np.isfinite(x) & np.isfinite(y))).any(0)
        c = np.maximum(np.where(live, np.abs(x), 0.0).max(0), np.where(live, np.abs(y), 0.0).max(0))
        tame = finite & present(s) & (c >= 2.0 ** -40) & (c <= 2.0 ** 50)
        return (np.where(live, x, np.inf).min(0), np.where(live, x, -np.inf).max(0), np.where(live, y, np.inf).min(0),
                np.where(live, y, -np.inf).max(0), c, tame)


def _plainly_far(ea, eb, rows, cols, max_dist):
    """bool[rows][cols]: both tame and apart along x or y by more than 1.02 max_dist + 2^-8 (C_A + C_B): _bounds' rule with u = x or y"""
    axlo, axhi, aylo, ayhi, ca, ta = (v[rows][:, None] for v in ea)
    bxlo, bxhi, bylo, byhi, cb, tb = (v[cols][None, :] for v in eb)
    gap = np.maximum(np.maximum(bxlo - axhi, axlo - bxhi), np.maximum(bylo - ayhi, aylo - byhi))
    return ta & tb & (gap > 1.02 * float(max_dist) + 2.0 ** -8 * (ca + cb))


def _first_axis_separates(a, b, rows, cols):
    """bool[rows][cols]: axis 0 of the pair (edge 0 of A) separates in the pairwise test of contact_ref"""
    ka, kb = cref._counts(a)[rows], cref._counts(b)[cols]
    ax, ay = np.asarray(a[0], F32)[:, rows], np.asarray(a[1], F32)[:, rows]
    bx, by = np.asarray(b[0], F32)[:, cols], np.asarray(b[1], F32)[:, cols]
    own = np.arange(len(rows))
    with np.errstate(all="ignore"):
        e1 = np.where(1 < ka, 1, 0) if ax.shape[0] > 1 else np.zeros(len(rows), np.int64)
        nx, ny = -(ay[e1, own] - ay[0]), ax[e1, own] - ax[0]
        min_a, max_a, first_a = cref._interval(nx, ny, ax, ay, ka)
        shape = (len(rows), len(cols))
        min_b, max_b = np.full(shape, np.inf, F32), np.full(shape, -np.inf, F32)
        for r in range(min(bx.shape[0], int(kb.max(initial=0)))):
            real = (r < kb)[None, :]
            p = nx[:, None] * bx[r][None, :] + ny[:, None] * by[r][None, :]
            min_b, max_b = np.where(real, np.fmin(min_b, p), min_b), np.where(real, np.fmax(max_b, p), max_b)
        first_b = nx[:, None] * bx[0][None, :] + ny[:, None] * by[0][None, :]
        return ((max_a[:, None] < min_b) | (max_b < min_a[:, None])) & ~(np.isnan(first_a)[:, None] | np.isnan(first_b))


def _axis_separates(a, b, ii, jj, side, e):
    """bool[len(ii)]: the axis of edge e of A (side 0) or of B (side 1) separates the pairs (ii, jj) in the pairwise test of contact_ref"""
    ka, kb = cref._counts(a)[ii], cref._counts(b)[jj]
    ax, ay = np.asarray(a[0], F32)[:, ii], np.asarray(a[1], F32)[:, ii]
    bx, by = np.asarray(b[0], F32)[:, jj], np.asarray(b[1], F32)[:, jj]
    px, py, kp = (bx, by, kb) if side else (ax, ay, ka)
    if e >= px.shape[0]:
        return np.zeros(len(ii), bool)
    own = np.arange(len(ii))
    with np.errstate(all="ignore"):
        live = e < kp
        e0, e1 = np.where(live, e, 0), np.where(e + 1 < kp, e + 1, 0)
        nx, ny = -(py[e1, own] - py[e0, own]), px[e1, own] - px[e0, own]
        min_a, max_a, first_a = cref._interval(nx, ny, ax, ay, ka)
        min_b, max_b, first_b = cref._interval(nx, ny, bx, by, kb)
        return live & ((max_a < min_b) | (max_b < min_a)) & ~(np.isnan(first_a) | np.isnan(first_b))


def candidate_d2(px, py, kp, e, qx, qy):
    """f32[m]: the d2 of one candidate per pair — edge e[m] of P (x, y f32[rows][m], kp live vertices) against the point (qx, qy) —
    by distance_ref's own float32 operations in their order (test_near_broad_ref_cpu.py pins the restatement bit for bit)"""
    cols = np.arange(px.shape[1])
    e1 = np.where(e + 1 < kp, e + 1, 0)
    x0, y0, x1, y1 = px[e, cols], py[e, cols], px[e1, cols], py[e1, cols]
    ex, ey = x1 - x0, y1 - y0
    len2 = ex * ex + ey * ey
    ux, uy = qx - x0, qy - y0
    s = ux * ex + uy * ey
    r0 = s <= 0
    r1 = ~r0 & (s >= len2)
    t = s / len2
    cx = np.where(r0, x0, np.where(r1, x1, x0 + t * ex))
    cy = np.where(r0, y0, np.where(r1, y1, y0 + t * ey))
    dx, dy = qx - cx, qy - cy
    return dx * dx + dy * dy


def _bounds(a, b, ii, jj, tame_a, tame_b, max_dist, step=1 << 14):
    """(near, apart) bool[len(ii)]: the pair's dist is surely <= max_dist, surely > max_dist.  Both start from the live vertices of A
    and of B nearest to each other (three greedy steps from A's first vertex) and the two edges of either polygon that end in them; a
    poor guess costs a walk through the judge, never a wrong answer.
      near   one of the four candidates vertex against such an edge of the other polygon has sqrt(d2) <= max_dist, by candidate_d2.  The
             record's dist is the root of the SMALLEST usable d2 (the sequential pick keeps the first and replaces it under strict <, a
             NaN is never taken) and the root is monotone: the pair is listed, with no slack to argue about.
      apart  both polygons are tame and along one of five directions u (vertex to vertex, the four edges' normals) all of A lies
             G > 1.02 max_dist + 2^-8 (C_A + C_B) beyond all of B, or the reverse, in float64.  Every candidate's computed closest
             point lies within 2^-20 C of its edge (c2d_clearance_bound.hpp proves 5.01 * 2^-24 C), so within that of the hull, and its
             vertex is a vertex of the other polygon: the computed offset has at least G - 2^-19 C along u, and the differences, squares,
             sum and root lose less than 2^-20 of it: dist > 0.99 (G - 2^-19 C) > max_dist."""
    near, apart = np.zeros(len(ii), bool), np.zeros(len(ii), bool)
    r = F32(max_dist)
    for s0 in range(0, len(ii), step):
        i, j = ii[s0:s0 + step], jj[s0:s0 + step]
        cols = np.arange(len(i))
        ka, kb = cref._counts(a)[i], cref._counts(b)[j]
        ax, ay = np.asarray(a[0], F32)[:, i], np.asarray(a[1], F32)[:, i]
        bx, by = np.asarray(b[0], F32)[:, j], np.asarray(b[1], F32)[:, j]
        live_a, live_b = np.arange(ax.shape[0])[:, None] < ka[None, :], np.arange(bx.shape[0])[:, None] < kb[None, :]

        def nearest(px, py, live, x, y):
            return np.argmin(np.where(live, (px - x) ** 2 + (py - y) ** 2, np.inf), axis=0)    # (0, a live vertex, when nothing compares)

        with np.errstate(all="ignore"):
            vb = nearest(bx, by, live_b, ax[0], ay[0])
            va = nearest(ax, ay, live_a, bx[vb, cols], by[vb, cols])
            vb = nearest(bx, by, live_b, ax[va, cols], ay[va, cols])
            wa, wb = np.where(va > 0, va, ka) - 1, np.where(vb > 0, vb, kb) - 1            # the edges that end in va, in vb
            qa, qb = (ax[va, cols], ay[va, cols]), (bx[vb, cols], by[vb, cols])
            best = np.full(len(i), np.nan, F32)
            for d2 in (candidate_d2(ax, ay, ka, va, *qb), candidate_d2(ax, ay, ka, wa, *qb),
                       candidate_d2(bx, by, kb, vb, *qa), candidate_d2(bx, by, kb, wb, *qa)):
                best = np.fmin(best, d2)
            near[s0:s0 + step] = np.sqrt(best) <= r                   # (NaN compares false)
            at = np.flatnonzero(~near[s0:s0 + step])                   # the rest of the step: apart?
            if len(at) == 0:
                continue
            i, j, cols, ka, kb, va, vb, wa, wb = i[at], j[at], np.arange(len(at)), ka[at], kb[at], va[at], vb[at], wa[at], wb[at]
            live_a, live_b, qa, qb = live_a[:, at], live_b[:, at], (qa[0][at], qa[1][at]), (qb[0][at], qb[1][at])
            dax, day, dbx, dby = (np.asarray(v[:, at], np.float64) for v in (ax, ay, bx, by))
            gap = np.full(len(i), -np.inf)
            nrm = lambda x, y, e0, e1: (-(y[e1, cols] - y[e0, cols]), x[e1, cols] - x[e0, cols])      # noqa: E731
            for ux, uy in ((qb[0].astype(np.float64) - qa[0], qb[1].astype(np.float64) - qa[1]), nrm(dax, day, wa, va),
                           nrm(dax, day, va, np.where(va + 1 < ka, va + 1, 0)), nrm(dbx, dby, wb, vb),
                           nrm(dbx, dby, vb, np.where(vb + 1 < kb, vb + 1, 0))):
                pa, pb = ux * dax + uy * day, ux * dbx + uy * dby
                g = np.maximum(np.where(live_b, pb, np.inf).min(0) - np.where(live_a, pa, -np.inf).max(0),
                               np.where(live_a, pa, np.inf).min(0) - np.where(live_b, pb, -np.inf).max(0)) / np.hypot(ux, uy)
                gap = np.fmax(gap, g)
            ca = np.maximum(np.where(live_a, np.abs(dax), 0.0).max(0), np.where(live_a, np.abs(day), 0.0).max(0))
            cb = np.maximum(np.where(live_b, np.abs(dbx), 0.0).max(0), np.where(live_b, np.abs(dby), 0.0).max(0))
            apart[s0 + at] = tame_a[i] & tame_b[j] & (gap > 1.02 * float(max_dist) + 2.0 ** -8 * (ca + cb))
    return near, apart


def _distances(a, b, ii, jj, step=1 << 12):
    """distance_ref.poly_distances in steps whose arrays stay in the cache"""
    if len(ii) == 0:
        return np.zeros(0, distance_ref.DISTANCE_DT)
    return np.concatenate([distance_ref.poly_distances(a, b, ii[s:s + step], jj[s:s + step]) for s in range(0, len(ii), step)])


def records(a, b, ii, jj):
    """the distance records of the listed pairs (ii, jj)"""
    return distance_ref.poly_distances(a, b, ii, jj)


def pairs(a, b, max_dist, upper=False, direct_limit=1 << 18, chunk=1 << 21, far_cache=None):
    """a, b: (vx f32[rows][n], vy, k u8[n] or None) -> u32[total][2], row-major.  far_cache: a dict in which the prefilter keeps the
    first-axis matrices between calls that differ in max_dist ONLY: one dict per (a, b, upper, chunk)"""
    n_a, n_b = a[0].shape[1], b[0].shape[1]
    if n_a == 0 or n_b == 0:
        return np.zeros((0, 2), np.uint32)
    ok_a, ok_b = present(a), present(b)
    cols = np.flatnonzero(ok_b)
    direct = n_a * n_b <= direct_limit
    if not direct:
        ea, eb = _extent(a), _extent(b)
    rows_per = max(1, chunk // max(1, n_b))
    out = []
    for r0 in range(0, n_a, rows_per):
        rows = np.arange(r0, min(n_a, r0 + rows_per))
        rows = rows[ok_a[rows]]
        cc = cols[cols > rows[0]] if upper and len(rows) else cols      # (the columns that some row of the chunk can pair with)
        if len(rows) == 0 or len(cc) == 0:
            continue
        if direct:
            ii, jj = np.repeat(rows, len(cc)), np.tile(cc, len(rows))
            near = np.zeros(len(ii), bool)
        else:
            sep = far_cache.get(r0) if far_cache is not None else None
            if sep is None:
                sep = _first_axis_separates(a, b, rows, cc)
                if far_cache is not None:
                    far_cache[r0] = sep
            far = _plainly_far(ea, eb, rows, cc, max_dist)
            ri, ci = np.nonzero(~(sep & far) & ((cc[None, :] > rows[:, None]) if upper else True))
            ii, jj, far = rows[ri], cc[ci], far[ri, ci]
            near = np.zeros(len(ii), bool)
            at = np.flatnonzero(~far)
            near[at], far[at] = _bounds(a, b, ii[at], jj[at], ea[5], eb[5], max_dist)
            for side, e in ((1, 0), (0, 1), (1, 1), (0, 2), (1, 2)):      # further single axes, for the pairs that are not near only
                at = np.flatnonzero(far)
                keep = np.ones(len(ii), bool)
                keep[at] = ~_axis_separates(a, b, ii[at], jj[at], side, e)
                ii, jj, far, near = ii[keep], jj[keep], far[keep], near[keep]
        if upper:
            keep = jj > ii
            ii, jj, near = ii[keep], jj[keep], near[keep]
        rest = np.flatnonzero(~near)
        near[rest] = listed(_distances(a, b, ii[rest], jj[rest]), max_dist)
        out.append(np.stack([ii[near], jj[near]], axis=1))
    if not out:
        return np.zeros((0, 2), np.uint32)
    return np.concatenate(out).astype(np.uint32).reshape(-1, 2)
