"""The reference of c2d_poly_sweep_broad_pairs (include/c2d.h): np.argwhere of tests/sweep_ref.py's poly_sweeps(...)["hit"] over all
pairs of the two sets, in row-major order, with the upper-triangle predicate and absent polygons (a vertex count outside 1..rows)
removed.  It is the judge of every test of the call; it knows nothing of boxes, grids or the kernel.

pairs(...) is that statement, literally, while the all-pairs list stays small.  Above `direct_limit` pairs it drops, before the
judge sees them, pairs that the judge's OWN pick already misses on three single axes (edge 0 of A, edge 0 of B, edge 1 of A): the
pick is monotone in the set of axes — another axis can only raise t_in, lower t_out, set `never` or separate at t = 0 — so a pair
that is a miss on one axis alone is a miss on all of them.  The single-axis pick is sweep_ref's own _Pick and _interval (for the
first axis, which sees every pair, B's intervals are made as one rows x columns matrix per vertex slot: the same float32
operations in the same order), and every survivor still goes through poly_sweeps.  test_sweep_broad_ref_cpu.py pins the two routes
to each other."""
import numpy as np

import sweep_ref

F32 = np.float32


def present(s):
    """bool[n]: the vertex count of each polygon is inside 1..rows"""
    k = sweep_ref._counts(s)
    return (k >= 1) & (k <= s[0].shape[0])


def _single_axis_hit(a, b, ii, jj, a_motion, b_motion, side, e):
    """the pick of sweep_ref over ONE axis (edge e of A for side 0, of B for side 1) of the pairs (ii, jj): its `hit`"""
    m = len(ii)
    ka, kb = sweep_ref._counts(a)[ii], sweep_ref._counts(b)[jj]
    ax, ay = np.asarray(a[0], F32)[:, ii], np.asarray(a[1], F32)[:, ii]
    bx, by = np.asarray(b[0], F32)[:, jj], np.asarray(b[1], F32)[:, jj]
    px, py, kp = (bx, by, kb) if side else (ax, ay, ka)
    cols = np.arange(m)
    with np.errstate(all="ignore"):
        pick = sweep_ref._Pick(m, *sweep_ref._relative_motion(a_motion, b_motion, ii, jj, m, F32), F32)
        live = e < kp
        e0, e1 = np.where(live, e, 0), np.where(e + 1 < kp, e + 1, 0)
        if e >= px.shape[0]:
            return np.ones(m, bool)
        e1 = np.minimum(e1, px.shape[0] - 1)
        nx, ny = -(py[e1, cols] - py[e0, cols]), px[e1, cols] - px[e0, cols]
        pick.add(live, e, nx, ny, *sweep_ref._interval(nx, ny, ax, ay, ka, F32)[:2], *sweep_ref._interval(nx, ny, bx, by, kb, F32)[:2],
                 nx * ax[0] + ny * ay[0], nx * bx[0] + ny * by[0])
        return ~pick.sep | (~pick.never & (pick.t_in <= pick.t_out))


def _first_axis_hit(a, b, rows, cols, ii, jj, a_motion, b_motion):
    """_single_axis_hit(side 0, e 0) of the pairs (ii, jj) = rows x cols: B's projections as one [rows][cols] matrix per vertex slot"""
    ka, kb = sweep_ref._counts(a)[rows], sweep_ref._counts(b)[cols]
    ax, ay = np.asarray(a[0], F32)[:, rows], np.asarray(a[1], F32)[:, rows]
    bx, by = np.asarray(b[0], F32)[:, cols], np.asarray(b[1], F32)[:, cols]
    own = np.arange(len(rows))
    with np.errstate(all="ignore"):
        e1 = np.where(1 < ka, 1, 0) if ax.shape[0] > 1 else np.zeros(len(rows), np.int64)
        nx, ny = -(ay[e1, own] - ay[0]), ax[e1, own] - ax[0]
        min_a, max_a, first_a = sweep_ref._interval(nx, ny, ax, ay, ka, F32)
        pad = np.arange(bx.shape[0])[:, None] >= kb[None, :]
        mx_, my_ = np.where(pad, F32(np.nan), bx), np.where(pad, F32(np.nan), by)      # fmin / fmax pass over a NaN as over a padded slot
        shape = (len(rows), len(cols))
        min_b, max_b = np.full(shape, np.inf, F32), np.full(shape, -np.inf, F32)
        for r in range(bx.shape[0]):
            p = nx[:, None] * mx_[r][None, :] + ny[:, None] * my_[r][None, :]
            min_b, max_b = np.fmin(min_b, p), np.fmax(max_b, p)
        first_b = nx[:, None] * bx[0][None, :] + ny[:, None] * by[0][None, :]
        full = lambda v: np.broadcast_to(v[:, None], shape).ravel()   # noqa: E731
        m = len(rows) * len(cols)
        pick = sweep_ref._Pick(m, *sweep_ref._relative_motion(a_motion, b_motion, ii, jj, m, F32), F32)
        pick.add(np.ones(m, bool), 0, full(nx), full(ny), full(min_a), full(max_a), min_b.ravel(), max_b.ravel(), full(first_a), first_b.ravel())
        return ~pick.sep | (~pick.never & (pick.t_in <= pick.t_out))


def pairs(a, b, a_motion=None, b_motion=None, upper=False, direct_limit=1 << 18, chunk=1 << 21):
    """a, b: (vx f32[rows][n], vy, k u8[n] or None); motions: None or (dx, dy) f32[n] -> u32[total][2], row-major"""
    n_a, n_b = a[0].shape[1], b[0].shape[1]
    if n_a == 0 or n_b == 0:
        return np.zeros((0, 2), np.uint32)
    ok_a, ok_b = present(a), present(b)
    cols = np.flatnonzero(ok_b)
    direct = n_a * n_b <= direct_limit
    rows_per = max(1, chunk // max(1, n_b))
    out = []
    for r0 in range(0, n_a, rows_per):
        rows = np.arange(r0, min(n_a, r0 + rows_per))
        rows = rows[ok_a[rows]]
        cc = cols[cols > rows[0]] if upper and len(rows) else cols      # (the columns that some row of the chunk can pair with)
        ii, jj = np.repeat(rows, len(cc)), np.tile(cc, len(rows))
        if not direct and len(rows) and len(cc):
            keep = _first_axis_hit(a, b, rows, cc, ii, jj, a_motion, b_motion)
            ii, jj = ii[keep], jj[keep]
        if upper:
            keep = jj > ii
            ii, jj = ii[keep], jj[keep]
        if not direct:
            for side, e in ((1, 0), (0, 1)):
                keep = _single_axis_hit(a, b, ii, jj, a_motion, b_motion, side, e)
                ii, jj = ii[keep], jj[keep]
        hit = sweep_ref.poly_sweeps(a, b, ii, jj, a_motion, b_motion)["hit"] == 1
        out.append(np.stack([ii[hit], jj[hit]], axis=1))
    return np.concatenate(out).astype(np.uint32).reshape(-1, 2)


def _rows16(s, idx):
    """(vx, vy f32[16][m], k u8[m]) of polygons idx, the planes padded to 16 rows with zeros (slots >= k are never read)"""
    vx, vy = np.zeros((16, len(idx)), F32), np.zeros((16, len(idx)), F32)
    rows = s[0].shape[0]
    vx[:rows], vy[:rows] = np.asarray(s[0], F32)[:, idx], np.asarray(s[1], F32)[:, idx]
    return vx, vy, sweep_ref._counts(s)[idx].astype(np.uint8)


def static_pairs(oracle, a, b, upper=False):
    """the CPU oracle's static polygon test over all pairs of the two sets (absent polygons in no pair): u32[total][2], row-major"""
    n_a, n_b = a[0].shape[1], b[0].shape[1]
    ok_a, ok_b = present(a), present(b)
    ii, jj = np.repeat(np.arange(n_a), n_b), np.tile(np.arange(n_b), n_a)
    keep = ok_a[ii] & ok_b[jj] & ((jj > ii) if upper else True)
    ii, jj = ii[keep], jj[keep]
    if len(ii) == 0:
        return np.zeros((0, 2), np.uint32)
    pa, pb = _rows16(a, ii), _rows16(b, jj)
    res, _ = oracle.sat_poly_pairs(np.stack([pa[0], pb[0]]), np.stack([pa[1], pb[1]]), np.stack([pa[2], pb[2]]))
    hit0 = np.asarray(res) != 0
    return np.stack([ii[hit0], jj[hit0]], axis=1).astype(np.uint32).reshape(-1, 2)
