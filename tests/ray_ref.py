"""CPU restatement of the ray contract of include/c2d.h (c2d_poly_ray_casts), written from the contract, not from the kernel: plain
numpy float32, element-wise and unfused (numpy never contracts a * b - c * d), / correctly rounded, and the sequential pick:
polygons in order of j, per polygon the inside candidate first and then the edges in order of e; a candidate replaces the best only
under strict t < best, so a NaN never wins and the first of equals stays.

ray_casts(rays, b, col_base) takes the four ray planes (ox, oy, dx, dy) and a polygon set (vx f32[rows][n], vy, k u8[n] or None) and
returns a RAY_HIT_DT record per ray; touched(rays, b) returns, per (ray, polygon), "the origin is inside or some edge is usable".
The work is chunked over rays: one chunk holds [rays of the chunk][polygons] arrays, one step per edge slot.  dtype=np.float64 runs
the same rule in double precision (the tests measure the float32 rule against it)."""
import numpy as np

RAY_HIT_DT = np.dtype([("poly", "<u4"), ("t", "<f4"), ("u", "<f4"), ("edge", "<u2"), ("hit", "u1"), ("flags", "u1")])
START_INSIDE = 1
NONE16, NONE32 = 0xFFFF, 0xFFFFFFFF
CHUNK_CELLS = 1 << 20        # (rays of a chunk) x (polygons)


def _counts(b):
    vx, _, k = b
    return np.full(vx.shape[1], vx.shape[0], np.int64) if k is None else np.asarray(k).astype(np.int64)


def _chunk(ox, oy, dx, dy, vx, vy, k):
    """one chunk of rays [m] against all polygons [rows][n] -> per (ray, polygon): inside bool, the best edge's t, u and
    index (-1: no edge was chosen), "some edge is usable" bool"""
    m, (rows, n) = len(ox), vx.shape
    dt = vx.dtype.type
    ox, oy, dx, dy = (v[:, None] for v in (ox, oy, dx, dy))
    present = (k >= 1) & (k <= rows)
    best_t = np.full((m, n), np.inf, dt)
    best_u = np.zeros((m, n), dt)
    best_e = np.full((m, n), -1, np.int64)
    pos, neg, nan, some = (np.zeros((m, n), bool) for _ in range(4))
    cols = np.arange(n)
    for e in range(rows):
        live = (present & (e < k))[None, :]
        if not live.any():
            break
        e1 = np.where((e + 1 < k) & (e + 1 < rows), e + 1, 0)    # the vertex index wraps at k (a count beyond the rows: not live)
        x0, y0, x1, y1 = vx[e][None, :], vy[e][None, :], vx[e1, cols][None, :], vy[e1, cols][None, :]
        ex, ey = x1 - x0, y1 - y0
        wx, wy = x0 - ox, y0 - oy
        den = dx * ey - dy * ex
        tn = wx * ey - wy * ex
        un = wx * dy - wy * dx
        usable = live & (((den > 0) & (tn >= 0) & (tn <= den) & (un >= 0) & (un <= den)) |
                         ((den < 0) & (tn <= 0) & (tn >= den) & (un <= 0) & (un >= den)))
        some |= usable
        t, u = tn / den, un / den
        take = usable & (t < best_t)
        best_t, best_u, best_e = np.where(take, t, best_t), np.where(take, u, best_u), np.where(take, e, best_e)
        pos |= live & (tn > 0)
        neg |= live & (tn < 0)
        nan |= live & np.isnan(tn)
    inside = ~nan & (pos != neg)
    return inside, best_t, best_u, best_e, some


def _run(rays, b, dtype, visit):
    ox, oy, dx, dy = (np.asarray(v, np.float32).astype(dtype) for v in rays)
    vx, vy = np.asarray(b[0], np.float32).astype(dtype), np.asarray(b[1], np.float32).astype(dtype)
    k = _counts(b)
    n_rays, n = len(ox), vx.shape[1]
    step = max(1, CHUNK_CELLS // max(n, 1))
    with np.errstate(all="ignore"):
        for r0 in range(0, n_rays, step):
            s = slice(r0, min(n_rays, r0 + step))
            visit(s, *_chunk(ox[s], oy[s], dx[s], dy[s], vx, vy, k))


def ray_casts(rays, b, col_base=0, dtype=np.float32, with_t=False):
    """rays: (ox, oy, dx, dy), f32[n_rays] each; b: (vx f32[rows][n], vy, k u8[n] or None) -> RAY_HIT_DT[n_rays]
    with_t: also the winning t in `dtype` (inf when nothing was chosen)"""
    n_rays, n = len(rays[0]), np.asarray(b[0]).shape[1]
    out = np.zeros(n_rays, RAY_HIT_DT)
    out["poly"], out["t"], out["edge"] = NONE32, np.inf, NONE16
    t_full = np.full(n_rays, np.inf, dtype)

    def visit(s, inside, t, u, e, some):
        # per polygon: the inside candidate (t = 0) comes before the edges; across polygons the first of equal t wins
        tj = np.where(inside, t.dtype.type(0), t)
        j = np.argmin(tj, axis=1)                                # (the first minimum; -0 is not below +0; tj holds no NaN)
        rows = np.arange(len(j))
        tw, hit = tj[rows, j], tj[rows, j] < np.inf
        ins = hit & inside[rows, j]
        rec = out[s]
        rec["hit"] = hit
        rec["poly"] = np.where(hit, col_base + j, NONE32)
        rec["t"] = np.where(hit, tw, np.inf)
        rec["u"] = np.where(hit & ~ins, u[rows, j], 0)
        rec["edge"] = np.where(hit & ~ins, e[rows, j], NONE16)
        rec["flags"] = np.where(ins, START_INSIDE, 0)
        out[s] = rec
        t_full[s] = np.where(hit, tw, np.inf)

    if n and n_rays:
        _run(rays, b, dtype, visit)
    return (out, t_full) if with_t else out


def touched(rays, b, dtype=np.float32):
    """bool [n_rays][n]: the origin of the ray is inside the polygon, or some live edge of the polygon is usable"""
    n_rays, n = len(rays[0]), np.asarray(b[0]).shape[1]
    out = np.zeros((n_rays, n), bool)

    def visit(s, inside, t, u, e, some):
        out[s] = inside | some

    if n and n_rays:
        _run(rays, b, dtype, visit)
    return out


def same(got, want):
    """every field equal; t and u bit for bit, except that +0 and -0 are equal and that a NaN u (inf / inf: an infinite input)
    is any NaN"""
    ok = np.ones(len(want), bool)
    for f in ("t", "u"):
        g, w = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        ok &= (g.view(np.uint32) == w.view(np.uint32)) | ((g == 0) & (w == 0)) | (np.isnan(g) & np.isnan(w) & (f == "u"))
    for f in ("poly", "edge", "hit", "flags"):
        ok &= got[f] == want[f]
    return ok
