"""CPU restatement of the contract of c2d_poly_ray_casts_grid (include/c2d.h "ray queries through a grid"), written from the contract,
not from the kernel: the float32 vertex box of every polygon, meets(r, j) in numpy float64 (element-wise, unfused, in the written
order), and per ray the pick of tests/ray_ref.py restricted to the polygons that are unboxed or that the ray meets.

boxes(b) -> xl, xh, yl, yh (f32[n]) and unboxed (bool[n]); meets(rays, b) -> bool[n_rays][n]; candidates(rays, b) -> unboxed | meets
on the polygons with a count in 1..rows; ray_casts(rays, b, col_base) -> RAY_HIT_DT[n_rays]."""
import numpy as np

import ray_ref as ref

RAY_HIT_DT, START_INSIDE, NONE16, NONE32, same = ref.RAY_HIT_DT, ref.START_INSIDE, ref.NONE16, ref.NONE32, ref.same
CHUNK_CELLS = 1 << 20        # (rays of a chunk) x (polygons)


def present(b):
    k = ref._counts(b)
    return (k >= 1) & (k <= np.asarray(b[0]).shape[0])


def boxes(b):
    """the binary32 min / max of the live vertices; unboxed: some live coordinate is NaN (polygons with a bad count: an empty box)"""
    vx, vy = np.asarray(b[0], np.float32), np.asarray(b[1], np.float32)
    rows, n = vx.shape
    k = np.where(present(b), ref._counts(b), 0)
    live = np.arange(rows)[:, None] < k[None, :]
    nan = (live & (np.isnan(vx) | np.isnan(vy))).any(axis=0)
    with np.errstate(all="ignore"):
        xl = np.where(live, np.nan_to_num(vx, nan=np.inf, posinf=np.inf, neginf=-np.inf), np.inf).min(axis=0, initial=np.inf)
        xh = np.where(live, np.nan_to_num(vx, nan=-np.inf, posinf=np.inf, neginf=-np.inf), -np.inf).max(axis=0, initial=-np.inf)
        yl = np.where(live, np.nan_to_num(vy, nan=np.inf, posinf=np.inf, neginf=-np.inf), np.inf).min(axis=0, initial=np.inf)
        yh = np.where(live, np.nan_to_num(vy, nan=-np.inf, posinf=np.inf, neginf=-np.inf), -np.inf).max(axis=0, initial=-np.inf)
    return tuple(v.astype(np.float32) for v in (xl, xh, yl, yh)) + (nan,)


def _meets(ox, oy, dx, dy, xl, xh, yl, yh):
    """float64 arrays that broadcast against each other -> the contract's meets, step by step"""
    with np.errstate(all="ignore"):
        bx, by = ox + dx, oy + dy
        C = np.abs(ox)
        for v in (oy, bx, by, xl, xh, yl, yh):
            C = np.maximum(C, np.abs(v))            # (np.maximum hands a NaN on)
        m = 2.0 ** -20 * C
        sx = (np.minimum(ox, bx) > xh + m) | (np.maximum(ox, bx) < xl - m)
        sy = (np.minimum(oy, by) > yh + m) | (np.maximum(oy, by) < yl - m)
        cx, hx = 0.5 * xl + 0.5 * xh, (0.5 * xh - 0.5 * xl) + m
        cy, hy = 0.5 * yl + 0.5 * yh, (0.5 * yh - 0.5 * yl) + m
        sn = np.abs(dx * (cy - oy) - dy * (cx - ox)) > hx * np.abs(dy) + hy * np.abs(dx)
    return ~(sx | sy | sn)


def meets(rays, b, box=None):
    """bool [n_rays][n]: meets(r, j) on the polygons' boxes (whatever their counts)"""
    xl, xh, yl, yh, _ = (boxes(b) if box is None else box)
    r = [np.asarray(v, np.float32).astype(np.float64)[:, None] for v in rays]
    q = [v.astype(np.float64)[None, :] for v in (xl, xh, yl, yh)]
    return _meets(*r, *q)


def candidates(rays, b):
    """bool [n_rays][n]: polygon j has a count in 1..rows and is unboxed or met by ray r"""
    box = boxes(b)
    return present(b)[None, :] & (box[4][None, :] | meets(rays, b, box))


def ray_casts(rays, b, col_base=0):
    """rays: (ox, oy, dx, dy), f32[n_rays] each; b: (vx f32[rows][n], vy, k u8[n] or None) -> RAY_HIT_DT[n_rays]: ray_ref.ray_casts with
    every polygon that is not a candidate of the ray taken out"""
    rays = tuple(np.asarray(v, np.float32) for v in rays)
    n_rays, n = len(rays[0]), np.asarray(b[0]).shape[1]
    out = np.zeros(n_rays, RAY_HIT_DT)
    out["poly"], out["t"], out["edge"] = NONE32, np.inf, NONE16
    if not (n and n_rays):
        return out
    vx, vy = np.asarray(b[0], np.float32), np.asarray(b[1], np.float32)
    k = ref._counts(b)
    box = boxes(b)
    ok_poly = present(b)
    step = max(1, CHUNK_CELLS // n)
    with np.errstate(all="ignore"):
        for r0 in range(0, n_rays, step):
            s = slice(r0, min(n_rays, r0 + step))
            sub = tuple(v[s] for v in rays)
            cand = ok_poly[None, :] & (box[4][None, :] | meets(sub, b, box))
            inside, t, u, e, _ = ref._chunk(*sub, vx, vy, k)
            tj = np.where(cand, np.where(inside, np.float32(0), t), np.float32(np.inf))
            j = np.argmin(tj, axis=1)
            rows = np.arange(len(j))
            tw = tj[rows, j]
            hit = tw < np.inf
            ins = hit & inside[rows, j]
            rec = out[s]
            rec["hit"] = hit
            rec["poly"] = np.where(hit, col_base + j, NONE32)
            rec["t"] = np.where(hit, tw, np.inf)
            rec["u"] = np.where(hit & ~ins, u[rows, j], 0)
            rec["edge"] = np.where(hit & ~ins, e[rows, j], NONE16)
            rec["flags"] = np.where(ins, START_INSIDE, 0)
            out[s] = rec
    return out
