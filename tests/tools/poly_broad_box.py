"""A numpy restatement of the polygon broad phase's box rule (poly_broad_box in csrc/c2d_poly_broad.hip and
broad_box_of_slabs in csrc/c2d_broad.hpp), independent of the kernels: used by tests/test_poly_broad_margin_cpu.py and, for its
candidate counts, by csrc/tools/poly_broad_bench.py."""
import numpy as np

F32, F64 = np.float32, np.float64
KMAX = 16


def padded16(vx, vy, k):
    """(x, y) f32[16][n]: slots >= k repeat vertex 0 (slots >= k of the input are never read)"""
    vx, vy = np.asarray(vx, F32), np.asarray(vy, F32)
    rows, n = vx.shape
    k = np.full(n, rows, np.int64) if k is None else np.asarray(k).astype(np.int64)
    x, y = np.repeat(vx[:1], KMAX, axis=0), np.repeat(vy[:1], KMAX, axis=0)
    use = np.arange(rows)[:, None] < k[None, :]
    x[:rows][use], y[:rows][use] = vx[use], vy[use]
    return x, y, k


def poly_broad_boxes(vx, vy, k):
    """vx, vy f32[rows][n], k [n] or None -> (box f32[4][n] = minx, miny, maxx, maxy; regular bool[n]).  Polygons with a count
    outside 1..rows are not regular either (the pipeline calls them absent)."""
    rows, n = np.asarray(vx).shape
    raw = np.full(n, rows, np.int64) if k is None else np.asarray(k).astype(np.int64)
    x, y, k = padded16(vx, vy, np.clip(raw, 1, rows))
    with np.errstate(all="ignore"):
        ok = (raw >= 1) & (raw <= rows) & (k >= 3) & np.isfinite(x).all(0) & np.isfinite(y).all(0)
        cmax = np.maximum(np.abs(np.where(np.isfinite(x), x, 0)).max(0), np.abs(np.where(np.isfinite(y), y, 0)).max(0)).astype(F64)
        ok &= cmax < 2.0 ** 60
        ex = (np.roll(x, -1, axis=0) - x).astype(F64)      # the float differences of the test: edge m = v[m+1 mod 16] - v[m]
        ey = (np.roll(y, -1, axis=0) - y).astype(F64)
        l1 = np.abs(ex) + np.abs(ey)
        usable = l1 >= 2.0 ** -80
        have = usable.any(0)
        p = np.argmax(usable, axis=0)                      # the first usable edge
        cols = np.arange(n)
        px, py, pl = ex[p, cols], ey[p, cols], l1[p, cols]
        score = np.where(usable, np.abs(px * ey - py * ex) / np.where(usable, l1, 1.0), 0.0)
        score[p, cols] = 0.0
        q = np.argmax(score, axis=0)                       # the first edge with the largest score, as the kernel's `>` keeps it
        ok &= have & (score[q, cols] > 0)
        qx, qy, ql = ex[q, cols], ey[q, cols], l1[q, cols]
        ax, ay = [-py, -qy], [px, qx]
        slo, shi = [], []
        for i, n1 in enumerate((pl, ql)):
            pr = ax[i] * x.astype(F64) + ay[i] * y.astype(F64)
            w = n1 * (2.0 ** -21 * cmax + 2.0 ** -66) + 2.0 ** -140
            slo.append(pr.min(0) - w)
            shi.append(pr.max(0) + w)
        det = ax[0] * ay[1] - ay[0] * ax[1]
        ok &= det != 0
        adet = np.where(det != 0, np.abs(det), 1.0)
        sdet = np.where(det != 0, det, 1.0)

        def rng(u0, u1, v0, v1):
            nlo = np.minimum(u0, u1) + np.minimum(v0, v1)
            nhi = np.maximum(u0, u1) + np.maximum(v0, v1)
            m = 2.0 ** -48 * (np.maximum(np.abs(u0), np.abs(u1)) + np.maximum(np.abs(v0), np.abs(v1))) / adet
            return np.where(det > 0, nlo, nhi) / sdet - m, np.where(det > 0, nhi, nlo) / sdet + m

        xlo, xhi = rng(slo[0] * ay[1], shi[0] * ay[1], -(slo[1] * ay[0]), -(shi[1] * ay[0]))
        ylo, yhi = rng(slo[1] * ax[0], shi[1] * ax[0], -(slo[0] * ax[1]), -(shi[0] * ax[1]))

        def down(d):
            f = d.astype(F32)
            return np.where(f.astype(F64) > d, np.nextafter(f, F32(-np.inf)), f)

        def up(d):
            f = d.astype(F32)
            return np.where(f.astype(F64) < d, np.nextafter(f, F32(np.inf)), f)

        box = np.stack([down(xlo), down(ylo), up(xhi), up(yhi)])
        ok &= np.isfinite(box).all(0)
    box[:, ~ok] = np.nan
    return box, ok
