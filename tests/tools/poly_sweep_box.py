"""A numpy restatement of the swept broad phase's box rule (poly_sweep_box in csrc/c2d_sweep_broad.hip and
broad_box_of_slabs in csrc/c2d_broad.hpp), independent of the kernels: used by tests/test_sweep_broad_margin_cpu.py and, for its
candidate counts, by csrc/tools/sweep_broad_bench.py.

The rule: the parallelogram of §5.10 (the normals of the first usable edge p and of the edge q that maximises |det(e_p, e_q)| /
|e_q|_1), each slab widened by W = |e|_1 (2^-21 C + 2^-17 D + 2^-66) + 2^-140 with C the polygon's largest |coordinate| and D its
larger |motion component|; its box in double, rounded outward to float; then the hull of that float box and the same box displaced
by (dx, dy), each displaced bound moved outward by 2^-52 of itself and rounded outward.  Not regular: what §5.10 calls so, a
non-finite motion component, a |motion component| >= 2^60, a displaced |coordinate| >= 2^60."""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("poly_broad_box", os.path.join(os.path.dirname(os.path.abspath(__file__)), "poly_broad_box.py"))
pbb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pbb)

F32, F64 = np.float32, np.float64
C_TERM, D_TERM, ABS_TERM, FLOOR_TERM = 2.0 ** -21, 2.0 ** -17, 2.0 ** -66, 2.0 ** -140   # the constants of §5.19 step 4


def _down(d):
    f = d.astype(F32)
    return np.where(f.astype(F64) > d, np.nextafter(f, F32(-np.inf)), f)


def _up(d):
    f = d.astype(F32)
    return np.where(f.astype(F64) < d, np.nextafter(f, F32(np.inf)), f)


def poly_sweep_boxes(vx, vy, k, motion=None):
    """vx, vy f32[rows][n], k [n] or None, motion None or (dx, dy) f32[n] -> (box f32[4][n] = minx, miny, maxx, maxy; regular bool[n]).
    Polygons with a count outside 1..rows are not regular either (the pipeline calls them absent)."""
    rows, n = np.asarray(vx).shape
    raw = np.full(n, rows, np.int64) if k is None else np.asarray(k).astype(np.int64)
    x, y, k = pbb.padded16(vx, vy, np.clip(raw, 1, rows))
    dx = np.zeros(n, F32) if motion is None else np.asarray(motion[0], F32)
    dy = np.zeros(n, F32) if motion is None else np.asarray(motion[1], F32)
    with np.errstate(all="ignore"):
        ok = (raw >= 1) & (raw <= rows) & (k >= 3) & np.isfinite(x).all(0) & np.isfinite(y).all(0) & np.isfinite(dx) & np.isfinite(dy)
        dmax = np.maximum(np.abs(np.where(np.isfinite(dx), dx, 0)), np.abs(np.where(np.isfinite(dy), dy, 0))).astype(F64)
        cmax = np.maximum(np.abs(np.where(np.isfinite(x), x, 0)).max(0), np.abs(np.where(np.isfinite(y), y, 0)).max(0)).astype(F64)
        moved = np.maximum(np.abs(x.astype(F64) + dx.astype(F64)).max(0), np.abs(y.astype(F64) + dy.astype(F64)).max(0))
        ok &= (cmax < 2.0 ** 60) & (dmax < 2.0 ** 60) & (moved < 2.0 ** 60)
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
            w = n1 * (C_TERM * cmax + D_TERM * dmax + ABS_TERM) + FLOOR_TERM
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
        b0 = np.stack([_down(xlo), _down(ylo), _up(xhi), _up(yhi)])
        ok &= np.isfinite(b0).all(0)
        ddx, ddy = dx.astype(F64), dy.astype(F64)
        x0, y0, x1, y1 = b0[0].astype(F64) + ddx, b0[1].astype(F64) + ddy, b0[2].astype(F64) + ddx, b0[3].astype(F64) + ddy
        e = 2.0 ** -52
        box = np.stack([np.fmin(b0[0], _down(x0 - e * np.abs(x0))), np.fmin(b0[1], _down(y0 - e * np.abs(y0))),
                        np.fmax(b0[2], _up(x1 + e * np.abs(x1))), np.fmax(b0[3], _up(y1 + e * np.abs(y1)))])
        ok &= np.isfinite(box).all(0)
    box[:, ~ok] = np.nan
    return box, ok
