"""A numpy restatement of the proximity pair search's box rule (poly_near_box in csrc/c2d_near_broad.hip), independent
of the kernels: used by tests/test_near_broad_margin_cpu.py and, for its candidate counts, by csrc/tools/near_broad_bench.py.

The rule: the hull of (1) §5.10's own-axes box (tests/tools/poly_broad_box.py) and (2) the exact float box of the live vertices widened
on every side by the half-margin h = (r (1 + 2^-19) + [r < 2^-60: r] + 2^-72) / 2 + 2^-20 C, with r the call's max_dist and C the
polygon's largest |coordinate|; each widened bound in double, moved outward by 2^-52 of itself and rounded outward to float.  Not
regular: what §5.10 calls so, and a largest |coordinate| below 2^-100."""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("poly_broad_box", os.path.join(os.path.dirname(os.path.abspath(__file__)), "poly_broad_box.py"))
pbb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pbb)

F32, F64 = np.float32, np.float64
R_REL, R_SMALL, R_FLOOR, C_TERM, C_MIN = 2.0 ** -19, 2.0 ** -60, 2.0 ** -72, 2.0 ** -20, 2.0 ** -100   # the constants of §5.20 part 2


def _down(d):
    f = d.astype(F32)
    return np.where(f.astype(F64) > d, np.nextafter(f, F32(-np.inf)), f)


def _up(d):
    f = d.astype(F32)
    return np.where(f.astype(F64) < d, np.nextafter(f, F32(np.inf)), f)


def half_margin(r, c):
    r = np.float64(np.float32(r))
    return 0.5 * (r * (1.0 + R_REL) + (r if r < R_SMALL else 0.0) + R_FLOOR) + C_TERM * np.asarray(c, F64)


def poly_near_boxes(vx, vy, k, max_dist):
    """vx, vy f32[rows][n], k [n] or None, max_dist -> (box f32[4][n] = minx, miny, maxx, maxy; regular bool[n]).  Polygons with a
    count outside 1..rows are not regular either (the pipeline calls them absent)."""
    rows, n = np.asarray(vx).shape
    raw = np.full(n, rows, np.int64) if k is None else np.asarray(k).astype(np.int64)
    own, ok = pbb.poly_broad_boxes(vx, vy, k)
    x, y, _ = pbb.padded16(vx, vy, np.clip(raw, 1, rows))
    with np.errstate(all="ignore"):
        cmax = np.maximum(np.abs(np.where(np.isfinite(x), x, 0)).max(0), np.abs(np.where(np.isfinite(y), y, 0)).max(0)).astype(F64)
        ok = ok & (cmax >= C_MIN)
        h = half_margin(max_dist, cmax)
        e = 2.0 ** -52
        x0, y0, x1, y1 = x.min(0).astype(F64) - h, y.min(0).astype(F64) - h, x.max(0).astype(F64) + h, y.max(0).astype(F64) + h
        box = np.stack([np.fmin(own[0], _down(x0 - e * np.abs(x0))), np.fmin(own[1], _down(y0 - e * np.abs(y0))),
                        np.fmax(own[2], _up(x1 + e * np.abs(x1))), np.fmax(own[3], _up(y1 + e * np.abs(y1)))])
        ok &= np.isfinite(box).all(0)
    box[:, ~ok] = np.nan
    return box, ok


def disjoint(box_a, box_b):
    return (box_a[2] < box_b[0]) | (box_b[2] < box_a[0]) | (box_a[3] < box_b[1]) | (box_b[3] < box_a[1])
