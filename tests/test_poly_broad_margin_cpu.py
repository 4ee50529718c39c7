"""CPU check of the polygon broad phase's box rule, independent of the kernel: a numpy restatement of
poly_broad_box (tests/tools/poly_broad_box.py) and the CPU oracle on adversarial polygon pairs.  Whenever the boxes of two regular
polygons are disjoint, the polygon test must report "no collision" — for near-regular and irregular convex polygons with 3 to 16
vertices, slivers, polygons whose first edges are nearly parallel, clockwise ones and ones with repeated vertices, at scales from
1e-20 to 1e15, with the second polygon pushed to within a few ulps of the first one's box on each side.  Padded slots hold NaN."""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("poly_broad_box", os.path.join(HERE, "tools", "poly_broad_box.py"))
pbb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pbb)
F32, F64 = np.float32, np.float64
KINDS = ["regular", "irregular", "sliver", "nearpar", "clockwise", "repeated"]
N_PER_COMBO = 40_000               # pairs per combination of two families: 18 combinations per scale
MIN_DISJOINT, MIN_CLOSE = 0.5, 0.2


def polygons(rng, n, kind, scale):
    """(vx, vy f32[16][n], k u8[n]) of one family around the origin, size ~ scale; slots >= k hold NaN"""
    k = rng.integers(4 if kind == "repeated" else 3, 17, n)
    used = np.arange(16)[:, None] < k[None, :]
    if kind == "regular":
        ang = 2 * np.pi * (np.arange(16)[:, None] + rng.uniform(-0.3, 0.3, (16, n))) / k[None, :]
    else:
        ang = np.where(used, rng.uniform(0, 2 * np.pi, (16, n)), np.inf)
        if kind == "nearpar":   # vertices 0, 1, 2 almost on one line: edges 0 and 1 differ by 1e-4 .. 1e-2 rad
            d = np.exp(rng.uniform(np.log(1e-4), np.log(1e-2), n))
            ang[0] = rng.uniform(0, 1, n)
            ang[1], ang[2] = ang[0] + d, ang[0] + d * rng.uniform(2, 3, n)
            ang[3:] = np.where(used[3:], rng.uniform(1.5, 2 * np.pi, (13, n)), np.inf)
        ang = np.sort(ang, axis=0)
    a = rng.uniform(0.05, 1, n) * scale
    b = rng.uniform(0.05, 1, n) * scale
    if kind == "sliver":
        b = a * 10 ** rng.uniform(-4, -1.5, n)
    ang = np.where(used, ang, 0.0)
    x, y = a * np.cos(ang), b * np.sin(ang)
    if kind == "clockwise":   # the used slots in reverse order
        idx = np.where(used, k[None, :] - 1 - np.arange(16)[:, None], np.arange(16)[:, None])
        x, y = np.take_along_axis(x, idx, 0), np.take_along_axis(y, idx, 0)
    if kind == "repeated":    # vertex j + 1 repeats vertex j
        j = rng.integers(0, k - 1)
        cols = np.arange(n)
        x[j + 1, cols], y[j + 1, cols] = x[j, cols], y[j, cols]
    rot = rng.uniform(0, 2 * np.pi, n)
    c, s = np.cos(rot), np.sin(rot)
    ctr = rng.uniform(-1, 1, (2, n)) * scale
    vx, vy = c * x - s * y + ctr[0], s * x + c * y + ctr[1]
    vx, vy = np.where(used, vx, np.nan), np.where(used, vy, np.nan)
    return vx.astype(F32), vy.astype(F32), k.astype(np.uint8)


def push_beyond(box_a, box_b, b, rng):
    """b translated so that its box starts just past box_a's edge (right, top or diagonally), by 0 to a few ulps or a few parts in
    1e7, or ends just in front of box_a's left / bottom edge; returns the moved polygons (float32)"""
    vx, vy, k = b
    n = vx.shape[1]
    side = rng.integers(0, 3, n)
    flip = rng.random(n) < 0.5         # approach from the left / from below instead
    gap_rel = rng.choice([0.0, 1e-7, 3e-7, 1e-6, 1e-5], n)
    hi_x, hi_y = box_a[2].astype(F64), box_a[3].astype(F64)
    lo_x, lo_y = box_a[0].astype(F64), box_a[1].astype(F64)
    dx = np.where(flip, (lo_x - box_b[2]) * (1 + gap_rel) - np.abs(lo_x) * gap_rel, (hi_x - box_b[0]) * (1 + gap_rel) + np.abs(hi_x) * gap_rel)
    dy = np.where(flip, (lo_y - box_b[3]) * (1 + gap_rel) - np.abs(lo_y) * gap_rel, (hi_y - box_b[1]) * (1 + gap_rel) + np.abs(hi_y) * gap_rel)
    dx = np.where(side == 1, rng.uniform(-1, 1, n) * (hi_x - lo_x), dx)
    dy = np.where(side == 0, rng.uniform(-1, 1, n) * (hi_y - lo_y), dy)
    jitter = np.where(rng.random(n) < 0.5, 0.0, rng.integers(-4, 5, (16, n)) * 2.0 ** -24)   # +-4 ulps on half of them
    return ((vx.astype(F64) + dx) * (1 + jitter)).astype(F32), ((vy.astype(F64) + dy) * (1 + jitter)).astype(F32), k


@pytest.mark.parametrize("scale", [1e-20, 1e-6, 1.0, 1e4, 1e15])
def test_disjoint_boxes_never_collide(oracle, scale):
    rng = np.random.default_rng(int(np.log10(scale)) + 300)
    n = N_PER_COMBO
    tested = close = total = 0
    for ia, ka in enumerate(KINDS):
        for kb in (KINDS[ia], KINDS[(ia + 1) % 6], KINDS[(ia + 3) % 6]):
            a = polygons(rng, n, ka, scale)
            b = polygons(rng, n, kb, scale)
            box_a, ok_a = pbb.poly_broad_boxes(*a)
            box_b, _ = pbb.poly_broad_boxes(*b)
            b = push_beyond(box_a, box_b, b, rng)
            box_b, ok_b = pbb.poly_broad_boxes(*b)
            keep = ok_a & ok_b
            disjoint = keep & ((box_a[2] < box_b[0]) | (box_b[2] < box_a[0]) | (box_a[3] < box_b[1]) | (box_b[3] < box_a[1]))
            sel = np.flatnonzero(disjoint)
            res, _ = oracle.sat_poly_pairs(np.stack([a[0][:, sel], b[0][:, sel]]), np.stack([a[1][:, sel], b[1][:, sel]]),
                                           np.stack([a[2][sel], b[2][sel]]))
            bad = np.flatnonzero(res)
            assert bad.size == 0, f"{ka} / {kb} at scale {scale}: pair {sel[bad[0]]} collides with disjoint boxes"
            total += n
            tested += sel.size
            gap = np.maximum(np.maximum(box_b[0] - box_a[2], box_a[0] - box_b[2]), np.maximum(box_b[1] - box_a[3], box_a[1] - box_b[3]))[sel]
            close += int((gap.astype(F64) <= 1e-5 * scale * 4).sum())
    print(f"scale {scale}: {total} pairs, {tested} box-disjoint, {close} of those within 4e-5 of touching")
    # what the generator yields here: 62 to 69 % of the pairs are box-disjoint and reach the oracle; 56 % of those nearly touch, 28 % at
    # 1e-20, where the absolute 2^-66 term of the widening is no longer small against the polygons
    assert tested > MIN_DISJOINT * total and close > MIN_CLOSE * tested, (total, tested, close)


def test_wild_rule():
    """non-finite or huge real vertices, fewer than three vertices, collinear polygons and counts out of range are not regular;
    ordinary polygons are, their box contains every real vertex, and NaN in padded slots changes nothing"""
    rng = np.random.default_rng(7)
    vx, vy, k = polygons(rng, 2000, "irregular", 3.0)
    box, ok = pbb.poly_broad_boxes(vx, vy, k)
    assert ok.all()
    assert (box[0] <= np.nanmin(vx, 0)).all() and (box[2] >= np.nanmax(vx, 0)).all()
    assert (box[1] <= np.nanmin(vy, 0)).all() and (box[3] >= np.nanmax(vy, 0)).all()
    w = np.maximum(box[2] - box[0], box[3] - box[1])
    size = np.maximum(np.nanmax(vx, 0) - np.nanmin(vx, 0), np.nanmax(vy, 0) - np.nanmin(vy, 0))
    assert np.median(w / size) < 2.0, "the parallelogram's box is far larger than the polygon"
    zx, zy = np.nan_to_num(vx), np.nan_to_num(vy)      # zeros instead of NaN in the padded slots: the same boxes
    box0, _ = pbb.poly_broad_boxes(zx, zy, k)
    assert np.array_equal(box0, box)
    bx, by, bk = vx[:, :8].copy(), vy[:, :8].copy(), k[:8].copy()
    bx[1, 0] = np.nan
    by[0, 1] = np.inf
    bx[:, 2] *= F32(2.0 ** 61)
    bk[3] = 2
    t = np.linspace(0, 1, 16, dtype=F32)
    bx[:, 4], by[:, 4] = t, F32(2) * t                   # every vertex on one line
    bk[5], bk[6] = 0, 17
    _, ok = pbb.poly_broad_boxes(bx, by, bk)
    assert not ok[:7].any() and ok[7]
