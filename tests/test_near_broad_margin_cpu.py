"""CPU check of the proximity pair search's box rule, independent of the kernel: the numpy restatement of poly_near_box
(tests/tools/poly_near_box.py, which holds the proof's constants) and the judge (tests/near_broad_ref.py's predicate on
tests/distance_ref.py's records) on adversarial pairs.  Whenever the boxes of two regular polygons are disjoint, the pair must not be
listed: hit == 0 and dist > max_dist.

Families: the polygon families of test_poly_broad_margin_cpu.py (slivers among them) and axis-aligned rectangles, which meet face to
face — there the box bound is tight — or vertex to vertex on the diagonal; scales 1e-20 .. 1e15; margins 0, 1e-30 of the scale, one ulp
of C, a tenth of a polygon size, one size and 100 sizes.  B is pushed so that the boxes lie from a few ulps inside to a few ulps
beyond touching.  Two shares keep the test from passing vacuously and are asserted over the whole run: at least a third of the pairs
are box-disjoint, and at least a third of those have a dist within max_dist (1 + 2^-18) + 2^-18 C of the margin.  (Only the
rectangles can be that near: a slanted polygon's distance exceeds the gap of its boxes by a share of its size, and at 1e-20 the
absolute 2^-72 of the half-margin, which keeps d2 from underflowing to 0, is 2^12 times 2^-18 C.  So the rectangles get 70 % of the
pairs.)"""
import importlib.util
import os

import numpy as np
import pytest

import distance_ref
import near_broad_ref as ref
import test_poly_broad_margin_cpu as base

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("poly_near_box", os.path.join(HERE, "tools", "poly_near_box.py"))
pnb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pnb)
F32, F64 = np.float32, np.float64
SCALES = [1e-20, 1e-6, 1.0, 1e4, 1e15]
MARGINS = ["zero", "1e-30", "ulp", "tenth", "one", "hundred"]
KINDS = base.KINDS + ["rect"]
N_PER_COMBO = 300                  # pairs per (scale, margin, family of A); the rectangles get RECT_SHARE times as many
RECT_SHARE = 14
MIN_DISJOINT, MIN_NEAR = 1 / 3, 1 / 3


def margin_of(name, scale):
    """the margin as the float the call would get; a polygon size is `scale`, C about 2 scale"""
    return F32({"zero": 0.0, "1e-30": 1e-30 * scale, "ulp": float(np.spacing(F32(2 * scale))), "tenth": 0.1 * scale, "one": scale, "hundred": 100 * scale}[name])


def polygons(rng, n, kind, scale):
    if kind != "rect":
        return base.polygons(rng, n, kind, scale)
    w, h = rng.uniform(0.05, 1, (2, n)) * scale
    cx, cy = rng.uniform(-1, 1, (2, n)) * scale
    vx, vy = np.full((16, n), np.nan), np.full((16, n), np.nan)
    vx[:4], vy[:4] = [cx - w, cx + w, cx + w, cx - w], [cy - h, cy - h, cy + h, cy + h]
    return vx.astype(F32), vy.astype(F32), np.full(n, 4, np.uint8)


def push_rects(a, box_a, box_b, b, rng):
    """rectangles b translated so that b's box starts 0 to a few ulps past (or ends in front of) a's box along one axis, with b's
    centre inside a's own extent along the other (four in five: face to face), or along both axes (vertex to vertex on the diagonal);
    half of them moved by up to +-4 ulps per coordinate, so that the boxes lie from a few ulps inside to a few ulps beyond touching"""
    vx, vy, k = b
    n = vx.shape[1]
    diag = rng.random(n) < 0.2
    along_x = rng.random(n) < 0.5
    flip = rng.random((2, n)) < 0.5
    gap_rel = rng.choice([0.0, 1e-7, 2e-7, 3e-7, 4e-7], n)
    moves = []
    for axis, (va, vb) in enumerate(((a[0], vx), (a[1], vy))):
        lo, hi = box_a[axis].astype(F64), box_a[axis + 2].astype(F64)
        past = np.where(flip[axis], (lo - box_b[axis + 2]) * (1 + gap_rel) - np.abs(lo) * gap_rel, (hi - box_b[axis]) * (1 + gap_rel) + np.abs(hi) * gap_rel)
        ca, ha = 0.5 * (va[0].astype(F64) + va[2]), 0.5 * np.abs(va[2].astype(F64) - va[0])
        inside = ca + rng.uniform(-1, 1, n) * ha - 0.5 * (vb[0].astype(F64) + vb[2])
        moves.append(np.where(diag | (along_x == (axis == 0)), past, inside))
    jitter = np.where(rng.random(n) < 0.5, 0.0, rng.integers(-4, 5, (16, n)) * 2.0 ** -24)
    return ((vx.astype(F64) + moves[0]) * (1 + jitter)).astype(F32), ((vy.astype(F64) + moves[1]) * (1 + jitter)).astype(F32), k


def adversarial_pairs(rng, n, kind_a, kind_b, scale, r):
    """(a, b, box_a, box_b, regular): b pushed so that its box starts just past a's (polygons: base.push_beyond; rectangles: push_rects)"""
    a, b = polygons(rng, n, kind_a, scale), polygons(rng, n, kind_b, scale)
    box_a, ok_a = pnb.poly_near_boxes(*a, r)
    box_b, _ = pnb.poly_near_boxes(*b, r)
    b = push_rects(a, box_a, box_b, b, rng) if kind_a == "rect" else base.push_beyond(box_a, box_b, b, rng)
    box_b, ok_b = pnb.poly_near_boxes(*b, r)
    return a, b, box_a, box_b, ok_a & ok_b


def run_scale(scale, seed):
    """(pairs, box-disjoint, near) over every margin and family at one scale; asserts that no box-disjoint pair is listed"""
    rng = np.random.default_rng(seed)
    total = tested = near = 0
    for m in MARGINS:
        r = margin_of(m, scale)
        for ia, ka in enumerate(KINDS):
            kb = "rect" if ka == "rect" else base.KINDS[(ia + (MARGINS.index(m) % 3) * 2) % 6]
            n = N_PER_COMBO * (RECT_SHARE if ka == "rect" else 1)
            a, b, box_a, box_b, keep = adversarial_pairs(rng, n, ka, kb, scale, r)
            sel = np.flatnonzero(keep & pnb.disjoint(box_a, box_b))
            rec = distance_ref.poly_distances(a, b, sel, sel)
            bad = np.flatnonzero(ref.listed(rec, r))
            assert bad.size == 0, (f"{ka} / {kb} at scale {scale}, margin {m} = {r}: pair {sel[bad[0]]} is listed with disjoint boxes: {rec[bad[0]]}, "
                                   f"boxes {box_a[:, sel[bad[0]]]} {box_b[:, sel[bad[0]]]}")
            c = np.maximum(np.nanmax(np.abs(a[0][:, sel]), 0), np.nanmax(np.abs(b[0][:, sel]), 0))
            c = np.maximum(c, np.maximum(np.nanmax(np.abs(a[1][:, sel]), 0), np.nanmax(np.abs(b[1][:, sel]), 0))).astype(F64)
            total, tested = total + n, tested + sel.size
            near += int((rec["dist"].astype(F64) <= float(r) * (1 + 2.0 ** -18) + 2.0 ** -18 * c).sum())
    return total, tested, near


def test_disjoint_boxes_are_never_listed():
    total = tested = near = 0
    for q, scale in enumerate(SCALES):
        t, d, c = run_scale(scale, 2000 + q)
        print(f"scale {scale}: {t} pairs, {d} box-disjoint ({d / t:.3f}), {c} of those within the margin's 2^-18 ({c / max(d, 1):.3f})")
        total, tested, near = total + t, tested + d, near + c
    print(f"all scales: {total} pairs, box-disjoint {tested / total:.3f}, of those near {near / tested:.3f}")
    assert tested >= MIN_DISJOINT * total and near >= MIN_NEAR * tested, (total, tested, near)


def test_wild_rule_and_containment():
    """what §5.10 calls wild and a polygon below 2^-100 are not regular; an ordinary polygon's box contains §5.10's box and its live
    vertices widened by at least max_dist / 2, grows with max_dist, and -0 is 0"""
    rng = np.random.default_rng(13)
    vx, vy, k = base.polygons(rng, 2000, "irregular", 3.0)
    static, _ = base.pbb.poly_broad_boxes(vx, vy, k)
    last = static
    for r in (0.0, 0.25, 3.0, 300.0):
        box, ok = pnb.poly_near_boxes(vx, vy, k, r)
        assert ok.all()
        assert (box[:2] <= last[:2]).all() and (box[2:] >= last[2:]).all()
        assert (box[0] <= np.nanmin(vx, 0) - r / 2).all() and (box[2] >= np.nanmax(vx, 0) + r / 2).all()
        assert (box[1] <= np.nanmin(vy, 0) - r / 2).all() and (box[3] >= np.nanmax(vy, 0) + r / 2).all()
        last = box
    assert np.array_equal(pnb.poly_near_boxes(vx, vy, k, -0.0)[0], pnb.poly_near_boxes(vx, vy, k, 0.0)[0])
    bx, by, bk = vx[:, :9].copy(), vy[:, :9].copy(), k[:9].copy()
    bx[1, 0] = np.nan
    by[0, 1] = np.inf
    bx[:, 2] *= F32(2.0 ** 61)
    bk[3] = 2
    t = np.linspace(0, 1, 16, dtype=F32)
    bx[:, 4], by[:, 4] = t, F32(2) * t                   # every vertex on one line
    bk[5], bk[6] = 0, 17
    bx[:, 7], by[:, 7] = bx[:, 7] * F32(2.0 ** -103), by[:, 7] * F32(2.0 ** -103)     # below 2^-100
    _, ok = pnb.poly_near_boxes(bx, by, bk, 1.0)
    assert not ok[:8].any() and ok[8]
