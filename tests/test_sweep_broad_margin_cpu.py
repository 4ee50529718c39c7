"""CPU check of the swept broad phase's box rule, independent of the kernel: the numpy restatement of
poly_sweep_box (tests/tools/poly_sweep_box.py, which holds the proof's constants) and the sweep contract's restatement
(tests/sweep_ref.py) on adversarial pairs.  Whenever the SWEPT boxes of two regular polygons are disjoint, the pair's sweep record
must have hit == 0 — for the polygon families of test_poly_broad_margin_cpu.py at scales from 1e-20 to 1e15, seven motion families,
and the second polygon pushed so that its swept box lies 0 to a few ulps beyond the first one's on each side."""
import importlib.util
import os

import numpy as np
import pytest

import sweep_ref
import test_poly_broad_margin_cpu as base

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("poly_sweep_box", os.path.join(HERE, "tools", "poly_sweep_box.py"))
psb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(psb)
F32, F64 = np.float32, np.float64
N_PER_COMBO = 6_000                # pairs per combination of two polygon families: 18 combinations per scale, 7 motion families in each
MOTIONS = ["zero", "equal", "tiny", "parallel", "head_on", "far", "one_at_rest"]
MIN_DISJOINT, MIN_CLOSE = 0.5, 0.2


def motions(rng, a, b, scale):
    """(a_motion, b_motion, family i32[n]): each pair draws one of the seven families"""
    n = a[0].shape[1]
    fam = rng.integers(0, len(MOTIONS), n)
    ang = rng.uniform(0, 2 * np.pi, (2, n))
    mag = rng.uniform(0.1, 3.0, (2, n)) * scale
    da = np.stack([mag[0] * np.cos(ang[0]), mag[0] * np.sin(ang[0])])
    db = np.stack([mag[1] * np.cos(ang[1]), mag[1] * np.sin(ang[1])])
    zero = np.zeros((2, n))
    far = 1e3 * rng.uniform(0.1, 1.0, (2, n)) * scale                     # 1e3 polygon sizes; at 1e15 still below 2^60
    far_a = np.stack([far[0] * np.cos(ang[0]), far[0] * np.sin(ang[0])])
    far_b = np.stack([far[1] * np.cos(ang[1]), far[1] * np.sin(ang[1])])
    # parallel: the relative motion runs along edge 0 or 1 of A or of B, turned by up to 1e-7 rad, so that v cancels on that edge's axis
    src = np.where(rng.random(n) < 0.5, 0, 1)
    e = rng.integers(0, 2, n)
    cols = np.arange(n)
    vx = np.where(src == 0, a[0][(e + 1), cols].astype(F64) - a[0][e, cols], b[0][(e + 1), cols].astype(F64) - b[0][e, cols])
    vy = np.where(src == 0, a[1][(e + 1), cols].astype(F64) - a[1][e, cols], b[1][(e + 1), cols].astype(F64) - b[1][e, cols])
    ln = np.maximum(np.hypot(vx, vy), 1e-300)
    turn = rng.uniform(-1e-7, 1e-7, n) * rng.integers(0, 2, n)          # half of them exactly along the edge (up to rounding)
    ca, sa = np.cos(turn), np.sin(turn)
    par = np.stack([(ca * vx - sa * vy) / ln, (sa * vx + ca * vy) / ln]) * mag[0] * rng.choice([-1.0, 1.0], n)
    compass = rng.integers(0, 8, n) * (np.pi / 4)
    head = np.stack([np.cos(compass), np.sin(compass)]) * mag[0]
    head[np.abs(head) < 1e-9 * scale] = 0.0
    share = rng.random(n)                                                 # how a relative motion is split between the two sets
    out_a, out_b = np.zeros((2, n)), np.zeros((2, n))
    for f, (ma, mb) in enumerate([(zero, zero), (da, da), (da * 1e-30, db * 1e-30), (da - par * share, da + par * (1 - share)),
                                  (-head * share, head * (1 - share)), (far_a, far_b), (zero, db)]):
        out_a, out_b = np.where(fam == f, ma, out_a), np.where(fam == f, mb, out_b)
    swap = (fam == 6) & (rng.random(n) < 0.5)                             # one set at rest: either one
    out_a, out_b = np.where(swap, out_b, out_a), np.where(swap, out_a, out_b)
    return (out_a[0].astype(F32), out_a[1].astype(F32)), (out_b[0].astype(F32), out_b[1].astype(F32)), fam


def adversarial_pairs(rng, n, kind_a, kind_b, scale):
    """(a, b, a_motion, b_motion, box_a, box_b, regular, family): b pushed so that its swept box starts just past a's"""
    a = base.polygons(rng, n, kind_a, scale)
    b = base.polygons(rng, n, kind_b, scale)
    ma, mb, fam = motions(rng, a, b, scale)
    box_a, ok_a = psb.poly_sweep_boxes(*a, ma)
    box_b, _ = psb.poly_sweep_boxes(*b, mb)
    b = base.push_beyond(box_a, box_b, b, rng)
    box_b, ok_b = psb.poly_sweep_boxes(*b, mb)
    return a, b, ma, mb, box_a, box_b, ok_a & ok_b, fam


def disjoint(box_a, box_b):
    return (box_a[2] < box_b[0]) | (box_b[2] < box_a[0]) | (box_a[3] < box_b[1]) | (box_b[3] < box_a[1])


@pytest.mark.parametrize("scale", [1e-20, 1e-6, 1.0, 1e4, 1e15])
def test_disjoint_swept_boxes_never_hit(scale):
    rng = np.random.default_rng(int(np.log10(scale)) + 1900)
    n = N_PER_COMBO
    tested = close = total = 0
    per_family = np.zeros(len(MOTIONS), np.int64)
    for ia, ka in enumerate(base.KINDS):
        for kb in (base.KINDS[ia], base.KINDS[(ia + 1) % 6], base.KINDS[(ia + 3) % 6]):
            a, b, ma, mb, box_a, box_b, keep, fam = adversarial_pairs(rng, n, ka, kb, scale)
            sel = np.flatnonzero(keep & disjoint(box_a, box_b))
            rec = sweep_ref.poly_sweeps(a, b, sel, sel, ma, mb)
            bad = np.flatnonzero(rec["hit"] != 0)
            assert bad.size == 0, (f"{ka} / {kb} at scale {scale}: pair {sel[bad[0]]} ({MOTIONS[fam[sel[bad[0]]]]}) is hit "
                                   f"with disjoint swept boxes: {rec[bad[0]]}")
            total += n
            tested += sel.size
            per_family += np.bincount(fam[sel], minlength=len(MOTIONS))
            gap = np.maximum(np.maximum(box_b[0] - box_a[2], box_a[0] - box_b[2]), np.maximum(box_b[1] - box_a[3], box_a[1] - box_b[3]))[sel]
            size = scale + np.abs(box_a[:, sel].astype(F64)).max(0)      # a far motion carries the box to 1e3 scales: ulps grow with it
            close += int((gap.astype(F64) <= 4e-5 * size).sum())
    print(f"scale {scale}: {total} pairs, {tested} swept-box-disjoint, {close} of those within 4e-5 of touching, per motion family {per_family.tolist()}")
    # what the generator yields here (on the box rule and the reference alone): 61 to 62 % of the pairs are swept-box-disjoint and reach
    # the reference, 54 to 61 % of those nearly touch; each motion family holds 12 to 16 % of the tested pairs
    assert tested > MIN_DISJOINT * total and close > MIN_CLOSE * tested, (total, tested, close)
    assert (per_family > 0.25 * tested / len(MOTIONS)).all(), per_family


def test_wild_rule():
    """non-finite or huge motions, a displaced coordinate beyond 2^60, fewer than three vertices, collinear polygons and counts out of
    range are not regular; ordinary moving polygons are, and their box contains every real vertex at t = 0 and at t = 1"""
    rng = np.random.default_rng(11)
    vx, vy, k = base.polygons(rng, 2000, "irregular", 3.0)
    dx, dy = rng.uniform(-5, 5, 2000).astype(F32), rng.uniform(-5, 5, 2000).astype(F32)
    box, ok = psb.poly_sweep_boxes(vx, vy, k, (dx, dy))
    assert ok.all()
    for tx, ty in ((0, 0), (dx.astype(F64), dy.astype(F64))):
        assert (box[0] <= np.nanmin(vx + tx, 0)).all() and (box[2] >= np.nanmax(vx + tx, 0)).all()
        assert (box[1] <= np.nanmin(vy + ty, 0)).all() and (box[3] >= np.nanmax(vy + ty, 0)).all()
    still, ok0 = psb.poly_sweep_boxes(vx, vy, k, None)                  # at rest the box contains §5.10's (its widening is not smaller)
    static, _ = base.pbb.poly_broad_boxes(vx, vy, k)
    assert ok0.all() and (still[:2] <= static[:2]).all() and (still[2:] >= static[2:]).all()
    assert (box[:2] <= still[:2]).all() and (box[2:] >= still[2:]).all()
    bx, by, bk = vx[:, :12].copy(), vy[:, :12].copy(), k[:12].copy()
    mx, my = dx[:12].copy(), dy[:12].copy()
    mx[0] = np.nan
    my[1] = np.inf
    mx[2] = F32(-np.inf)
    my[3] = F32(2.0 ** 60)
    mx[4] = F32(-2.0 ** 61)
    bx[:, 5], by[:, 5] = bx[:, 5] * F32(2.0 ** 54) + F32(2.0 ** 58), by[:, 5] * F32(2.0 ** 54)   # |coordinate| < 2^59 ...
    mx[5] = F32(2.0 ** 59.9)                                             # ... |motion| < 2^60, and displaced beyond 2^60
    bk[6] = 2
    t = np.linspace(0, 1, 16, dtype=F32)
    bx[:, 7], by[:, 7] = t, F32(2) * t                                   # every vertex on one line
    bk[8], bk[9] = 0, 17
    bx[1, 10] = np.nan
    _, ok = psb.poly_sweep_boxes(bx, by, bk, (mx, my))
    assert not ok[:11].any() and ok[11]
    mx[5] = F32(-2.0 ** 59)                                              # the same polygon moving back towards the origin is regular
    _, ok = psb.poly_sweep_boxes(bx, by, bk, (mx, my))
    assert ok[5]
