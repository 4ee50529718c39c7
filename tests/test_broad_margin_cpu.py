"""CPU check of the broad phase's box rule, independent of the kernel: a numpy restatement of broad_box
(csrc/c2d_broad.hip) and the CPU oracle on adversarial pairs.  Whenever the boxes of two regular objects are disjoint, the
reference's test must report "no collision" — for rectangles, sheared parallelograms, kites with an acute angle between
edges 0 and 1, bow-ties and random quads, at scales from 1e-20 to 1e15, with the second object pushed to within a few ulps of
the first one's box."""
import numpy as np
import pytest

F32, F64 = np.float32, np.float64


def broad_boxes(r):
    """r f32[8][n] -> (box f32[4][n] = minx, miny, maxx, maxy; regular bool[n]), the rule of broad_box"""
    r = np.asarray(r, F32)
    n = r.shape[1]
    with np.errstate(all="ignore"):
        finite = np.isfinite(r).all(0)
        cmax = np.abs(np.where(np.isfinite(r), r, 0)).max(0).astype(F64)
        ok = finite & (cmax < 2.0 ** 60)
        ax = [(r[2] - r[0]).astype(F64), (r[4] - r[2]).astype(F64)]
        ay = [(r[3] - r[1]).astype(F64), (r[5] - r[3]).astype(F64)]
        slo, shi = [], []
        for i in range(2):
            n1 = np.abs(ax[i]) + np.abs(ay[i])
            ok &= n1 >= 2.0 ** -80
            p = np.stack([ax[i] * r[2 * v].astype(F64) + ay[i] * r[2 * v + 1].astype(F64) for v in range(4)])
            w = n1 * (2.0 ** -21 * cmax + 2.0 ** -66) + 2.0 ** -140
            slo.append(p.min(0) - w)
            shi.append(p.max(0) + w)
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
    assert box.shape == (4, n)
    return box, ok


def quads(rng, n, kind, scale):
    """f32[8][n] quads of one family around the origin, size ~ scale"""
    c = rng.uniform(-1, 1, (2, n)) * scale
    th = rng.uniform(0, 2 * np.pi, n)
    u = np.stack([np.cos(th), np.sin(th)])
    v = np.stack([-u[1], u[0]])
    w, h = rng.uniform(0.05, 1, n) * scale, rng.uniform(0.05, 1, n) * scale
    if kind == "rect":
        p = [c - w * u - h * v, c + w * u - h * v, c + w * u + h * v, c - w * u + h * v]
    elif kind == "sheared":   # parallelogram with an angle of 1e-3 .. 0.3 rad between edges 0 and 1
        ang = np.exp(rng.uniform(np.log(1e-3), np.log(0.3), n))
        e1 = np.stack([np.cos(th + ang), np.sin(th + ang)]) * h
        p0 = c - w * u
        p = [p0, p0 + 2 * w * u, p0 + 2 * w * u + e1, p0 + e1]
    elif kind == "kite":      # acute angle at vertex 1 between edge 0 and edge 1
        ang = np.exp(rng.uniform(np.log(1e-3), np.log(0.5), n))
        p1 = c + w * u
        p = [c - w * u, p1, p1 - 2 * w * np.stack([np.cos(th + ang), np.sin(th + ang)]), c + h * v]
    elif kind == "bowtie":
        p = [c - w * u - h * v, c + w * u + h * v, c + w * u - h * v, c - w * u + h * v]
    else:                     # four random points
        p = [c + rng.uniform(-1, 1, (2, n)) * scale for _ in range(4)]
    if kind != "bowtie" and rng.random() < 0.5:
        p = p[::-1]           # reversed winding
    return np.stack([p[k // 2][k % 2] for k in range(8)]).astype(F32)


def push_beyond(box_a, box_b, b, rng):
    """b translated so that its box starts just past box_a's edge (right, top or diagonally), by 0 to a few ulps or a few parts
    in 1e7; returns the moved quads (float32)"""
    n = b.shape[1]
    side = rng.integers(0, 3, n)
    gap_rel = rng.choice([0.0, 1e-7, 3e-7, 1e-6, 1e-5], n)
    dx = (box_a[2].astype(F64) - box_b[0].astype(F64)) * (1 + gap_rel) + np.abs(box_a[2]).astype(F64) * gap_rel
    dy = (box_a[3].astype(F64) - box_b[1].astype(F64)) * (1 + gap_rel) + np.abs(box_a[3]).astype(F64) * gap_rel
    dx = np.where(side == 1, rng.uniform(-1, 1, n) * (box_a[2] - box_a[0]), dx)
    dy = np.where(side == 0, rng.uniform(-1, 1, n) * (box_a[3] - box_a[1]), dy)
    out = b.astype(F64).copy()
    out[0::2] += dx
    out[1::2] += dy
    jitter = np.where(rng.random(n) < 0.5, 0.0, rng.integers(-4, 5, (8, n)) * 2.0 ** -24)   # +-4 ulps on half of them
    return (out * (1 + jitter)).astype(F32)


@pytest.mark.parametrize("scale", [1e-20, 1e-6, 1.0, 1e4, 1e15])
def test_disjoint_boxes_never_collide(oracle, scale):
    rng = np.random.default_rng(int(np.log10(scale)) + 100)
    kinds = ["rect", "sheared", "kite", "bowtie", "random"]
    n = 120_000
    tested = close = 0
    for ka in kinds:
        for kb in kinds:
            a = quads(rng, n, ka, scale)
            b = quads(rng, n, kb, scale)
            box_a, ok_a = broad_boxes(a)
            box_b, _ = broad_boxes(b)
            b = push_beyond(box_a, box_b, b, rng)
            box_b, ok_b = broad_boxes(b)
            keep = ok_a & ok_b
            disjoint = keep & ((box_a[2] < box_b[0]) | (box_b[2] < box_a[0]) | (box_a[3] < box_b[1]) | (box_b[3] < box_a[1]))
            sel = np.flatnonzero(disjoint)
            res, _ = oracle.sat_rect_pairs_verts(np.concatenate([a[:, sel], b[:, sel]]))
            bad = np.flatnonzero(res)
            assert bad.size == 0, f"{ka} / {kb} at scale {scale}: pair {sel[bad[0]]} collides with disjoint boxes"
            tested += sel.size
            gap = np.maximum(box_b[0] - box_a[2], box_b[1] - box_a[3])[sel].astype(F64)
            close += int((gap <= 1e-5 * scale * 4).sum())
    # 3 million pairs per scale, of which about 1.5 million have disjoint boxes and reach the oracle (7.7 million over the five scales)
    assert tested > 1_400_000 and close > 300_000, (tested, close)


def test_wild_rule():
    """non-finite, |coordinate| >= 2^60, zero-length or parallel first axes are wild; ordinary rectangles are not, and their
    box contains every vertex"""
    rng = np.random.default_rng(7)
    r = quads(rng, 1000, "rect", 3.0)
    box, ok = broad_boxes(r)
    assert ok.all()
    assert (box[0] <= r[0::2].min(0)).all() and (box[2] >= r[0::2].max(0)).all()
    assert (box[1] <= r[1::2].min(0)).all() and (box[3] >= r[1::2].max(0)).all()
    bad = r[:, :6].copy()
    bad[3, 0] = np.nan
    bad[6, 1] = np.inf
    bad[:, 2] *= F32(2.0 ** 61)
    bad[2:4, 3] = bad[0:2, 3]                 # edge 0 of zero length
    bad[:, 4] = [0, 0, 1, 2, 2, 4, 0, 5]       # edge 1 parallel to edge 0 (collinear first three vertices)
    _, ok = broad_boxes(bad)
    assert not ok[:5].any() and ok[5]
