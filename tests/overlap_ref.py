"""CPU restatement of the overlap contract of include/c2d.h (c2d_poly_pair_overlaps / c2d_rect_pair_overlaps), written from the
contract, not from the kernel: plain numpy float32, element-wise and unfused (numpy never contracts a * b + c), / correctly rounded,
every max and min a compare and select (np.where), so that a NaN falls through each compare as the contract says.  The rule is a
boundary integral: each edge of A is clipped to the part inside B, each edge of B to the part inside A, and the pieces are summed;
the intersection polygon is never built.  Where an edge is cut, the crossing is one point for both sides (A's p0 + t * e); two
edges within 8 u D of one line are told apart by the ends of A's edge against B's half-plane, from the same bits on both sides.

poly_overlaps(a, b, i, j) and rect_overlaps(a, b, i, j) take LOCAL indices (the list entry minus its bases) and return an OVERLAP_DT
record per pair.  The sets are loaded as tests/contact_ref.py loads them, and `hit` and the BAD_PAIR entries are contact_ref's own
(the contract: "exactly the hit of the contact calls")."""
import numpy as np

import contact_ref as cref

OVERLAP_DT = np.dtype([("area", "<f4"), ("iou", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("area_a", "<f4"), ("area_b", "<f4"), ("hit", "u1"), ("flags", "u1"),
                       ("pieces_a", "u1"), ("pieces_b", "u1"), ("reserved", "<u4")])
DEGENERATE, CLAMPED, NO_CENTROID, BAD_PAIR = 1, 2, 4, 8
F = np.float32
FLOATS = ("area", "iou", "cx", "cy", "area_a", "area_b")
ON_LINE = F(2.0 ** -21)        # 8 u: two edges count as lying on one line within 8 u D (|x| + |y|) of each cross product
QUIET_NAN = np.array([0x7FC00000], np.uint32).view(F)[0]


def _cross(ux, uy, vx, vy):
    return ux * vy - uy * vx


def _vertex(x, y, idx):
    cols = np.arange(x.shape[1])
    return x[idx, cols], y[idx, cols]


def _shoelace(x, y, k):
    """cross(v_0, v_1) + ... + cross(v_k-1, v_0), from 0 in that order"""
    total = np.zeros(x.shape[1], F)
    for i in range(x.shape[0]):
        x0, y0 = _vertex(x, y, np.where(i < k, i, 0))
        x1, y1 = _vertex(x, y, np.where(i + 1 < k, i + 1, 0))
        total = np.where(i < k, total + _cross(x0, y0, x1, y1), total)
    return total


def _extent(ax, ay, ka, bx, by, kb):
    """D: the largest |coordinate| of the shifted real slots, A's slots in order (x, then y), then B's; a compare and select"""
    D = np.zeros(ax.shape[1], F)
    for x, y, k in ((ax, ay, ka), (bx, by, kb)):
        for v in range(x.shape[0]):
            for c in (np.abs(x[v]), np.abs(y[v])):
                D = np.where((v < k) & (c > D), c, D)
    return D


def _side(px, py, kp, sp, qx, qy, kq, sq, side0, kD):
    """the kp edges of P (x, y f32 [rows_p][m]), each clipped by the kq edges of Q -> S, Mx, My, pieces of this side"""
    m = px.shape[1]
    S, Mx, My = (np.zeros(m, F) for _ in range(3))
    pieces = np.zeros(m, np.int64)
    edges = []          # Q's edges in order: q0, q1, g and whether the edge imposes anything
    for f in range(qx.shape[0]):
        a0, b0 = _vertex(qx, qy, np.where(f < kq, f, 0))
        a1, b1 = _vertex(qx, qy, np.where(f + 1 < kq, f + 1, 0))
        gx, gy = a1 - a0, b1 - b0
        edges.append((a0, b0, a1, b1, gx, gy, (f < kq) & ~((gx == 0) & (gy == 0))))
    for e in range(px.shape[0]):
        live_e = e < kp
        x0, y0 = _vertex(px, py, np.where(live_e, e, 0))
        x1, y1 = _vertex(px, py, np.where(e + 1 < kp, e + 1, 0))
        ex, ey = x1 - x0, y1 - y0
        tol_e = kD * (np.abs(ex) + np.abs(ey))
        t0, t1 = np.zeros(m, F), np.ones(m, F)
        ux, uy, vx, vy = x0, y0, x1, y1
        alive = np.ones(m, bool)
        for a0, b0, a1, b1, gx, gy, real in edges:
            tol_g = kD * (np.abs(gx) + np.abs(gy))
            c_p0 = _cross(gx, gy, x0 - a0, y0 - b0)
            c_p1 = _cross(gx, gy, x1 - a0, y1 - b0)
            c_q0 = _cross(ex, ey, a0 - x0, b0 - y0)
            c_q1 = _cross(ex, ey, a1 - x0, b1 - y0)
            on_line = real & (np.abs(c_p0) <= tol_g) & (np.abs(c_p1) <= tol_g) & (np.abs(c_q0) <= tol_e) & (np.abs(c_q1) <= tol_e)
            same_way = (sp * sq) * (ex * gx + ey * gy) > 0
            # two edges that cross: the half-plane of g cuts e at q, and the crossing is ONE point for both sides, A's p0 + t * e
            num = sq * c_p0
            den = sq * _cross(gx, gy, ex, ey)
            q = (-num) / den
            if side0:
                cx, cy = x0 + q * ex, y0 + q * ey
            else:           # A's edge is Q's here: the same operations on the same operands as side 0's of this pair of edges
                tq = (-(sp * c_q0)) / (sp * _cross(ex, ey, gx, gy))
                cx, cy = a0 + tq * gx, b0 + tq * gy
            cuts = real & ~on_line
            lower, upper = cuts & (den > 0) & (q > t0), cuts & (den < 0) & (q < t1)
            t0, ux, uy = np.where(lower, q, t0), np.where(lower, cx, ux), np.where(lower, cy, uy)
            t1, vx, vy = np.where(upper, q, t1), np.where(upper, cx, vx), np.where(upper, cy, vy)
            keeps = num > 0
            if side0:
                keeps = keeps | ((num == 0) & same_way)
            alive &= ~(cuts & (den == 0) & ~keeps)
            # two edges on one line: the ends of A's edge against B's half-plane (da, db: the same bits on both sides) say which
            # of the two is the boundary of A and B: A's where it is inside, B's elsewhere, split where A's edge passes through
            if side0:
                da, db = sq * c_p0, sq * c_p1
            else:
                da, db = sp * c_q0, sp * c_q1
            inside = (da >= 0) & (db >= 0)
            outside = ~inside & (da <= 0) & (db <= 0)
            enters, leaves = (da < 0) & (db > 0), (da > 0) & (db < 0)
            ts = da / (da - db)
            if side0:
                sx, sy = x0 + ts * ex, y0 + ts * ey
                s = ts
                from_s, to_s = enters, leaves
                alive &= ~(on_line & ~(same_way & ~outside))
            else:           # B's edge keeps the other part, up to the same point; s is that point's parameter on B's edge
                sx, sy = a0 + ts * gx, b0 + ts * gy
                s = ((sx - x0) * ex + (sy - y0) * ey) / (ex * ex + ey * ey)
                along = (sp * sq) > 0         # (same_way: the two edges run the same way as listed iff the windings agree)
                from_s, to_s = np.where(along, leaves, enters), np.where(along, enters, leaves)
                alive &= ~(on_line & ~(same_way & ~inside))
            lower, upper = on_line & same_way & from_s & (s > t0), on_line & same_way & to_s & (s < t1)
            t0, ux, uy = np.where(lower, s, t0), np.where(lower, sx, ux), np.where(lower, sy, uy)
            t1, vx, vy = np.where(upper, s, t1), np.where(upper, sx, vx), np.where(upper, sy, vy)
        c = sp * _cross(ux, uy, vx, vy)
        piece = live_e & alive & (t0 < t1)
        S = np.where(piece, S + c, S)
        Mx = np.where(piece, Mx + (ux + vx) * c, Mx)
        My = np.where(piece, My + (uy + vy) * c, My)
        pieces += piece
    return S, Mx, My, pieces


def _canonical(v):
    return np.where(np.isnan(v), QUIET_NAN, v)


def _run(ax, ay, ka, bx, by, kb, hit, bad):
    """ax, ay f32[rows_a][m], ka[m] and the same of B; hit u8[m], bad bool[m] -> OVERLAP_DT[m]"""
    m = len(hit)
    out = np.zeros(m, OVERLAP_DT)
    with np.errstate(all="ignore"):
        rx, ry = ax[0].copy(), ay[0].copy()
        ax, ay, bx, by = ax - rx, ay - ry, bx - rx, by - ry
        sum_a, sum_b = _shoelace(ax, ay, ka), _shoelace(bx, by, kb)
        sa, sb = np.where(sum_a > 0, F(1), F(-1)), np.where(sum_b > 0, F(1), F(-1))
        area_a, area_b = F(0.5) * np.abs(sum_a), F(0.5) * np.abs(sum_b)
        kD = ON_LINE * _extent(ax, ay, ka, bx, by, kb)
        S0, Mx0, My0, pa = _side(ax, ay, ka, sa, bx, by, kb, sb, True, kD)
        S1, Mx1, My1, pb = _side(bx, by, kb, sb, ax, ay, ka, sa, False, kD)
        S, Mx, My = S0 + S1, Mx0 + Mx1, My0 + My1
        raw = F(0.5) * S
        lo = np.where(raw > 0, raw, F(0))
        cap = np.where(area_b < area_a, area_b, area_a)
        area = np.where(cap < lo, cap, lo)
        flags = np.where(area == raw, 0, CLAMPED)
        union = (area_a + area_b) - area
        iou = np.where(union > 0, area / union, F(0))
        has_c = S > 0
        s3 = F(3) * S
        cx, cy = np.where(has_c, rx + Mx / s3, F(0)), np.where(has_c, ry + My / s3, F(0))
        flags = flags | np.where(has_c, 0, NO_CENTROID)
        degenerate = ~((sum_a > 0) | (sum_a < 0)) | ~((sum_b > 0) | (sum_b < 0))
    whole = (hit == 1) & ~degenerate
    for name, v in (("area", area), ("iou", iou), ("cx", cx), ("cy", cy)):
        out[name] = np.where(whole, _canonical(v), F(0))
    out["area_a"], out["area_b"] = _canonical(area_a), _canonical(area_b)
    out["hit"] = hit
    out["flags"] = np.where(hit == 0, NO_CENTROID, np.where(degenerate, DEGENERATE | NO_CENTROID, flags))
    out["pieces_a"], out["pieces_b"] = np.where(whole, pa, 0), np.where(whole, pb, 0)
    out[bad] = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, BAD_PAIR, 0, 0, 0)
    return out


def _all_bad(contacts):
    out = np.zeros(len(contacts), OVERLAP_DT)
    out["flags"] = BAD_PAIR
    return out


def poly_overlaps(a, b, i, j):
    """a, b: (vx f32[rows][n], vy, k u8[n] or None); i, j: local indices of the pairs -> OVERLAP_DT[len(i)]"""
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    contacts = cref.poly_contacts(a, b, i, j)
    bad = (contacts["flags"] & cref.BAD_PAIR) != 0
    if bad.all():           # (an empty set among them)
        return _all_bad(contacts)
    ii, jj = np.where(bad, 0, i), np.where(bad, 0, j)
    ka, kb = np.where(bad, 1, cref._counts(a)[ii]), np.where(bad, 1, cref._counts(b)[jj])
    ax, ay = np.asarray(a[0], F)[:, ii], np.asarray(a[1], F)[:, ii]
    bx, by = np.asarray(b[0], F)[:, jj], np.asarray(b[1], F)[:, jj]
    return _run(ax, ay, ka, bx, by, kb, contacts["hit"], bad)


def rect_overlaps(a, b, i, j):
    """a f32[8][n_a], b f32[8][n_b] (planes x0, y0, ..., x3, y3); i, j: local indices of the pairs -> OVERLAP_DT[len(i)]"""
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    a, b = np.asarray(a, F), np.asarray(b, F)
    contacts = cref.rect_contacts(a, b, i, j)
    bad = (contacts["flags"] & cref.BAD_PAIR) != 0
    if bad.all():
        return _all_bad(contacts)
    r1, r2 = a[:, np.where(bad, 0, i)], b[:, np.where(bad, 0, j)]
    four = np.full(len(i), 4, np.int64)
    return _run(r1[0::2], r1[1::2], four, r2[0::2], r2[1::2], four, contacts["hit"], bad)


def same(got, want):
    """byte equality of whole records"""
    g = np.ascontiguousarray(got).view(np.uint8).reshape(-1, OVERLAP_DT.itemsize)
    w = np.ascontiguousarray(want).view(np.uint8).reshape(-1, OVERLAP_DT.itemsize)
    return (g == w).all(axis=1)
