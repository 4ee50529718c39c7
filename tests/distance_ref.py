"""CPU restatement of the distance contract of include/c2d.h (c2d_poly_pair_distances / c2d_rect_pair_distances), written from the
contract, not from the kernel: plain numpy float32, element-wise and unfused (numpy never contracts a * b + c), / and np.sqrt (both
correctly rounded) and the sequential pick: candidates in the order side, edge, vertex; the first usable candidate is the first
best, a later one replaces it only under strict d2 < best.

poly_distances(a, b, i, j) and rect_distances(a, b, i, j) take LOCAL indices (the list entry minus its bases) and return a
DISTANCE_DT record per pair.  The sets are loaded as tests/contact_ref.py loads them, and `hit` and the BAD_PAIR entries are
contact_ref's own (the contract: "exactly the hit of the contact calls")."""
import numpy as np

import contact_ref as cref

DISTANCE_DT = np.dtype([("dist", "<f4"), ("ax", "<f4"), ("ay", "<f4"), ("bx", "<f4"), ("by", "<f4"), ("edge", "<u2"), ("vert", "<u2"), ("hit", "u1"),
                        ("flags", "u1"), ("reserved0", "<u2"), ("reserved1", "<u4")])
EDGE_ON_B, INTERIOR, NO_CANDIDATE, BAD_PAIR = 1, 2, 4, 8
NONE = 0xFFFF
F = np.float32
FLOATS = ("dist", "ax", "ay", "bx", "by")


class _Pick:
    """the sequential pick over the candidates of a batch of pairs"""

    def __init__(self, m):
        self.best = np.full(m, np.inf, F)
        self.cx, self.cy, self.px, self.py = (np.zeros(m, F) for _ in range(4))
        self.side, self.edge, self.vert = (np.full(m, -1, np.int64) for _ in range(3))
        self.interior = np.zeros(m, bool)

    def side_of(self, side, px, py, kp, qx, qy, kq):
        """edges of P (x, y f32 [rows_p][m], kp real vertices per pair) against the vertices of Q, in the order e, v"""
        cols = np.arange(px.shape[1])
        for e in range(px.shape[0]):
            live_e = e < kp
            e0, e1 = np.where(live_e, e, 0), np.where(e + 1 < kp, e + 1, 0)          # the vertex index wraps at k
            x0, y0, x1, y1 = px[e0, cols], py[e0, cols], px[e1, cols], py[e1, cols]
            ex, ey = x1 - x0, y1 - y0
            len2 = ex * ex + ey * ey
            ux, uy = qx - x0, qy - y0                                                # [rows_q][m]: every vertex of Q at once
            s = ux * ex + uy * ey
            r0 = s <= 0
            r1 = ~r0 & (s >= len2)
            t = s / len2
            cx = np.where(r0, x0, np.where(r1, x1, x0 + t * ex))
            cy = np.where(r0, y0, np.where(r1, y1, y0 + t * ey))
            dx, dy = qx - cx, qy - cy
            d2 = dx * dx + dy * dy
            for v in range(qx.shape[0]):
                take = live_e & (v < kq) & ~np.isnan(d2[v]) & ((self.side < 0) | (d2[v] < self.best))
                self.best = np.where(take, d2[v], self.best)
                self.cx, self.cy = np.where(take, cx[v], self.cx), np.where(take, cy[v], self.cy)
                self.px, self.py = np.where(take, qx[v], self.px), np.where(take, qy[v], self.py)
                self.side, self.edge, self.vert = np.where(take, side, self.side), np.where(take, e, self.edge), np.where(take, v, self.vert)
                self.interior = np.where(take, ~r0[v] & ~r1[v], self.interior)

    def records(self, hit, bad):
        out = np.zeros(len(self.best), DISTANCE_DT)
        none, on_b = self.side < 0, self.side == 1
        out["dist"] = np.where(none, F(np.inf), np.sqrt(self.best))
        out["ax"], out["ay"] = np.where(on_b, self.px, self.cx), np.where(on_b, self.py, self.cy)
        out["bx"], out["by"] = np.where(on_b, self.cx, self.px), np.where(on_b, self.cy, self.py)
        out["edge"], out["vert"] = np.where(none, NONE, self.edge), np.where(none, NONE, self.vert)
        out["flags"] = np.where(none, NO_CANDIDATE, np.where(on_b, EDGE_ON_B, 0) | np.where(self.interior, INTERIOR, 0))
        out[hit == 1] = (0.0, 0.0, 0.0, 0.0, 0.0, NONE, NONE, 1, 0, 0, 0)
        out[bad] = (0.0, 0.0, 0.0, 0.0, 0.0, NONE, NONE, 0, BAD_PAIR, 0, 0)
        return out


def _run(ax, ay, ka, bx, by, kb, contacts):
    bad = (contacts["flags"] & cref.BAD_PAIR) != 0
    pick = _Pick(len(contacts))
    with np.errstate(all="ignore"):
        pick.side_of(0, ax, ay, ka, bx, by, kb)
        pick.side_of(1, bx, by, kb, ax, ay, ka)
    return pick.records(contacts["hit"], bad)


def poly_distances(a, b, i, j):
    """a, b: (vx f32[rows][n], vy, k u8[n] or None); i, j: local indices of the pairs -> DISTANCE_DT[len(i)]"""
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    contacts = cref.poly_contacts(a, b, i, j)
    bad = (contacts["flags"] & cref.BAD_PAIR) != 0
    if bad.all():           # (an empty set among them)
        return _Pick(len(i)).records(contacts["hit"], bad)
    ii, jj = np.where(bad, 0, i), np.where(bad, 0, j)
    ka, kb = np.where(bad, 1, cref._counts(a)[ii]), np.where(bad, 1, cref._counts(b)[jj])
    ax, ay = np.asarray(a[0], F)[:, ii], np.asarray(a[1], F)[:, ii]
    bx, by = np.asarray(b[0], F)[:, jj], np.asarray(b[1], F)[:, jj]
    return _run(ax, ay, ka, bx, by, kb, contacts)


def rect_distances(a, b, i, j):
    """a f32[8][n_a], b f32[8][n_b] (planes x0, y0, ..., x3, y3); i, j: local indices of the pairs -> DISTANCE_DT[len(i)]"""
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    a, b = np.asarray(a, F), np.asarray(b, F)
    contacts = cref.rect_contacts(a, b, i, j)
    bad = (contacts["flags"] & cref.BAD_PAIR) != 0
    if bad.all():
        return _Pick(len(i)).records(contacts["hit"], bad)
    r1, r2 = a[:, np.where(bad, 0, i)], b[:, np.where(bad, 0, j)]
    four = np.full(len(i), 4, np.int64)
    return _run(r1[0::2], r1[1::2], four, r2[0::2], r2[1::2], four, contacts)


def same(got, want):
    """every field equal; the five floats bit for bit, except that +0 and -0 are equal"""
    ok = np.ones(len(want), bool)
    for f in FLOATS:
        g, w = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        ok &= (g.view(np.uint32) == w.view(np.uint32)) | ((g == 0) & (w == 0))
    for f in ("edge", "vert", "hit", "flags", "reserved0", "reserved1"):
        ok &= got[f] == want[f]
    return ok
