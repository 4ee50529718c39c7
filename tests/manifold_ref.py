"""CPU restatement of the manifold contract of include/c2d.h (c2d_poly_pair_manifolds), written from the contract, not from the
kernel, on top of tests/contact_ref.py: the contact rule (contact_ref._poly_rule) names the winning axis; its raw normal, both
intervals, `pos` and `len` are restated here with contact_ref's own terms (_interval, _axis_terms) and must reproduce the
contact's depth bit for bit (asserted on every call).  Plain numpy float32, element-wise and unfused; compare-and-select for the
deepest vertex (first of equals, a NaN never replaces); / is correctly rounded.

poly_manifolds(a, b, i, j) takes LOCAL indices and returns (CONTACT_DT[len(i)], MANIFOLD_DT[len(i)]); with details=True also a
dict of per-pair intermediates (only meaningful where `live`).  A BAD_PAIR or NO_AXIS contact has the empty manifold."""
import numpy as np

import contact_ref as ref

MANIFOLD_DT = np.dtype([("x0", "<f4"), ("y0", "<f4"), ("d0", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("d1", "<f4"), ("feature", "<u2"), ("count", "u1"),
                        ("flags", "u1"), ("reserved", "<u4")])
REF_IS_B, P0_CLIPPED, P1_CLIPPED, OUTSIDE_SLAB = 1, 2, 4, 8
FEATURE_NONE = 0xFFFF
F = np.float32
FLOATS = ("x0", "y0", "d0", "x1", "y1", "d1")


def empty(m):
    out = np.zeros(m, MANIFOLD_DT)
    out["feature"] = FEATURE_NONE
    return out


def _rows16(v, cols):
    """the columns `cols` of a plane [rows][n] as [16][len(cols)], zeros below (slots at or beyond k are never indexed)"""
    out = np.zeros((16, len(cols)), F)
    out[:v.shape[0]] = np.asarray(v, F)[:, cols]
    return out


def poly_manifolds(a, b, i, j, details=False):
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    rule, bad = ref._poly_rule(a, b, i, j, False)
    contacts = rule.records(bad)
    out = empty(len(i))
    live = ~bad & (contacts["flags"] == 0)
    idx = np.flatnonzero(live)
    info = {"live": live}
    if len(idx) == 0:
        return (contacts, out, info) if details else (contacts, out)
    n = len(idx)
    cols = np.arange(n)
    ka, kb = ref._counts(a)[i[idx]], ref._counts(b)[j[idx]]
    ax, ay, bx, by = _rows16(a[0], i[idx]), _rows16(a[1], i[idx]), _rows16(b[0], j[idx]), _rows16(b[1], j[idx])
    e = contacts["axis"][idx].astype(np.int64)
    with np.errstate(all="ignore"):
        # step 1: reference and incident polygon; the winning axis as the contact rule computes it
        ref_b = e >= ka
        r = e - np.where(ref_b, ka, 0)
        rx, ry, k_r = np.where(ref_b, bx, ax), np.where(ref_b, by, ay), np.where(ref_b, kb, ka)
        ix, iy, k_i = np.where(ref_b, ax, bx), np.where(ref_b, ay, by), np.where(ref_b, ka, kb)
        r1 = np.where(r + 1 < k_r, r + 1, 0)
        nx = -(ry[r1, cols] - ry[r, cols])
        ny = rx[r1, cols] - rx[r, cols]
        min_a, max_a, _ = ref._interval(nx, ny, ax, ay, ka)
        min_b, max_b, _ = ref._interval(nx, ny, bx, by, kb)
        pos, _, _, length, d, usable = ref._axis_terms(np.ones(n, bool), nx, ny, min_a, max_a, min_b, max_b)
        depth = contacts["depth"][idx]
        assert usable.all() and ((d.view(np.uint32) == depth.view(np.uint32)) | ((d == 0) & (depth == 0))).all(), "the winning axis, restated, is not the contact's"
        up = ~ref_b == pos                                         # sigma > 0
        face = np.where(up, np.where(ref_b, max_b, max_a), np.where(ref_b, min_b, min_a))
        # step 2: the deepest vertex of I
        p = nx[None, :] * ix + ny[None, :] * iy                    # [16][n]; rows at or beyond kI are never looked at
        w, pw = np.zeros(n, np.int64), p[0].copy()
        for f in range(1, 16):
            deeper = (f < k_i) & np.where(up, p[f] < pw, p[f] > pw)
            w, pw = np.where(deeper, f, w), np.where(deeper, p[f], pw)
        # step 3: the other end of the incident edge
        nxt, prv = (w + 1) % k_i, (w - 1 + k_i) % k_i
        back = np.where(up, p[prv, cols] < p[nxt, cols], p[prv, cols] > p[nxt, cols])
        u = np.where(back, prv, nxt)
        feature = np.where(u == nxt, w, prv)
        single = k_i == 1
        xw, yw, xu, yu = ix[w, cols], iy[w, cols], ix[u, cols], iy[u, cols]
        # step 4: the slab
        tau0, tau1 = ny * rx[r, cols] - nx * ry[r, cols], ny * rx[r1, cols] - nx * ry[r1, cols]
        lo, hi = np.where(tau0 <= tau1, tau0, tau1), np.where(tau0 <= tau1, tau1, tau0)
        # step 5: the clip, each end against the original other end
        tw, tu = ny * xw - nx * yw, ny * xu - nx * yu

        def clip(xg, yg, tg, xh, yh, th):
            below, above = tg < lo, tg > hi
            s = (np.where(below, lo, hi) - tg) / (th - tg)
            moved = below | above
            return np.where(moved, xg + (xh - xg) * s, xg), np.where(moved, yg + (yh - yg) * s, yg), moved

        cx0, cy0, c0 = clip(xw, yw, tw, xu, yu, tu)
        cx1, cy1, c1 = clip(xu, yu, tu, xw, yw, tw)
        outside = ~single & (((tw < lo) & (tu < lo)) | ((tw > hi) & (tu > hi)))
        two = ~single & ~outside
        x0, y0 = np.where(two, cx0, xw), np.where(two, cy0, yw)
        # step 6: depths from the final coordinates
        p0, p1 = nx * x0 + ny * y0, nx * cx1 + ny * cy1
        d0 = np.where(up, face - p0, p0 - face) / length
        d1 = np.where(up, face - p1, p1 - face) / length
    rec = empty(n)
    rec["x0"], rec["y0"], rec["d0"] = x0, y0, d0
    rec["x1"], rec["y1"], rec["d1"] = np.where(two, cx1, F(0)), np.where(two, cy1, F(0)), np.where(two, d1, F(0))
    rec["feature"] = np.where(single, 0, feature)
    rec["count"] = np.where(two, 2, 1)
    rec["flags"] = (np.where(ref_b, REF_IS_B, 0) | np.where(two & c0, P0_CLIPPED, 0) | np.where(two & c1, P1_CLIPPED, 0)
                    | np.where(outside, OUTSIDE_SLAB, 0))
    out[idx] = rec
    if details:
        def spread(v, fill=0):
            full = np.full(len(i), fill, v.dtype)
            full[idx] = v
            return full
        info.update({name: spread(v) for name, v in dict(ref_b=ref_b, up=up, w=w, u=u, prv=prv, nxt=nxt, k_i=k_i, k_r=k_r, r=r, r1=r1, nx=nx, ny=ny,
                                                         lo=lo, hi=hi, length=length, face=face).items()})
    return (contacts, out, info) if details else (contacts, out)


def same(got, want):
    """every field equal; floats bit for bit, except that +0 equals -0 and a NaN equals a NaN"""
    ok = np.ones(len(want), bool)
    for f in FLOATS:
        g, w = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        ok &= (g.view(np.uint32) == w.view(np.uint32)) | ((g == 0) & (w == 0)) | (np.isnan(g) & np.isnan(w))
    for f in ("feature", "count", "flags", "reserved"):
        ok &= got[f] == want[f]
    return ok
