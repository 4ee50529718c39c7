"""CPU restatement of the contact contract of include/c2d.h (c2d_poly_pair_contacts / c2d_rect_pair_contacts), written from the
contract, not from the kernel: plain numpy float32, element-wise and unfused (numpy never contracts a * b + c), np.fmin / np.fmax
for the intervals, np.sqrt and / (both correctly rounded) and the sequential axis rule: axes in axis order, the first usable axis
is the first candidate, a later one replaces it only under strict <.

poly_contacts(a, b, i, j) and rect_contacts(a, b, i, j) take LOCAL indices (the list entry minus its bases) and return a
CONTACT_DT record per pair.  An index outside its set, or a polygon whose vertex count is outside 1..rows, gives the BAD_PAIR
record.  `hit` is the pairwise boolean restated the same way (strict <, the NaN rule of the first projections); the tests pin it to
the oracle."""
import numpy as np

CONTACT_DT = np.dtype([("depth", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("axis", "<u2"), ("hit", "u1"), ("flags", "u1")])
NO_AXIS, BAD_PAIR = 1, 2
AXIS_NONE = 0xFFFF
F = np.float32


def _axis_terms(live, nx, ny, min_a, max_a, min_b, max_b):
    """the contract's float32 terms of one axis of every pair: (pos, o, len2, sqrt(len2), d, usable)"""
    o1, o2 = max_a - min_b, max_b - min_a
    pos = o1 <= o2
    o = np.where(pos, o1, o2)
    len2 = nx * nx + ny * ny
    length = np.sqrt(len2)
    d = o / length
    return pos, o, len2, length, d, live & (len2 != 0) & ~np.isnan(d)


class _Rule:
    """the sequential rule over the axes of a batch of pairs"""

    def __init__(self, m, keep_terms=False):
        self.terms = [] if keep_terms else None        # per add(): the contract's own terms of that axis (axis_terms())
        self.d = np.full(m, np.inf, F)
        self.nx, self.ny = np.zeros(m, F), np.zeros(m, F)
        self.axis = np.full(m, AXIS_NONE, np.int64)
        self.sep = np.zeros(m, bool)

    def add(self, live, axis, nx, ny, min_a, max_a, min_b, max_b, first_a, first_b):
        """one axis of every pair where `live`; first_a, first_b: the projections of the two first vertices"""
        pos, o, len2, length, d, usable = _axis_terms(live, nx, ny, min_a, max_a, min_b, max_b)
        if self.terms is not None:
            self.terms.append((np.broadcast_to(axis, d.shape).astype(np.int64), o, len2, d, usable))
        take = usable & ((self.axis == AXIS_NONE) | (d < self.d))
        sign = np.where(pos, F(1), F(-1))
        self.d = np.where(take, d, self.d)
        self.nx = np.where(take, sign * (nx / length), self.nx)
        self.ny = np.where(take, sign * (ny / length), self.ny)
        self.axis = np.where(take, axis, self.axis)
        self.sep |= live & ((max_a < min_b) | (max_b < min_a)) & ~(np.isnan(first_a) | np.isnan(first_b))

    def axis_terms(self, bad):
        """what add() saw: axis i64, o f32, len2 f32, d f32, usable bool, each [pairs][axis slots in axis order]"""
        m = len(self.d)
        if not self.terms:      # an empty set: no axis was looked at
            return {"axis": np.zeros((m, 0), np.int64), "o": np.zeros((m, 0), F), "len2": np.zeros((m, 0), F), "d": np.zeros((m, 0), F),
                    "usable": np.zeros((m, 0), bool)}
        axis, o, len2, d, usable = (np.stack(x, axis=1) for x in zip(*self.terms))
        return {"axis": axis, "o": o, "len2": len2, "d": d, "usable": usable & ~bad[:, None]}

    def records(self, bad):
        out = np.zeros(len(self.d), CONTACT_DT)
        none = self.axis == AXIS_NONE
        out["depth"] = np.where(none, F(np.inf), self.d)
        out["nx"], out["ny"] = np.where(none, F(0), self.nx), np.where(none, F(0), self.ny)
        out["axis"] = self.axis
        out["hit"] = ~self.sep
        out["flags"] = np.where(none, NO_AXIS, 0)
        out[bad] = (0.0, 0.0, 0.0, AXIS_NONE, 0, BAD_PAIR)
        return out


def _counts(s):
    vx, _, k = s
    return np.full(vx.shape[1], vx.shape[0], np.int64) if k is None else np.asarray(k).astype(np.int64)


def _interval(nx, ny, x, y, k):
    """running fmin / fmax of nx * x + ny * y over the first k vertices of each column; also the first projection"""
    mn, mx = np.full(nx.shape, np.inf, F), np.full(nx.shape, -np.inf, F)
    for r in range(x.shape[0]):
        p = nx * x[r] + ny * y[r]
        real = r < k
        mn, mx = np.where(real, np.fmin(mn, p), mn), np.where(real, np.fmax(mx, p), mx)
    return mn, mx, nx * x[0] + ny * y[0]


def poly_contacts(a, b, i, j):
    """a, b: (vx f32[rows][n], vy, k u8[n] or None); i, j: local indices of the pairs -> CONTACT_DT[len(i)]"""
    rule, bad = _poly_rule(a, b, i, j, False)
    return rule.records(bad)


def poly_axis_terms(a, b, i, j):
    """The terms the rule of poly_contacts consumed, per pair and per axis slot (A's `rows` edges, then B's): a dict of
    axis i64, o f32, len2 f32, d f32 and usable bool, each [len(i)][rows_a + rows_b].  A slot at or beyond its polygon's vertex
    count, and every slot of a BAD_PAIR entry, is not usable."""
    rule, bad = _poly_rule(a, b, i, j, True)
    return rule.axis_terms(bad)


def _poly_rule(a, b, i, j, keep_terms):
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    ka_all, kb_all = _counts(a), _counts(b)
    n_a, n_b = a[0].shape[1], b[0].shape[1]
    bad = (i < 0) | (i >= n_a) | (j < 0) | (j >= n_b)
    ii, jj = np.where(bad, 0, i), np.where(bad, 0, j)
    if n_a == 0 or n_b == 0:
        return _Rule(len(i), keep_terms), np.ones(len(i), bool)
    ka, kb = ka_all[ii], kb_all[jj]
    bad |= (ka < 1) | (ka > a[0].shape[0]) | (kb < 1) | (kb > b[0].shape[0])
    ka, kb = np.where(bad, 1, ka), np.where(bad, 1, kb)
    ax, ay = np.asarray(a[0], F)[:, ii], np.asarray(a[1], F)[:, ii]
    bx, by = np.asarray(b[0], F)[:, jj], np.asarray(b[1], F)[:, jj]
    rule = _Rule(len(i), keep_terms)
    cols = np.arange(len(i))
    with np.errstate(all="ignore"):
        for side, (px, py, kp) in enumerate(((ax, ay, ka), (bx, by, kb))):
            for e in range(px.shape[0]):
                live = e < kp
                e1 = np.where(e + 1 < kp, e + 1, 0)        # the vertex index wraps at k
                e0 = np.where(live, e, 0)
                nx = -(py[e1, cols] - py[e0, cols])
                ny = px[e1, cols] - px[e0, cols]
                min_a, max_a, first_a = _interval(nx, ny, ax, ay, ka)
                min_b, max_b, first_b = _interval(nx, ny, bx, by, kb)
                rule.add(live, e + (ka if side else 0), nx, ny, min_a, max_a, min_b, max_b, first_a, first_b)
    return rule, bad


def rect_contacts(a, b, i, j):
    """a f32[8][n_a], b f32[8][n_b] (planes x0, y0, ..., x3, y3); i, j: local indices of the pairs -> CONTACT_DT[len(i)]"""
    rule, bad = _rect_rule(a, b, i, j, False)
    return rule.records(bad)


def rect_axis_terms(a, b, i, j):
    """poly_axis_terms for rect_contacts: each field [len(i)][8], the edge-vector axes 0..3 of a's quad, then 4..7 of b's"""
    rule, bad = _rect_rule(a, b, i, j, True)
    return rule.axis_terms(bad)


def _rect_rule(a, b, i, j, keep_terms):
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    a, b = np.asarray(a, F), np.asarray(b, F)
    bad = (i < 0) | (i >= a.shape[1]) | (j < 0) | (j >= b.shape[1])
    if a.shape[1] == 0 or b.shape[1] == 0:
        return _Rule(len(i), keep_terms), np.ones(len(i), bool)
    r1, r2 = a[:, np.where(bad, 0, i)], b[:, np.where(bad, 0, j)]
    four = np.full(len(i), 4, np.int64)
    live = np.ones(len(i), bool)
    rule = _Rule(len(i), keep_terms)
    with np.errstate(all="ignore"):
        for which, r in enumerate((r1, r2)):
            for e in range(4):
                nx = r[(2 * e + 2) & 7] - r[2 * e]          # the edge VECTOR is the axis (convex_collide)
                ny = r[(2 * e + 3) & 7] - r[2 * e + 1]
                min_a, max_a, first_a = _interval(nx, ny, r1[0::2], r1[1::2], four)
                min_b, max_b, first_b = _interval(nx, ny, r2[0::2], r2[1::2], four)
                rule.add(live, np.full(len(i), 4 * which + e), nx, ny, min_a, max_a, min_b, max_b, first_a, first_b)
    return rule, bad


def same(got, want):
    """every field equal; floats bit for bit, except that +0 and -0 are equal"""
    ok = np.ones(len(want), bool)
    for f in ("depth", "nx", "ny"):
        g, w = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        ok &= (g.view(np.uint32) == w.view(np.uint32)) | ((g == 0) & (w == 0))
    for f in ("axis", "hit", "flags"):
        ok &= got[f] == want[f]
    return ok
