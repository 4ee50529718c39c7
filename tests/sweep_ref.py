"""CPU restatement of the sweep contract of include/c2d.h (c2d_poly_pair_sweeps / c2d_rect_pair_sweeps), written from the contract,
not from the kernel: plain numpy, element-wise and unfused (numpy never contracts a * b + c), np.fmin / np.fmax for the intervals,
/ and np.sqrt (both correctly rounded), and the sequential pick: axes in axis order, lo > t_in replaces t_in with its axis and the sign
of v, hi < t_out replaces t_out, both by compare and select.

poly_sweeps(a, b, i, j, a_motion, b_motion) and rect_sweeps(...) take LOCAL indices (the list entry minus its bases) and a motion per
set: the pair (dx, dy) of f32[n] planes, or None for a set that stands still.  They return a SWEEP_DT record per pair.  An index
outside its set, or a polygon whose vertex count is outside 1..rows, gives the BAD_PAIR record.  hit0 is the pairwise boolean restated
as tests/contact_ref.py restates it (strict <, the NaN rule of the first projections); test_sweep_ref_cpu.py pins the two to each
other.  dtype=np.float64 runs the same rule in binary64 on the same inputs (records with float64 toi, nx, ny): the yardstick of the
float32 rule's own rounding."""
import numpy as np

SWEEP_DT = np.dtype([("toi", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("axis", "<u2"), ("hit", "u1"), ("flags", "u1")])
SWEEP_DT64 = np.dtype([("toi", "<f8"), ("nx", "<f8"), ("ny", "<f8"), ("axis", "<u2"), ("hit", "u1"), ("flags", "u1")])
START_OVERLAP, BAD_PAIR = 1, 2
NONE = 0xFFFF
FLOATS = ("toi", "nx", "ny")


class _Pick:
    """the sequential pick over the axes of a batch of pairs, in the float type F"""

    def __init__(self, m, rx, ry, F):
        self.F, self.rx, self.ry = F, rx, ry
        self.t_in, self.t_out = np.zeros(m, F), np.ones(m, F)
        self.nx, self.ny = np.zeros(m, F), np.zeros(m, F)
        self.axis = np.full(m, NONE, np.int64)
        self.closing, self.never, self.sep = np.zeros(m, bool), np.zeros(m, bool), np.zeros(m, bool)

    def add(self, live, axis, nx, ny, min_a, max_a, min_b, max_b, first_a, first_b):
        """one axis of every pair where `live`; first_a, first_b: the projections of the two first vertices (hit0's NaN rule)"""
        self.sep |= live & ((max_a < min_b) | (max_b < min_a)) & ~(np.isnan(first_a) | np.isnan(first_b))
        o1, o2 = max_a - min_b, max_b - min_a
        v = nx * self.rx + ny * self.ry
        pos, neg = v > 0, v < 0
        self.never |= live & (v == 0) & ((o1 < 0) | (o2 < 0))
        q1, q2 = o1 / v, (-o2) / v
        lo, hi = np.where(pos, q2, q1), np.where(pos, q1, q2)
        moving = live & (pos | neg)
        enters, leaves = moving & (lo > self.t_in), moving & (hi < self.t_out)
        self.t_in = np.where(enters, lo, self.t_in)
        self.nx, self.ny = np.where(enters, nx, self.nx), np.where(enters, ny, self.ny)
        self.axis = np.where(enters, axis, self.axis)
        self.closing = np.where(enters, neg, self.closing)
        self.t_out = np.where(leaves, hi, self.t_out)

    def records(self, bad):
        F = self.F
        out = np.zeros(len(self.t_in), SWEEP_DT if F is np.float32 else SWEEP_DT64)
        hit = ~self.never & (self.t_in <= self.t_out)
        won = hit & (self.axis != NONE)
        s = np.where(self.closing, F(1), F(-1))
        out["toi"] = np.where(hit, self.t_in, F(np.inf))
        with np.errstate(all="ignore"):
            length = np.sqrt(self.nx * self.nx + self.ny * self.ny)
            out["nx"], out["ny"] = np.where(won, s * (self.nx / length), F(0)), np.where(won, s * (self.ny / length), F(0))
        out["axis"] = np.where(won, self.axis, NONE)
        out["hit"] = hit
        out[~self.sep] = (0.0, 0.0, 0.0, NONE, 1, START_OVERLAP)
        out[bad] = (0.0, 0.0, 0.0, NONE, 0, BAD_PAIR)
        return out


def _interval(nx, ny, x, y, k, F):
    """running fmin / fmax of nx * x + ny * y over the first k vertices of each column; also the first projection"""
    mn, mx = np.full(nx.shape, np.inf, F), np.full(nx.shape, -np.inf, F)
    for r in range(x.shape[0]):
        p = nx * x[r] + ny * y[r]
        real = r < k
        mn, mx = np.where(real, np.fmin(mn, p), mn), np.where(real, np.fmax(mx, p), mx)
    return mn, mx, nx * x[0] + ny * y[0]


def _relative_motion(a_motion, b_motion, ii, jj, m, F):
    """rx = b_dx[j] - a_dx[i], ry = b_dy[j] - a_dy[i]; a set that stands still contributes +0"""
    def of(motion, idx):
        if motion is None:
            return np.zeros(m, F), np.zeros(m, F)
        return np.asarray(motion[0], np.float32)[idx].astype(F), np.asarray(motion[1], np.float32)[idx].astype(F)

    (adx, ady), (bdx, bdy) = of(a_motion, ii), of(b_motion, jj)
    return bdx - adx, bdy - ady


def _counts(s):
    vx, _, k = s
    return np.full(vx.shape[1], vx.shape[0], np.int64) if k is None else np.asarray(k).astype(np.int64)


def poly_sweeps(a, b, i, j, a_motion=None, b_motion=None, dtype=np.float32):
    """a, b: (vx f32[rows][n], vy, k u8[n] or None); i, j: local indices of the pairs -> SWEEP_DT[len(i)] (SWEEP_DT64 under float64)"""
    F = dtype
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    m, n_a, n_b = len(i), a[0].shape[1], b[0].shape[1]
    bad = (i < 0) | (i >= n_a) | (j < 0) | (j >= n_b)
    if n_a == 0 or n_b == 0:
        return _Pick(m, np.zeros(m, F), np.zeros(m, F), F).records(np.ones(m, bool))
    ii, jj = np.where(bad, 0, i), np.where(bad, 0, j)
    ka, kb = _counts(a)[ii], _counts(b)[jj]
    bad |= (ka < 1) | (ka > a[0].shape[0]) | (kb < 1) | (kb > b[0].shape[0])
    ka, kb = np.where(bad, 1, ka), np.where(bad, 1, kb)
    ax, ay = np.asarray(a[0], np.float32)[:, ii].astype(F), np.asarray(a[1], np.float32)[:, ii].astype(F)
    bx, by = np.asarray(b[0], np.float32)[:, jj].astype(F), np.asarray(b[1], np.float32)[:, jj].astype(F)
    cols = np.arange(m)
    with np.errstate(all="ignore"):
        pick = _Pick(m, *_relative_motion(a_motion, b_motion, ii, jj, m, F), F)
        for side, (px, py, kp) in enumerate(((ax, ay, ka), (bx, by, kb))):
            for e in range(px.shape[0]):
                live = e < kp
                e0, e1 = np.where(live, e, 0), np.where(e + 1 < kp, e + 1, 0)        # the vertex index wraps at k
                nx, ny = -(py[e1, cols] - py[e0, cols]), px[e1, cols] - px[e0, cols]
                pick.add(live, e + (ka if side else 0), nx, ny, *_interval(nx, ny, ax, ay, ka, F)[:2], *_interval(nx, ny, bx, by, kb, F)[:2],
                         nx * ax[0] + ny * ay[0], nx * bx[0] + ny * by[0])
        return pick.records(bad)


def rect_sweeps(a, b, i, j, a_motion=None, b_motion=None, dtype=np.float32):
    """a f32[8][n_a], b f32[8][n_b] (planes x0, y0, ..., x3, y3); i, j: local indices of the pairs -> SWEEP_DT[len(i)]"""
    F = dtype
    i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    m = len(i)
    bad = (i < 0) | (i >= a.shape[1]) | (j < 0) | (j >= b.shape[1])
    if a.shape[1] == 0 or b.shape[1] == 0:
        return _Pick(m, np.zeros(m, F), np.zeros(m, F), F).records(np.ones(m, bool))
    ii, jj = np.where(bad, 0, i), np.where(bad, 0, j)
    r1, r2 = a[:, ii].astype(F), b[:, jj].astype(F)
    four, live = np.full(m, 4, np.int64), np.ones(m, bool)
    with np.errstate(all="ignore"):
        pick = _Pick(m, *_relative_motion(a_motion, b_motion, ii, jj, m, F), F)
        for which, r in enumerate((r1, r2)):
            for e in range(4):
                nx, ny = r[(2 * e + 2) & 7] - r[2 * e], r[(2 * e + 3) & 7] - r[2 * e + 1]      # the edge VECTOR is the axis
                min_a, max_a, first_a = _interval(nx, ny, r1[0::2], r1[1::2], four, F)
                min_b, max_b, first_b = _interval(nx, ny, r2[0::2], r2[1::2], four, F)
                pick.add(live, np.full(m, 4 * which + e), nx, ny, min_a, max_a, min_b, max_b, first_a, first_b)
        return pick.records(bad)


def same(got, want):
    """every field equal; the three floats bit for bit, except that +0 and -0 are equal"""
    ok = np.ones(len(want), bool)
    for f in FLOATS:
        g, w = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        ok &= (g.view(np.uint32) == w.view(np.uint32)) | ((g == 0) & (w == 0))
    for f in ("axis", "hit", "flags"):
        ok &= got[f] == want[f]
    return ok
