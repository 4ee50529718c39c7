"""The bands of relative gap between a pair's two best axes and a numpy model of the DECISION of the contact kernel's first pass
(c2d_contact.hip FastPick::decided), shared by test_contact_near_ties_cpu.py and test_gpu_contact_ties.py.  The
model is for judging inputs and for the proof only: what the GPU computes is compared with contact_ref alone."""
import numpy as np

F = np.float32
BANDS = ((0.0, 0.0), (0.0, 2.0 ** -22), (2.0 ** -22, 2.0 ** -20), (2.0 ** -20, 2.0 ** -19), (2.0 ** -19, 2.0 ** -18), (2.0 ** -18, 2.0 ** -16))
BAND_NAMES = ("0", "(0, 2^-22]", "(2^-22, 2^-20]", "(2^-20, 2^-19]", "(2^-19, 2^-18]", "(2^-18, 2^-16]", "above 2^-16")
SHIPPED = (2.0 ** -19, 1e-36)      # FastPick::decided: the relative and the absolute margin


def relative_gap(terms):
    """(d2 - d1) / |d1| of the two smallest usable float32 d of each pair (in float64; inf with fewer than two usable axes)"""
    d = np.sort(np.where(terms["usable"], terms["d"], np.inf).astype(np.float64), axis=1)
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(d[:, 1]), (d[:, 1] - d[:, 0]) / np.abs(d[:, 0]), np.inf)


def band_of(gap):
    """index into BAND_NAMES per pair"""
    out = np.full(len(gap), len(BANDS), np.int64)
    for q, (lo, hi) in enumerate(BANDS):
        out[(gap == 0) if hi == 0 else ((gap > lo) & (gap <= hi))] = q
    return out


def band_shares(terms):
    b = band_of(relative_gap(terms))
    return np.array([(b == q).mean() for q in range(len(BANDS))])


def fast_pick_model(terms, rel, absolute, seed):
    """The decision of the first pass only: q = o * r per usable axis with r = float32(1 / sqrt(len2)) moved by a seeded -1, 0 or +1
    ulp, the smallest estimate (the first of equals) and the smallest of all others, and decided()'s inequality in float32 with the
    margins (rel, absolute).  -> decided bool[m], axis i64[m] (of the smallest estimate), q f32 [m][slots]"""
    rng = np.random.default_rng(seed)
    usable, o, len2 = terms["usable"], terms["o"], terms["len2"]
    with np.errstate(all="ignore"):
        r = (1.0 / np.sqrt(len2.astype(np.float64))).astype(F)
        move = rng.integers(-1, 2, r.shape)
        r = np.where(move < 0, np.nextafter(r, F(0)), np.where(move > 0, np.nextafter(r, F(np.inf)), r)).astype(F)
        q = np.where(usable, o * r, F(np.inf)).astype(F)
        first = np.argmin(q, axis=1)                      # (numpy: the first of equal minima, as `q < q1` keeps it)
        rows = np.arange(len(q))
        q1 = q[rows, first]
        rest = q.copy()
        rest[rows, first] = np.inf
        q2 = rest.min(axis=1)
        lo2 = q2 - np.abs(q2) * F(rel) - F(absolute)
        hi1 = q1 + np.abs(q1) * F(rel) + F(absolute)
        decided = np.where(np.isinf(q2), True, lo2 > hi1)
    return decided, terms["axis"][rows, first], q
