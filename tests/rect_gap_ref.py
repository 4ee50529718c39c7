"""float32 numpy restatement of rect_gap_certified (csrc/c2d_math.hpp), operation by operation: the first tier of the pairwise
rectangle kernels (collide_pairs, csrc/c2d_sat.hip).  The fused products go through float64 as test_oracle._fma32 does.
Shared by tests/test_rect_gap_cpu.py (decisions against the oracle, the margin's inequality) and tests/test_gpu_sat_gap_form.py
(which pairs of a constructed batch are thin)."""
import numpy as np

F = np.float32
U = 2.0 ** -24

# the constants of rect_gap_certified, as float32
K_EDGE = F(120.0 * U)     # x C x |d|_1: roundings of the reference's projections and of the gap's own evaluation
K_DEFECT_EDGE = F(3.02)   # x (e1 + e2) x |d|_1: the quads against their v0 / v1 / v3 models
K_DEFECT_C = F(4.02)      # x C x e_q: the reference's edges 1, 2 against b, -a
K_CC = F(33.0 * U)        # x C x C: the defect's own rounding
ABS_SLACK = F(1e-36)
DOMAIN = F(2.0 ** 61)


def _fma32(a, b, c):
    return (np.asarray(a, F).astype(np.float64) * np.asarray(b, F).astype(np.float64) + np.asarray(c, F).astype(np.float64)).astype(F)


def _dot(px, py, qx, qy):
    return _fma32(px, qx, (py * qy).astype(F))


def _quad(r):
    """edge vectors a = v1 - v0, b = v3 - v0, doubled centre v0 + v2, |defect|_1 of a quad given as 8 planes"""
    x0, y0, x1, y1, x2, y2, x3, y3 = r
    ax, ay = (x1 - x0).astype(F), (y1 - y0).astype(F)
    bx, by = (x3 - x0).astype(F), (y3 - y0).astype(F)
    sx, sy = (x0 + x2).astype(F), (y0 + y2).astype(F)
    tx, ty = (x1 + x3).astype(F), (y1 + y3).astype(F)
    e = (np.abs((sx - tx).astype(F)) + np.abs((sy - ty).astype(F))).astype(F)
    return (ax, ay), (bx, by), (sx, sy), e


def rect_gap_terms(planes):
    """-> (G[4], M[4], C): the four computed gaps (directions a1, b1, a2, b2), their margins, the coordinate bound"""
    planes = np.asarray(planes, F)
    with np.errstate(all="ignore"):
        a1, b1, s1, e1 = _quad(planes[:8])
        a2, b2, s2, e2 = _quad(planes[8:])
        dx, dy = (s2[0] - s1[0]).astype(F), (s2[1] - s1[1]).astype(F)
        C = np.abs(planes[0])
        for k in range(1, 16):
            C = np.fmax(C, np.abs(planes[k]))
        sq = [_dot(*d, *d) for d in (a1, b1, a2, b2)]
        a1b1, a2b2 = np.abs(_dot(*a1, *b1)), np.abs(_dot(*a2, *b2))
        a1a2, a1b2 = np.abs(_dot(*a1, *a2)), np.abs(_dot(*a1, *b2))
        b1a2, b1b2 = np.abs(_dot(*b1, *a2)), np.abs(_dot(*b1, *b2))
        S = [((sq[0] + a1b1).astype(F) + (a1a2 + a1b2).astype(F)).astype(F),
             ((sq[1] + a1b1).astype(F) + (b1a2 + b1b2).astype(F)).astype(F),
             ((sq[2] + a2b2).astype(F) + (a1a2 + b1a2).astype(F)).astype(F),
             ((sq[3] + a2b2).astype(F) + (a1b2 + b1b2).astype(F)).astype(F)]
        G = [(np.abs(_dot(*d, dx, dy)) - s).astype(F) for d, s in zip((a1, b1, a2, b2), S)]
        m0 = _fma32(K_DEFECT_EDGE, (e1 + e2).astype(F), (K_EDGE * C).astype(F))
        c4 = (K_DEFECT_C * C).astype(F)
        cc = _fma32((K_CC * C).astype(F), C, ABS_SLACK)
        n = [_fma32(c4, e1, cc), _fma32(c4, e2, cc)]
        M = [_fma32((np.abs(d[0]) + np.abs(d[1])).astype(F), m0, n[q]) for d, q in zip((a1, b1, a2, b2), (0, 0, 1, 1))]
    return G, M, C


def rect_gap_certified(planes):
    """-> (col, sep, thin) of every pair of f32[16][n] vertex planes"""
    G, M, C = rect_gap_terms(planes)
    with np.errstate(all="ignore"):
        over = np.fmax(np.fmax((G[0] - M[0]).astype(F), (G[1] - M[1]).astype(F)), np.fmax((G[2] - M[2]).astype(F), (G[3] - M[3]).astype(F)))
        under = np.fmax(np.fmax((G[0] + M[0]).astype(F), (G[1] + M[1]).astype(F)), np.fmax((G[2] + M[2]).astype(F), (G[3] + M[3]).astype(F)))
        sep, col = over > 0, under < 0
        thin = ~((C < DOMAIN) & (sep | col))
    return col & ~thin, sep & ~thin, thin
