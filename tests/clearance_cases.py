"""Inputs shared by the tests of the clearance query (test_clearance_ref_cpu.py, test_clearance_bound_cpu.py, test_gpu_clearances.py,
best_key_graph_check.py, tools/clearance_fuzz.py): hand cases that are exact in binary32 with what the contract says of them, the
sparse clearance scene, the adversarial set of the certified bound, the numpy statement of a polygon's vertex box, and two
constructions that make the main kernel's own decisions visible in `poly`: the hard input classes of contact_cases.py beside a witness
(witness_batches) and obstacles that tie within a few ulp of dist (slid_near_ties); tests/test_clearance_cases_cpu.py holds what they
promise on the reference alone.  numpy only."""
import functools

import numpy as np

import contact_cases

F = np.float32
INF, NAN = float("inf"), float("nan")
NO_POLY, NONE16 = 0xFFFFFFFF, 0xFFFF
SKIP_SELF, NONE_FLAG = 1, 16
EDGE_ON_B, INTERIOR, NO_CANDIDATE, BAD_PAIR = 1, 2, 4, 8


def polys(*vertex_lists, rows=16, counts=None):
    """a polygon set (vx f32[rows][n], vy, k u8[n]) from vertex lists; counts overrides the stored vertex counts"""
    n = len(vertex_lists)
    vx, vy, k = np.zeros((rows, n), F), np.zeros((rows, n), F), np.zeros(n, np.uint8)
    for q, vs in enumerate(vertex_lists):
        for r, (x, y) in enumerate(vs):
            vx[r, q], vy[r, q] = x, y
        k[q] = len(vs)
    if counts is not None:
        k[:] = counts
    return vx, vy, k


def box(x, y, w=1.0, h=1.0):
    return [(x, y), (x + w, y), (x + w, y + h), (x, y + h)]


def empty(rows=16):
    return np.zeros((rows, 0), F), np.zeros((rows, 0), F), np.zeros(0, np.uint8)


TRIANGLE = [(0.5, 1.5), (1.5, 2.5), (-0.5, 2.5)]     # counter-clockwise, its lowest vertex half a unit above the unit box's top edge
NAN_BOX = [(NAN, NAN)] * 4
SKEW = [(0, 0), (1, -1), (0, 1)]                     # against the single point (inf, inf): separated, and every d2 is NaN


def hand_cases():
    """name -> (a, b, kw, expect): expect maps a field to the values the contract gives (one per query); all exact in binary32"""
    q = polys(box(0, 0))
    sqrt2 = float(np.sqrt(F(2.0)))
    out = {
        # unit boxes on a 1/4 grid
        "nearest_to_the_right": (q, polys(box(3, 0), box(1.5, 0), box(-4, 0)), {}, dict(poly=[1], dist=[0.5], hit=[0], flags=[0])),
        "two_equally_far": (q, polys(box(-1.5, 0), box(1.5, 0)), {}, dict(poly=[0], dist=[0.5], hit=[0])),
        "identical_obstacles": (q, polys(box(3, 0), box(1.5, 0), box(1.5, 0)), {}, dict(poly=[1], dist=[0.5], hit=[0])),
        # a hit beats a nearer-than-anything separated obstacle; the smallest hitting j
        "overlapping_one": (q, polys(box(1.25, 0), box(0.5, 0.5), box(0.25, 0.25)), {},
                            dict(poly=[1], dist=[0.0], hit=[1], ax=[0.0], ay=[0.0], bx=[0.0], by=[0.0], edge=[NONE16], vert=[NONE16], flags=[0])),
        "vertex_to_vertex": (q, polys(box(2, 2)), {}, dict(poly=[0], dist=[sqrt2], hit=[0], ax=[1.0], ay=[1.0], bx=[2.0], by=[2.0])),
        "triangle_over_box_edge": (polys(TRIANGLE), polys(box(0, 0)), {},
                                   dict(poly=[0], dist=[0.5], hit=[0], ax=[0.5], ay=[1.5], bx=[0.5], by=[1.0], flags=[EDGE_ON_B | INTERIOR])),
        "box_edge_under_triangle": (polys(box(0, 0)), polys(TRIANGLE), {},
                                    dict(poly=[0], dist=[0.5], hit=[0], ax=[0.5], ay=[1.0], bx=[0.5], by=[1.5], flags=[INTERIOR])),
        "no_obstacles": (polys(box(0, 0), box(5, 5)), empty(), {},
                         dict(poly=[NO_POLY] * 2, dist=[INF] * 2, hit=[0] * 2, flags=[NONE_FLAG] * 2, edge=[NONE16] * 2, vert=[NONE16] * 2, ax=[0.0] * 2, by=[0.0] * 2)),
        "only_the_self_pair": (q, q, dict(flags=SKIP_SELF), dict(poly=[NO_POLY], dist=[INF], hit=[0], flags=[NONE_FLAG], edge=[NONE16], vert=[NONE16])),
        "self_pair_by_the_bases": (q, polys(box(0, 0), box(3, 0)), dict(flags=SKIP_SELF, row_base=7, col_base=6), dict(poly=[6], dist=[0.0], hit=[1])),
        "self_clearance": (polys(box(0, 0), box(3, 0), box(7, 0)), polys(box(0, 0), box(3, 0), box(7, 0)), dict(flags=SKIP_SELF),
                           dict(poly=[1, 0, 1], dist=[2.0, 2.0, 3.0], hit=[0, 0, 0])),
        "without_the_flag_self_hits": (polys(box(0, 0), box(3, 0)), polys(box(0, 0), box(3, 0)), {}, dict(poly=[0, 1], hit=[1, 1], dist=[0.0, 0.0])),
        # vertex counts out of range: a bad query gets the BAD_PAIR record, a bad obstacle is not considered (here it would be the nearest)
        "bad_counts": (polys(box(0, 0), box(0, 0), box(0, 0), counts=[4, 0, 17]), polys(box(5, 0), box(1.5, 0), box(3, 0), counts=[4, 0, 4]), {},
                       dict(poly=[2, NO_POLY, NO_POLY], dist=[2.0, 0.0, 0.0], hit=[0, 0, 0], flags=[0, BAD_PAIR, BAD_PAIR], edge=[0, NONE16, NONE16])),
        "only_bad_obstacles": (q, polys(box(2, 0), box(3, 0), counts=[0, 200]), {}, dict(poly=[NO_POLY], dist=[INF], flags=[NONE_FLAG])),
        # every coordinate NaN: no axis has ordered first projections, so the pairwise boolean says hit
        "nan_obstacle_beside_a_clean_one": (q, polys(box(1.5, 0), NAN_BOX), {}, dict(poly=[1], hit=[1], dist=[0.0])),
        "nan_query": (polys(NAN_BOX), polys(box(1.5, 0), box(0, 0)), {}, dict(poly=[0], hit=[1], dist=[0.0])),
        # separated by A's axis (1, 1), and every d2 is NaN: dist = +inf, which wins only when nothing nearer is considered
        "no_candidate_alone": (polys(SKEW), polys([(INF, INF)]), {},
                               dict(poly=[0], dist=[INF], hit=[0], flags=[NO_CANDIDATE], edge=[NONE16], vert=[NONE16], ax=[0.0], bx=[0.0])),
        "no_candidate_beside_a_far_one": (polys(SKEW), polys([(INF, INF)], box(1000, -1.5)), {},
                                          dict(poly=[1], dist=[999.0], hit=[0], flags=[EDGE_ON_B | INTERIOR])),
        "two_no_candidates": (polys(SKEW), polys([(INF, INF)], [(INF, INF)]), {}, dict(poly=[0], dist=[INF], flags=[NO_CANDIDATE])),
    }
    # A hit and a separated pair whose d2 underflowed to 0 tie at dist = +0: boxes of side s = 2^-73 on a grid of g = 2^-76.  The
    # obstacle a gap of g to the right is separated by the exact test (its projections on the query's right edge, multiples of
    # s * g = 2^-149, are still distinct subnormals), and every candidate's d2 is at most g * g = 2^-152, which rounds to +0.
    s, g = 2.0 ** -73, 2.0 ** -76
    tiny = polys(box(0, 0, s, s))
    near, over, far = box(s + g, 0, s, s), box(s / 2, s / 2, s, s), box(4 * s, 0, s, s)
    zero_sep = dict(dist=[0.0], hit=[0], flags=[0], ax=[s], ay=[0.0], bx=[s + g], by=[0.0], edge=[0], vert=[0])
    out.update({
        "underflowed_separated_before_a_hit": (tiny, polys(far, near, over), {}, dict(poly=[1], **zero_sep)),
        "hit_before_an_underflowed_separated": (tiny, polys(far, over, near), {}, dict(poly=[1], dist=[0.0], hit=[1], edge=[NONE16], bx=[0.0])),
        "two_underflowed_separated": (tiny, polys(near, far, near), {}, dict(poly=[0], **zero_sep)),
    })
    return out


def scene(wl, n_a=200, n_b=500, extent=64.0, seeds=(9301, 9302)):
    """the sparse clearance scene: K ~ U{3..16}, radii 0.3 .. 2.5, centres in a box of +-extent: about half of the queries are
    separated from everything"""
    a = wl.random_convex_polygon_set(n_a, seed=seeds[0], extent=extent)
    b = wl.random_convex_polygon_set(n_b, seed=seeds[1], extent=extent)
    return a, b


def boxes(s):
    """per polygon the float vertex box of its live vertices and the largest |coordinate| among them, as the kernel stages them:
    -> f32[5][n] = xlo, xhi, ylo, yhi, c; c = +inf when a live coordinate is NaN or infinite (fmin / fmax drop NaN operands); a
    polygon with a count outside 1..rows gets NaN everywhere (the kernel never asks the bound about it)"""
    vx, vy, k = s
    rows, n = vx.shape
    kk = np.full(n, rows, np.int64) if k is None else np.asarray(k).astype(np.int64)
    ok = (kk >= 1) & (kk <= rows)
    live = np.arange(rows)[:, None] < np.where(ok, kk, 0)[None, :]
    out = np.full((5, n), np.nan, F)
    with np.errstate(all="ignore"):
        x, y = np.where(live, vx, np.nan), np.where(live, vy, np.nan)      # (fmin / fmax drop the NaN operands, as v_min / v_max do)
        out[0], out[1], out[2], out[3] = np.fmin.reduce(x, axis=0), np.fmax.reduce(x, axis=0), np.fmin.reduce(y, axis=0), np.fmax.reduce(y, axis=0)
        c = np.fmax(np.fmax.reduce(np.where(live, np.abs(vx), np.nan), axis=0), np.fmax.reduce(np.where(live, np.abs(vy), np.nan), axis=0))
        finite = (np.where(live, np.isfinite(vx) & np.isfinite(vy), True)).all(axis=0)
        out[4] = np.where(finite, c, np.inf)
    out[:, ~ok] = np.nan
    return out


def lb2(box_a, box_b):
    """the numpy statement of clearance_lb2 (csrc/c2d_clearance_bound.hpp) for boxes f32[5][m] each: used to COUNT what the skip
    leaves, never to decide a result"""
    a, b = np.asarray(box_a, F), np.asarray(box_b, F)
    with np.errstate(all="ignore"):
        C = np.where(a[4] > b[4], a[4], b[4])
        ok = (a[4] >= 0) & (b[4] >= 0) & (C >= F(2.0 ** -100)) & (C <= F(2.0 ** 60))
        for s in (a, b):
            for r in range(4):
                ok &= (s[r] >= -C) & (s[r] <= C)
        g = b[0] - a[1]
        for t in (a[0] - b[1], b[2] - a[3], a[2] - b[3]):
            g = np.where(t > g, t, g)
        L = (g - F(2.0 ** -21) * C).astype(F)
        return np.where(ok & (L > 0), L * L, F(0)).astype(F)


def adversarial_bound_sets():
    """-> a, b: on a 2^-20 grid, obstacles placed so that the box gap EQUALS the true distance (axis-parallel faces, and diamonds
    whose nearest vertices face each other along an axis), at coordinates near 1, 1e3 and 1e6, with gaps from one grid step up:
    where the margin of the bound has to work.  Query i faces obstacles of every gap at its own scale."""
    step = 2.0 ** -20
    qa, qb = [], []
    for base in (1.0, 1000.0, 1.0e6):
        ulp = float(np.spacing(F(base)))
        unit = max(step, ulp)                       # the grid that is representable at this scale
        x0 = float(F(base))
        qa.append(box(x0, x0, 64 * unit, 64 * unit))
        qa.append([(x0, x0 + 32 * unit), (x0 + 32 * unit, x0), (x0 + 64 * unit, x0 + 32 * unit), (x0 + 32 * unit, x0 + 64 * unit)])   # a diamond
        for gap in (1, 2, 3, 5, 8, 9, 16, 17, 64, 1024, 65536):
            g = gap * unit
            right = x0 + 64 * unit + g
            qb.append(box(right, x0, 32 * unit, 64 * unit))                                          # face to face on x
            qb.append(box(x0 - 16 * unit, x0 + 64 * unit + g, 96 * unit, 8 * unit))                  # face to face on y
            qb.append([(right, x0 + 32 * unit), (right + 8 * unit, x0 + 24 * unit), (right + 16 * unit, x0 + 32 * unit),
                       (right + 8 * unit, x0 + 40 * unit)])                                          # vertex to vertex (the diamond), vertex to face
            qb.append(box(x0 - g - 8 * unit, x0 + 8 * unit, 8 * unit, 8 * unit))                     # on the left
    a, b = polys(*qa), polys(*qb)
    for s in (a, b):      # every coordinate is a float as written
        assert np.isfinite(s[0]).all()
    return a, b


# ---- a witness beside every obstacle: the boolean of every single pair shows in `poly` ----------------------------------------------
WITNESS_LAYOUTS = {"one_tile": 1, "two_tiles": 64}      # name -> copies of B_j in front of the witness: [B_j, W] and [B_j x 64, W]
FLT_MAX = float(np.finfo(F).max)


def witness_half_side(a, b):
    """S = four times the largest finite |coordinate| of the batch, clamped to what float32 holds"""
    c = np.abs(np.concatenate([x.ravel() for x in (a[0], a[1], b[0], b[1])]).astype(np.float64))
    return float(F(min(4.0 * c[np.isfinite(c)].max(), FLT_MAX)))


@functools.lru_cache(maxsize=None)
def witness_batches(wl):
    """name -> (a, b, w, layouts) for every batch of contact_cases.hard_poly_batches: its sets a and b, the witness w (a set of one
    polygon: the axis-parallel box of half side witness_half_side(a, b) about the origin, in b's rows), and layouts[name of
    WITNESS_LAYOUTS] = (set, width): for every obstacle j the `width` polygons [B_j x (width - 1), W], laid out one behind the
    other, so that the shard of obstacle j is the polygons width * j .. width * (j + 1) - 1.  By the contract the winner of query i
    in the shard of j is the shard's index 0 exactly when D(i, j) is a hit or has dist == +0, as long as W is a hit for every query
    (then W's key is (+0, width - 1), and only a B_j at +0 comes before it)."""
    out = {}
    for name, (a, b, _, _) in contact_cases.hard_poly_batches(wl).items():
        S = witness_half_side(a, b)
        rows, n_b = b[0].shape
        w = polys([(-S, -S), (S, -S), (S, S), (-S, S)], rows=rows)
        layouts = {}
        for layout, copies in WITNESS_LAYOUTS.items():
            width = copies + 1
            idx = np.repeat(np.arange(n_b), width)
            is_w = np.tile(np.arange(width) == copies, n_b)
            layouts[layout] = (tuple(np.ascontiguousarray(np.where(is_w, w[p][..., :1], b[p][..., idx])) for p in range(3)), width)
        for s in (a, b, w) + tuple(l[0] for l in layouts.values()):
            for x in s:
                x.setflags(write=False)
        out[name] = (a, b, w, layouts)
    return out


# ---- obstacles within a few ulp of the best: where the main kernel's d2min must be the contract's to the last bit ----------------------
SLAB = [(-30.0, -1.0), (30.0, -1.0), (30.0, 0.0), (-30.0, 0.0)]                      # 60 x 1, its top edge on the local x axis
PENTAGON = [(0.0, 0.75), (0.6, 1.1), (0.4, 1.9), (-0.5, 1.8), (-0.7, 1.2)]           # its lowest vertex 0.75 above that edge
NEAR_TIE_THETAS = (0.37, 1.1, 2.9, 4.0)
NEAR_TIE_OFFSETS = ((0.0, 0.0), (100.0, -50.0))      # at the second the ulp of a coordinate is much larger than the ulp of dist


def slid_near_ties(theta, offset, seed=9401, n_a=64, n_b=130):
    """-> a, b: n_a copies of SLAB, each slid along its long direction by up to +-3, and n_b copies of PENTAGON, each slid along the
    same direction by up to +-20 (its lowest vertex stays over the inside of every slab's top edge); everything rotated by theta
    and moved by offset in float64 and rounded to float32 last.  In exact arithmetic every pair is 0.75 apart; in float32 the
    obstacles of a query differ by rounding alone."""
    rng = np.random.default_rng(seed)
    c, s = np.cos(theta), np.sin(theta)

    def place(shape, slide):
        local = np.array(shape, np.float64)[None, :, :] + np.stack([slide, np.zeros_like(slide)], axis=-1)[:, None, :]     # [n][k][2]
        x, y = c * local[..., 0] - s * local[..., 1] + offset[0], s * local[..., 0] + c * local[..., 1] + offset[1]
        vx, vy = np.zeros((16, len(slide)), F), np.zeros((16, len(slide)), F)
        vx[:len(shape)], vy[:len(shape)] = x.T.astype(F), y.T.astype(F)
        return vx, vy, np.full(len(slide), len(shape), np.uint8)

    return place(SLAB, rng.uniform(-3.0, 3.0, n_a)), place(PENTAGON, rng.uniform(-20.0, 20.0, n_b))


def near_tie_shares(dist):
    """dist f32 [n_a][n_b] (> 0) -> the share of the queries whose runner-up is 1..4 ulp of dist behind the winner, the share
    whose best is exactly tied with another obstacle, and the share whose winner (the smallest index at the best) is beyond tile 0"""
    bits = np.ascontiguousarray(dist).view(np.uint32).astype(np.int64)
    low = np.sort(bits, axis=1)[:, :2]
    gap = low[:, 1] - low[:, 0]
    return float(((gap >= 1) & (gap <= 4)).mean()), float((gap == 0).mean()), float((bits.argmin(axis=1) >= 64).mean())
