"""Inputs shared by the tests of the shape casts (test_cast_ref_cpu.py, test_cast_cases_cpu.py, test_gpu_casts.py, best_key_graph_check.py,
tools/cast_fuzz.py): hand cases that are exact in binary32 with what the contract says of them, the sparse scene with its motions,
and the constructions that make the main kernel's own decisions visible in `poly`: the slid near-ties of clearance_cases.py set in
motion (every pair touches at toi = 1/2 in exact arithmetic) and boxes on a 1/64 grid that graze (t_in == t_out) or miss by one grid
step.  tests/test_cast_cases_cpu.py holds what they promise on the reference alone.  numpy only."""
import numpy as np

import clearance_cases as cc

F = np.float32
INF, NAN = float("inf"), float("nan")
NO_POLY, NONE16 = cc.NO_POLY, cc.NONE16
SKIP_SELF = 1
START_OVERLAP, BAD_PAIR = 1, 2
polys, box, empty = cc.polys, cc.box, cc.empty


def move(*d):
    """the motion of a set from one (dx, dy) per object"""
    return np.array([x for x, _ in d], F), np.array([y for _, y in d], F)


def hand_cases():
    """name -> (a, b, a_motion, b_motion, kw, expect): expect maps a field to the values the contract gives (one per query); all
    exact in binary32.  Unit boxes on a 1/4 grid; a query that moves by (4, 0) closes a gap of 1 at t = 1/4 on its axis 1 = (-1, 0)
    with v = 4 > 0 (tests/test_sweep_ref_cpu.py), so the normal is (1, 0)."""
    q, go = polys(box(0, 0)), move((4, 0))
    none = dict(poly=[NO_POLY], toi=[INF], nx=[0.0], ny=[0.0], axis=[NONE16], hit=[0], flags=[0], reserved0=[0])
    facing = dict(toi=[0.25], nx=[1.0], ny=[0.0], axis=[1], hit=[1], flags=[0], reserved0=[0])
    start = dict(toi=[0.0], nx=[0.0], ny=[0.0], axis=[NONE16], hit=[1], flags=[START_OVERLAP])
    g = 2.0 ** -140
    sliver = [(g, 0), (1, 0), (1, 1), (g, 1)]
    out = {
        "the_nearer_of_two_in_the_path": (q, polys(box(3, 0), box(2, 0), box(-4, 0)), go, None, {}, dict(poly=[1], **facing)),
        "two_reached_at_the_same_instant": (q, polys(box(2, 0.5), box(2, -0.5)), go, None, {}, dict(poly=[0], **facing)),
        "the_same_obstacle_twice": (q, polys(box(3, 0), box(2, 0), box(2, 0)), go, None, {}, dict(poly=[1], **facing)),
        "an_obstacle_behind_is_never_reached": (q, polys(box(-4, 0)), go, None, {}, none),
        "a_start_overlap_beats_any_moving_hit": (q, polys(box(2, 0), box(0.5, 0.5)), go, None, {}, dict(poly=[1], **start)),
        # B_0 is separated by 2^-140 and moves by -2^100: lo underflows to 0, a hit at +0 with no axis and START_OVERLAP clear
        # (tests/test_sweep_ref_cpu.py); B_1 overlaps from the start.  Both keys have toi = +0: the smaller index wins.
        "a_hit_at_zero_with_no_axis_before_a_start_overlap": (polys(box(-1, 0)), polys(sliver, box(-0.5, 0.5)), None, move((-2.0 ** 100, 0), (0, 0)), {},
                                                              dict(poly=[0], toi=[0.0], nx=[0.0], ny=[0.0], axis=[NONE16], hit=[1], flags=[0])),
        "a_start_overlap_before_a_hit_at_zero": (polys(box(-1, 0)), polys(box(-0.5, 0.5), sliver), None, move((0, 0), (-2.0 ** 100, 0)), {},
                                                 dict(poly=[0], **start)),
        # B = [2, 3] x [0, 1] moving by (-2, 2) shares the one point (1, 1) with A at t = 1/2: t_in == t_out, a hit;
        # by (-2, 2.5) y parts at t = 0.4, before x meets at t = 0.5: a miss
        "the_diagonal_graze_is_a_hit": (q, polys(box(2, 0)), None, move((-2, 2)), {}, dict(poly=[0], toi=[0.5], nx=[1.0], ny=[0.0], axis=[1], hit=[1], flags=[0])),
        "the_same_pass_a_little_steeper_misses": (q, polys(box(2, 0)), None, move((-2, 2.5)), {}, none),
        "the_steeper_pass_in_front_of_the_graze": (q, polys(box(2, 0), box(2, 0)), None, move((-2, 2.5), (-2, 2)), {}, dict(poly=[1], toi=[0.5], hit=[1])),
        "an_obstacle_moving_away_at_the_querys_speed": (q, polys(box(2, 0)), go, move((4, 0)), {}, none),      # r = 0: `never`
        "b_moving_and_a_still": (q, polys(box(3, 0), box(2, 0)), None, move((-4, 0), (-4, 0)), {}, dict(poly=[1], **facing)),
        "both_moving": (q, polys(box(3, 0), box(2, 0)), move((1, 0)), move((-3, 0), (-3, 0)), {}, dict(poly=[1], **facing)),
        "no_obstacles": (polys(box(0, 0), box(5, 5)), empty(), move((4, 0), (0, 1)), None, {}, {f: v * 2 for f, v in none.items()}),
        "only_the_self_pair": (q, q, go, go, dict(flags=SKIP_SELF), none),
        "self_pair_by_the_bases": (q, polys(box(2, 0), box(3, 0)), go, None, dict(flags=SKIP_SELF, row_base=7, col_base=7), dict(poly=[8], toi=[0.5], hit=[1])),
        "without_the_flag_self_hits": (polys(box(0, 0), box(3, 0)), polys(box(0, 0), box(3, 0)), move((4, 0), (4, 0)), move((4, 0), (4, 0)), {},
                                       dict(poly=[0, 1], hit=[1, 1], toi=[0.0, 0.0], flags=[START_OVERLAP] * 2)),
        # vertex counts out of range: a bad query gets the BAD_PAIR record, a bad obstacle is not considered (here it would be the first)
        "bad_counts": (polys(box(0, 0), box(0, 0), box(0, 0), counts=[4, 0, 17]), polys(box(5, 0), box(2, 0), box(3, 0), counts=[4, 0, 4]),
                       move((4, 0), (4, 0), (4, 0)), None, {},
                       dict(poly=[2, NO_POLY, NO_POLY], toi=[0.5, 0.0, 0.0], hit=[1, 0, 0], flags=[0, BAD_PAIR, BAD_PAIR], axis=[1, NONE16, NONE16])),
        "only_bad_obstacles": (q, polys(box(2, 0), box(3, 0), counts=[0, 200]), go, None, {}, none),
        # every coordinate NaN: no axis has ordered first projections, so the pairwise boolean says hit
        "nan_obstacle_beside_a_clean_one": (q, polys(box(2, 0), cc.NAN_BOX), go, None, {}, dict(poly=[1], **start)),
        "nan_query": (polys(cc.NAN_BOX), polys(box(2, 0), box(0, 0)), go, None, {}, dict(poly=[0], **start)),
        # a NaN motion: every v is NaN, every axis is ignored, nothing sets `never`: a hit at +0 with no axis
        "nan_motion": (q, polys(box(3, 0), box(2, 0)), None, move((-4, 0), (NAN, 0)), {}, dict(poly=[1], toi=[0.0], axis=[NONE16], hit=[1], flags=[0])),
        "all_misses": (q, polys(box(2, 0), box(0, 3), box(-3, -3)), move((0.5, 0)), None, {}, none),
    }
    return out


def scene(wl, n_a=64, n_b=513, extent=80.0, reach=6.0, seeds=(9501, 9502, 9503)):
    """the sparse scene of clearance_cases.scene with motions of up to +-reach per component (a few polygon radii) on both sets
    -> a, b, ma, mb"""
    a, b = cc.scene(wl, n_a=n_a, n_b=n_b, extent=extent, seeds=seeds[:2])
    rng = np.random.default_rng(seeds[2])
    ma, mb = (tuple((rng.uniform(-1, 1, n) * reach).astype(F) for _ in range(2)) for n in (n_a, n_b))
    return a, b, ma, mb


# ---- the slid near-ties set in motion: every pair touches at toi = 1/2 in exact arithmetic ---------------------------------------------
NEAR_TIE_THETAS, NEAR_TIE_OFFSETS = cc.NEAR_TIE_THETAS, cc.NEAR_TIE_OFFSETS


def moving_near_ties(theta, offset):
    """-> a, b, ma: clearance_cases.slid_near_ties(theta, offset) with every slab moved by 1.5 along its rotated local +y,
    (-1.5 sin theta, 1.5 cos theta) rounded to float32; the pentagons stand still.  Every pair is 0.75 apart along that direction."""
    a, b = cc.slid_near_ties(theta, offset)
    n_a = a[0].shape[1]
    return a, b, (np.full(n_a, F(-1.5 * np.sin(theta))), np.full(n_a, F(1.5 * np.cos(theta))))


def near_tie_shares(S):
    """S: the per-pair records [n_a][n_b], all hits -> the share of the queries whose best toi is exactly tied with, or 1..4 ulp ahead
    of, another obstacle's; the share with a runner-up 1..4 ulp behind; the share whose winner is beyond tile 0"""
    bits = np.ascontiguousarray(S["toi"]).view(np.uint32).astype(np.int64)
    low = np.sort(bits, axis=1)[:, :2]
    gap = low[:, 1] - low[:, 0]
    return float((gap <= 4).mean()), float(((gap >= 1) & (gap <= 4)).mean()), float((bits.argmin(axis=1) >= 64).mean())


# ---- grazes: boxes on a 1/64 grid, motions that are multiples of 1/16 ----------------------------------------------------------------
def grazes(n_a=96, seed=9601):
    """-> a, b, ma, mb, graze, miss.  Per query i (a box on the 1/64 grid with a motion on the 1/16 grid) three obstacles in a row:
    b[3 i]      the pass of DESIGN.md §5.15 one grid step too high: a gap of gx to the right, the relative motion (-2 gx, 2 dy) with
                dy + 1/64 the distance by which its bottom has to clear the query's top: y parts one grid step of time before x
                meets at t = 1/2.  A miss: miss[i] = 3 i.
    b[3 i + 1]  the same pass exactly: the two boxes share one point at t = 1/2 and nothing else, t_in == t_out.  graze[i] = 3 i + 1.
    b[3 i + 2]  the same pass one grid step lower: a hit at t = 1/2 as well, behind the graze by its index.
    gx and dy are multiples of 1/32, so every motion is a multiple of 1/16 and every quotient of the rule is exact.  The queries
    are far enough apart (16 units) that no query reaches another query's obstacles within the step."""
    rng = np.random.default_rng(seed)
    g = lambda lo, hi, step: rng.integers(int(lo / step), int(hi / step) + 1, n_a) * step  # noqa: E731
    x0, y0 = 16.0 * (np.arange(n_a) % 12) + g(0, 1, 1 / 64), 16.0 * (np.arange(n_a) // 12) + g(0, 1, 1 / 64)
    w, hh, wb, hb = g(0.25, 2, 1 / 64), g(0.5, 2, 1 / 64), g(0.25, 2, 1 / 64), g(0.25, 2, 1 / 64)
    gx, dy = g(1 / 32, 1, 1 / 32), g(1 / 32, 0.5, 1 / 32)      # dy <= 0.5 <= hh: the obstacle's bottom starts inside the query's height
    adx, ady = (rng.integers(-16, 17, n_a) / 16.0 for _ in range(2))
    qa, qb, mdx, mdy = [], [], [], []
    for i in range(n_a):
        qa.append(box(x0[i], y0[i], w[i], hh[i]))
        for lift in (1 / 64, 0.0, -1 / 64):
            qb.append(box(x0[i] + w[i] + gx[i], y0[i] + hh[i] - dy[i] + lift, wb[i], hb[i]))
            mdx.append(adx[i] - 2 * gx[i])
            mdy.append(ady[i] + 2 * dy[i])
    a, b = polys(*qa, rows=4), polys(*qb, rows=4)
    for s in (a, b):      # every coordinate is a float as written
        assert np.array_equal(s[0].astype(np.float64) * 64, np.round(s[0].astype(np.float64) * 64))
    return a, b, (adx.astype(F), ady.astype(F)), (np.array(mdx, F), np.array(mdy, F)), 3 * np.arange(n_a) + 1, 3 * np.arange(n_a)
