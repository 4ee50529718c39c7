"""What the tests of c2d_poly_set_clearances_grid share (test_gpu_clearances_grid.py, tools/clearance_grid_fuzz.py), modelled on
clearance_harness.py: the frame's call between guard bands and its comparisons (tests/best_key_harness.py) bound to the query, the
check that runs it beside c2d_poly_set_clearances, the sparse scenes with the margins taken from the judge's own distances, and the constructions whose answer depends on the order in which
the candidates are met.  The scenes and the judge are numpy only, so the CPU tests can reach them; nothing here loads libc2d.so."""
import functools
import itertools

import numpy as np

import best_key_harness as best
import clearance_grid_ref as ref
import near_broad_harness as nh
import near_broad_ref as nref
import pair_search_harness as psh

DT = ref.CLEARANCE_DT
F32 = np.float32
NO_POLY = 0xFFFFFFFF
SIZES = [1, 63, 64, 65, 257, 1031]
FORMS = ["two_sets", "self_skip", "mixed_layouts"]
MARGIN_NAMES = ["zero", "below_median", "median", "all"]
REACH = 3.0 * nh.SIZE          # the judge looks this far for the scenes' nearest neighbours


# ---- the device side ----------------------------------------------------------------------------------------------------------
call = functools.partial(best.call, best.CLEARANCES_GRID)                # call(eng, a_set, b_set, n_a, max_dist, capacity=None, expect_error=False, band=None, **kw)
twice = functools.partial(best.twice, best.CLEARANCES_GRID)              # twice(eng, a_set, b_set, n_a, max_dist, what, **kw): the call, run twice: the same bytes
assert_same = functools.partial(best.assert_same, best.CLEARANCES_GRID)  # assert_same(got, want, what)


def check(eng, a, b, max_dist, what, want=None, place_a=(1, 3), place_b=(2, 0), with_k=True, expect_error=False, all_winners=None, **kw):
    """a against b (b None: the set against itself, the same memory) through the call, twice (the same bytes), against the judge;
    where the judge says that every query has a winner (or all_winners is True), also against c2d_poly_set_clearances on the GPU,
    byte for byte.  Returns (records, the judge's)."""
    A = psh.DeviceSet(eng, a, offset=place_a[0], stride=a[0].shape[1] + place_a[1], with_k=with_k)
    B = A if b is None else psh.DeviceSet(eng, b, offset=place_b[0], stride=b[0].shape[1] + place_b[1], with_k=with_k)
    n_a = a[0].shape[1]
    try:
        got = twice(eng, A.set, B.set, n_a, max_dist, what, expect_error=expect_error, **kw)
        if want is None:
            want = ref.clearances(a, a if b is None else b, max_dist, **kw)
        assert_same(got, want, what)
        if all_winners is None:
            all_winners = bool((want["poly"] != NO_POLY).all())
        if all_winners and n_a:
            assert (want["poly"] != NO_POLY).all(), what
            full = best.call(best.CLEARANCES, eng, A.set, B.set, n_a, expect_error=expect_error, **kw)
            best.check_against_sibling(got, full, what + ": every query has a winner", ("grid", "c2d_poly_set_clearances"))
    finally:
        A.free()
        if B is not A:
            B.free()
    return got, want


# ---- the sparse scenes (numpy only) ---------------------------------------------------------------------------------------------
def scene_of(wl, n, form, shift=0):
    """(a, b, kw): the scene of test_gpu_near_broad.py for (n, form) at half its density, so that a good share of the queries touch
    nothing; b None: the set against itself under SKIP_SELF.  shift: another draw of the same scene"""
    a = psh.sparse_set(wl, n, 1000 + n + 100 * shift, density=0.5)
    b = psh.sparse_set(wl, n // 2 + 37, 2000 + n, density=0.5)
    kw = {}
    if form == "self_skip":
        b, kw = None, dict(flags=ref.SKIP_SELF, row_base=5, col_base=5)
    elif form == "mixed_layouts":                       # rows 4 without a count plane against rows 8 with one, other strides and offsets
        full = wl.random_convex_polygon_set(n, seed=3000 + n + 100 * shift, kmin=4, kmax=4, extent=400.0 * np.sqrt(max(n, 64) / 32768), rows=4)
        a = (full[0], full[1], None)
        b = psh.sparse_set(wl, n // 2 + 37, 2000 + n, rows=8, kmax=8, density=0.5)
    return a, b, kw


_SCENES = {}


def scene_with_margins(wl, n, form):
    """-> a, b, kw, margins {name: max_dist}, judge(max_dist) -> CLEARANCE_DT[n].  The considered pairs within REACH and their records
    are computed once per scene; the judge of a smaller margin is the same reduction over the records with hit | dist <= max_dist,
    which is what near_broad_ref.pairs lists at that margin (test_clearance_grid_ref_cpu.py pins the two).  The margins: 0; the
    (lower) median of the nearest distances of the queries that touch nothing, which that query's record meets exactly
    (dist == max_dist); the float below it; and the largest of them, at which every query that has a neighbour within REACH has a
    winner."""
    if (n, form) in _SCENES:
        return _SCENES[n, form]
    for shift in range(16):                             # (n = 1: a draw whose one query touches nothing but has a neighbour)
        a, b, kw = scene_of(wl, n, form, shift)
        bb = a if b is None else b
        with np.errstate(all="ignore"):
            ii, jj, rec = ref.considered(a, bb, REACH, **kw)
        bad_a = ref.cref.bad_counts(a)
        col_base = kw.get("col_base", 0)

        def judge(max_dist, ii=ii, jj=jj, rec=rec, bad_a=bad_a, col_base=col_base):
            keep = nref.listed(rec, max_dist)
            return ref.reduce_pairs(n, bad_a, ii[keep], jj[keep], rec[keep], col_base)

        nearest = judge(REACH)
        apart = np.sort(nearest["dist"][(nearest["poly"] != NO_POLY) & (nearest["hit"] == 0)])
        if len(apart):
            break
    if n == 1 and b is None:                            # one polygon against itself under SKIP_SELF: nothing to consider at any margin
        apart = np.array([0.1, 1.0], F32)
    assert len(apart), (n, form)
    median = F32(apart[(len(apart) - 1) // 2])
    margins = {"zero": 0.0, "below_median": float(np.nextafter(median, F32(0))), "median": float(median), "all": float(apart[-1])}
    _SCENES[n, form] = (a, b, kw, margins, judge)
    return _SCENES[n, form]


# ---- ties in a free order (numpy only) ------------------------------------------------------------------------------------------
def shuffled_equidistant(step=1.0 / 64, gap=8, pitch=64.0):
    """(a, b, tied): one query square of 32 steps per permutation of four obstacle indices (24 stations, pitch apart), and per station
    four equal squares at the same exact distance gap * step: below, left, right and above the query, each in another grid cell,
    their indices within the station dealt by the permutation, so that whatever order a walk meets them in, in some station it meets
    the largest index first.  A fifth obstacle per station is a copy of the one dealt index 3 (a duplicate at a larger index), a sixth
    lies one step farther out.  tied[q]: the indices of station q's obstacles at the smallest distance.  Every coordinate is a
    multiple of 1/64 below 2^12: the distance rule is exact."""
    perms = list(itertools.permutations(range(4)))
    n = len(perms)
    s, g = 32 * step, gap * step
    ax, ay = np.zeros((16, n), F32), np.zeros((16, n), F32)
    bx, by = np.zeros((16, 6 * n), F32), np.zeros((16, 6 * n), F32)
    tied = []
    sq = lambda x, y: ([x, x + s, x + s, x], [y, y, y + s, y + s])     # noqa: E731
    rng = np.random.default_rng(77)
    slots = rng.permutation(6 * n).reshape(n, 6)                       # the stations' obstacles lie scattered through B
    for q, perm in enumerate(perms):
        x0, y0 = pitch * (q % 6), pitch * (q // 6)
        ax[:4, q], ay[:4, q] = sq(x0, y0)
        where = [(x0, y0 - g - s), (x0 - g - s, y0), (x0 + s + g, y0), (x0, y0 + s + g)]      # below, left, right, above
        own = np.sort(slots[q])                                        # the station's six indices, ascending
        for side, rank in enumerate(perm):
            bx[:4, own[rank]], by[:4, own[rank]] = sq(*where[side])
        dup_of = perm.index(3)
        bx[:4, own[4]], by[:4, own[4]] = sq(*where[dup_of])
        bx[:4, own[5]], by[:4, own[5]] = sq(x0 + s + g + step, y0 + s + g + step)               # farther: the corner, beyond the gap
        tied.append(own[:5])
    k_a, k_b = np.full(n, 4, np.uint8), np.full(6 * n, 4, np.uint8)
    return (ax, ay, k_a), (bx, by, k_b), np.array(tied)


def record_d2(rec):
    """the d2 of a separated record's winning candidate, from its own closest points: dx, dy, the squares and the sum as the rule forms them"""
    with np.errstate(all="ignore"):
        on_b = (rec["flags"] & 1) != 0                                 # EDGE_ON_B: the vertex is A's
        dx = np.where(on_b, rec["ax"] - rec["bx"], rec["bx"] - rec["ax"]).astype(F32)
        dy = np.where(on_b, rec["ay"] - rec["by"], rec["by"] - rec["ay"]).astype(F32)
        return (dx * dx + dy * dy).astype(F32)


def overlapping_three(step=1.0 / 64, pitch=64.0):
    """(a, b): per permutation of three indices a query square overlapped by three squares (shifted below-left, right, above: three
    different cells' worth of minimum corners), their indices dealt by the permutation, and beside them a separated square at a
    quarter of a step whose index is smaller than all three: a hit wins over the nearer-looking neighbour, and the smallest hit index
    wins whichever is met last."""
    perms = list(itertools.permutations(range(3)))
    n = len(perms)
    s = 32 * step
    ax, ay = np.zeros((16, n), F32), np.zeros((16, n), F32)
    bx, by = np.zeros((16, 4 * n), F32), np.zeros((16, 4 * n), F32)
    sq = lambda x, y: ([x, x + s, x + s, x], [y, y, y + s, y + s])     # noqa: E731
    for q, perm in enumerate(perms):
        x0, y0 = pitch * q, 3.0 * q
        ax[:4, q], ay[:4, q] = sq(x0, y0)
        where = [(x0 - s / 2, y0 - s / 2), (x0 + s / 2, y0), (x0, y0 + s / 2)]
        bx[:4, 4 * q], by[:4, 4 * q] = sq(x0 + s + step / 4, y0)                                # separated, index below the three
        for side, rank in enumerate(perm):
            bx[:4, 4 * q + 1 + rank], by[:4, 4 * q + 1 + rank] = sq(*where[side])
    return (ax, ay, np.full(n, 4, np.uint8)), (bx, by, np.full(4 * n, 4, np.uint8))


@functools.lru_cache(maxsize=None)
def exact_grid():
    """near_broad_harness.grid_boxes' squares: (a, b, dist of pair (q, q) in steps of 1/64)"""
    offsets = [(8, 0), (9, 0), (1, 0), (2, 0), (3, 4), (6, 8), (4, 3), (3, 5), (12, 16), (12, 17)]
    a, b = nh.grid_boxes(offsets)
    return a, b, [float(np.hypot(ox, oy)) for ox, oy in offsets]
