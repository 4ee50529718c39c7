"""What the tests of c2d_poly_set_casts_grid share (test_gpu_casts_grid.py, test_cast_grid_cases_cpu.py, tools/cast_grid_fuzz.py),
built on cast_harness.py and clearance_grid_harness.py: the frame's call between guard bands (tests/best_key_harness.py) bound to the
query, the check that runs it beside c2d_poly_set_casts on the same arguments, the sparse scene
with its per-pair records computed once, the deals of B's indices, and the constructions whose answer depends on the order in which
the candidates are met.  The judge is cast_ref, unchanged.  The scenes are numpy only, so the CPU tests can reach them; nothing here
loads libc2d.so."""
import functools
import itertools

import numpy as np

import best_key_harness as best
import cast_cases as cases
import cast_harness as ch
import cast_ref as ref
import clearance_grid_harness as gh
import pair_list_harness as h
import pair_search_harness as psh
import sweep_broad_harness as sh
import sweep_broad_ref
import sweep_ref as sref

DT = ref.CAST_DT
F32 = np.float32
NO_POLY = ref.NO_POLY
N_A_SIZES = [1, 63, 64, 65, 255, 256, 257]
N_B_SIZES = [1, 64, 513, 1031]
REACHES = [2.0, 6.0]
CANDIDATE_CAP = 1024             # kCandidateCap of csrc/c2d_broad.hpp: the sorted entries a walk may look at in the row kernel
Scene, take, take_motion, assert_same = ch.Scene, ch.take, ch.take_motion, ch.assert_same


# ---- the device side ----------------------------------------------------------------------------------------------------------
call = functools.partial(best.call, best.CASTS_GRID)                # call(eng, a_set, b_set, n_a, a_motion=None, b_motion=None, capacity=None, expect_error=False, band=None, **kw)
twice = functools.partial(best.twice, best.CASTS_GRID)              # twice(eng, a_set, b_set, n_a, what, **kw): the call, run twice: the same bytes


def check(eng, a_set, b_set, n_a, want, what, nxm=True, **kw):
    """the grid call, twice (the same bytes), against the reference's records `want` (None: not judged here); then
    c2d_poly_set_casts on the same arguments in the same run: the same bytes.  Returns the records."""
    got = twice(eng, a_set, b_set, n_a, what, **kw)
    if want is not None:
        assert_same(got, want, what)
    if nxm:
        best.check_against_sibling(got, ch.call(eng, a_set, b_set, n_a, **kw), what, ("grid", "c2d_poly_set_casts"))
    return got


def check_scene(eng, a, b, ma, mb, what, want=None, place_a=(1, 3), place_b=(2, 0), with_k=True, same=False, expect_error=False, **kw):
    """(a, ma) against (b, mb) uploaded with offsets and strides (same: one set against itself, the same memory and motion planes)
    through check(); the reference is cast_ref.casts unless handed in.  Returns (records, the reference's)."""
    n_a = a[0].shape[1]
    sc = Scene(eng, a, b, ma, mb, place_a, place_b, with_k=with_k, same=same)
    try:
        if want is None:
            with np.errstate(all="ignore"):
                want = ref.casts(a, b, ma, mb, **kw)
        got = check(eng, sc.a.set, sc.b_set, n_a, want, what, expect_error=expect_error, **sc.motions(), **kw)
    finally:
        sc.free()
    return got, want


# ---- the sparse scene (numpy only) ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sparse(wl, reach):
    """-> a, b, ma, mb, S [257][1031]: cast_cases.scene(wl, 257, 1031, extent=160.0, reach=reach) and the per-pair records of all its
    pairs, computed once per process and read-only"""
    a, b, ma, mb = cases.scene(wl, 257, 1031, extent=160.0, reach=reach)
    S = ref.pair_records(a, b, ma, mb)
    S.setflags(write=False)
    return a, b, ma, mb, S


@functools.lru_cache(maxsize=None)
def own_set(wl):
    """-> s, ms, S [257][257]: the 257 queries of cast_cases.scene in a quarter of the area (the density of the scene's obstacles)
    with motions of up to +-6, and the per-pair records of the set against itself with its own motion (read-only)"""
    s, _, ms, _ = cases.scene(wl, 257, 1, extent=80.0, reach=6.0, seeds=(9504, 9505, 9506))
    S = ref.pair_records(s, s, ms, ms)
    S.setflags(write=False)
    return s, ms, S


def shares(rec):
    """-> the shares of miss records, start overlaps (toi == 0) and moving hits (toi > 0) among the records"""
    hit = rec["hit"] == 1
    return float(((rec["hit"] == 0) & (rec["flags"] == 0)).mean()), float((hit & (rec["toi"] == 0)).mean()), float((hit & (rec["toi"] > 0)).mean())


def mixed_rows(wl, n_a, n_b, rows_a, rows_b, reach=4.0):
    """two small sparse sets in other row layouts with their motions: rows_a without a count plane's help (every polygon has rows_a
    vertices), rows_b with counts 3..rows_b"""
    ext = 160.0 * np.sqrt(max(n_a + n_b, 64) / 1288)
    a = wl.random_convex_polygon_set(n_a, seed=9700 + rows_a, kmin=rows_a, kmax=rows_a, extent=ext, rows=rows_a)
    b = wl.random_convex_polygon_set(n_b, seed=9800 + rows_b, kmin=min(3, rows_b), kmax=rows_b, extent=ext, rows=rows_b)
    ma, mb = h.motions(9900 + rows_a + rows_b, n_a, n_b, reach)
    return (a[0], a[1], None), b, ma, mb


def reference_by_hits(a, b, ma, mb, **kw):
    """cast_ref.reduce over per-pair records that are computed only where sweep_broad_ref.pairs (the judge of the swept pair search:
    sweep_ref's own `hit` over all pairs, behind an exact single-axis filter) lists a hit; every other pair keeps a miss record,
    which the reduction never looks into.  For scenes whose n_a x n_b is beyond pair_records (the station scene).
    test_cast_grid_cases_cpu.py pins it to cast_ref.casts."""
    n_a, n_b = a[0].shape[1], b[0].shape[1]
    with np.errstate(all="ignore"):
        p = sweep_broad_ref.pairs(a, b, ma, mb).astype(np.int64)
        S = np.zeros((n_a, n_b), sref.SWEEP_DT)
        S["toi"] = np.inf
        S[p[:, 0], p[:, 1]] = sref.poly_sweeps(a, b, p[:, 0], p[:, 1], ma, mb)
    return ref.reduce(S, ref.bad_counts(a), ref.bad_counts(b), **kw)


# ---- B's indices dealt in another order (numpy only) --------------------------------------------------------------------------------
def deals(n_b, seed=9650, random=3):
    """{name: ib}: orders of B's indices (B'[k] = B[ib[k]]): as built, reversed and `random` shuffles"""
    rng = np.random.default_rng(seed)
    out = {"as built": np.arange(n_b), "reversed": np.arange(n_b)[::-1].copy()}
    for r in range(random):
        out[f"shuffle {r}"] = rng.permutation(n_b)
    return out


def with_duplicates(ib, j):
    """{name: ib'}: obstacle j of the original set once more, at an index above every other (appended) and below (in front)"""
    return {"a duplicate at a larger index": np.concatenate([ib, [j]]), "a duplicate at a smaller index": np.concatenate([[j], ib])}


def permuted_hand_cases():
    """(name, a, b, ma, mb, kw, expect or None): every hand case of cast_cases.py with B's indices in every order (B has at most three
    polygons); expect only for the order as built"""
    for name, (a, b, ma, mb, kw, expect) in cases.hand_cases().items():
        n_b = b[0].shape[1]
        for perm in itertools.permutations(range(n_b)):
            ib = np.array(perm, np.int64)
            as_built = list(perm) == sorted(perm)
            yield (name + ("" if as_built else f" dealt {perm}"), a, take(b, ib) if n_b else b, ma, take_motion(mb, ib) if n_b else mb, kw,
                   expect if as_built else None)


def overlaps_beside_a_later_hit():
    """(a, b, ma): clearance_grid_harness.overlapping_three() set in motion.  Per permutation of three indices a query square that
    three squares overlap at t = 0 (their minimum corners in different places, their indices 4 q + 1 .. 4 q + 3 dealt by the
    permutation), and at the SMALLER index 4 q a square a quarter of a step to its right, which the query, moving by (+1, 0),
    reaches at t = 1/256.  The winner is the smallest overlapping index, 4 q + 1, at toi = 0: a start overlap beats the earlier
    index, and among the overlaps the index decides whichever is met last."""
    a, b = gh.overlapping_three()
    n = a[0].shape[1]
    return a, b, (np.ones(n, F32), np.zeros(n, F32))


def ties_across_cells(step=1.0 / 64, pitch=64.0, fillers=40):
    """(a, b, ma, tied): per permutation of three indices a query square of 32 steps moving by (+16, +16) steps; R, 8 steps to its
    right, 32 wide and reaching 29 steps below the query's bottom; U, 8 steps above it, 32 high and reaching 29 steps to the left of
    the query's left side; and a square F 12 steps beyond its upper right corner.  R and U are reached at the same instant, t = 1/2
    exactly (every coordinate and motion is a multiple of 1/64, every quotient of the rule is exact), F at t = 3/4.  Behind the
    stations B holds `fillers` squares of 58 steps far from everything: with R and U (61 steps long) they put the largest common box
    extent into [7/8, 1), so the grid's cell size is 1 (the upper edge of that bin of c2d_broad.hip's extent histogram), every box
    is narrower than a cell and nothing is wild.  The minimum corners of R and U are 69 steps apart in x and in y, more than a cell:
    they lie in different cells of different cell rows, R's row first, and a walk in cell order meets R before U.  The indices
    3 q .. 3 q + 2 are dealt by the permutation, so in half of the stations R has the larger index, and in two the later F has the
    smallest.  tied[q]: the indices of R and U.  The winner is the smaller of the two."""
    perms = list(itertools.permutations(range(3)))
    n = len(perms)
    s, g, far, reach, fill = 32 * step, 8 * step, 12 * step, 29 * step, 58 * step
    ax, ay = np.zeros((16, n), F32), np.zeros((16, n), F32)
    bx, by = np.zeros((16, 3 * n + fillers), F32), np.zeros((16, 3 * n + fillers), F32)
    rect = lambda x, y, w, hgt: ([x, x + w, x + w, x], [y, y, y + hgt, y + hgt])     # noqa: E731
    tied = []
    for q, perm in enumerate(perms):
        x0, y0 = pitch * (q % 3) + 5.0, pitch * (q // 3) + 3.0
        ax[:4, q], ay[:4, q] = rect(x0, y0, s, s)
        shapes = [(x0 + s + g, y0 - reach, s, s + reach), (x0 - reach, y0 + s + g, s + reach, s), (x0 + s + far, y0 + s + far, s, s)]      # R, U, F
        for which, rank in enumerate(perm):
            bx[:4, 3 * q + rank], by[:4, 3 * q + rank] = rect(*shapes[which])
        tied.append([3 * q + perm[0], 3 * q + perm[1]])
    for f in range(fillers):
        bx[:4, 3 * n + f], by[:4, 3 * n + f] = rect(4.0 * f, -100.0, fill, fill)
    k_a, k_b = np.full(n, 4, np.uint8), np.full(3 * n + fillers, 4, np.uint8)
    return (ax, ay, k_a), (bx, by, k_b), (np.full(n, 16 * step, F32), np.full(n, 16 * step, F32)), np.array(tied)


# ---- wild and absent (numpy only) ------------------------------------------------------------------------------------------------
def wild_scene(wl, n_a=257, n_b=230):
    """(a, b, ma, mb) after test_gpu_sweep_broad.py's wild scene, at a size the N x M reference affords: non-finite motions in A and
    motions of 2^60 and more in both sets, vertices carried past 2^60 by their motion, points and segments, one fast mover in each
    set whose swept box spans the scene, NaN and inf vertices, counts of 0 and rows + 1"""
    a, ma = sh.sparse_scene(wl, n_a, 5001, density=0.3)
    b, mb = sh.sparse_scene(wl, n_b, 5002, rows=12, kmax=12, density=0.3)
    a, b = tuple(np.array(x) for x in a), tuple(np.array(x) for x in b)
    ma, mb = (ma[0].copy(), ma[1].copy()), (mb[0].copy(), mb[1].copy())
    big = F32(2.0 ** 61)
    ma[0][[10, 11, 12, 13]] = [np.nan, np.inf, -np.inf, big]
    mb[1][[20, 21, 22, 23]] = [1e30, -1e30, 2.0 ** 59, -big]          # (a non-finite motion of an OBSTACLE is a hit at +0 for every query: the transposed call)
    ma[1][14], mb[0][24] = F32(3e38), F32(-3e38)
    ma[0][15], mb[1][25] = F32(2.0 ** 60), F32(-2.0 ** 60)
    a[0][:, 30] = a[0][:, 30] * F32(2.0 ** 50) + F32(2.0 ** 59)          # a vertex carried past 2^60 by its motion
    a[1][:, 30] = a[1][:, 30] * F32(2.0 ** 50)
    ma[0][30] = F32(2.0 ** 59.5)
    b[0][:, 31], mb[0][31] = b[0][:, 31] + F32(-2.0 ** 59.9), F32(-2.0 ** 58)
    a[2][[40, 41, 42]], b[2][[43, 44, 45]] = [1, 2, 2], [1, 1, 2]          # points and segments
    ma[0][40], ma[1][41] = F32(50.0), F32(-50.0)
    ma[0][50], ma[1][50] = F32(40.0), F32(30.0)                            # one fast mover per set: its swept box spans many cells
    mb[0][51], mb[1][51] = F32(-1e6), F32(1e6)
    a[0][1, 70], a[1][0, 71], b[0][2, 72], b[1][1, 73] = np.nan, np.inf, -np.inf, np.nan      # NaN and inf vertices
    a[2][[60, 61, 62]], b[2][[63, 64, 65]] = [0, 17, 255], [0, 13, 200]   # counts 0 and rows + 1
    return psh.nan_padded(a), psh.nan_padded(b), ma, mb
