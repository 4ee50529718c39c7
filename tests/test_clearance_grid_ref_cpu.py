"""CPU tests of the judge of c2d_poly_set_clearances_grid (tests/clearance_grid_ref.py) and of the constructions the GPU tests run
(tests/clearance_grid_harness.py).  The judge's route (near_broad_ref.pairs, the distances of exactly those pairs, a per-row minimum)
is pinned against the direct one: all pairs through clearance_ref.pair_records, masked with near_broad_ref.listed; against
clearance_ref.clearances where the margin covers every nearest neighbour; and on cases that are exact in binary32.  No GPU."""
import numpy as np
import pytest

import clearance_cases as cases
import clearance_grid_harness as gh
import clearance_grid_ref as ref
import clearance_harness as ch
import clearance_ref as cref
import near_broad_ref as nref
import pair_search_harness as psh

F32 = np.float32
NO_POLY = 0xFFFFFFFF


def direct(a, b, max_dist, row_base=0, col_base=0, flags=0):
    """the contract, literally: every pair's record, the considered ones, the smallest key per row"""
    n_a, n_b = a[0].shape[1], b[0].shape[1]
    out = np.zeros(n_a, ref.CLEARANCE_DT)
    out[:] = ref.NONE_RECORD
    if n_b:
        with np.errstate(all="ignore"):
            D = cref.pair_records(a, b)
        ok = nref.listed(D, max_dist) & ~cref.bad_counts(b)[None, :]
        if flags & ref.SKIP_SELF:
            ok &= (row_base + np.arange(n_a))[:, None] != (col_base + np.arange(n_b))[None, :]
        for i in range(n_a):
            best = None
            for j in np.flatnonzero(ok[i]):
                key = (int(np.array(D["dist"][i, j]).view(np.uint32)), col_base + int(j))
                if best is None or key < best[0]:
                    best = (key, j)
            if best is not None:
                for f in cref.COPIED:
                    out[f][i] = D[f][i, best[1]]
                out["poly"][i], out["reserved0"][i] = col_base + best[1], 0
    out[cref.bad_counts(a)] = ref.BAD_RECORD
    return out


@pytest.mark.parametrize("n_a,n_b", [(1, 37), (17, 5), (64, 64), (40, 0)])
def test_the_route_equals_the_direct_one(wl, n_a, n_b):
    a, b = psh.sparse_set(wl, n_a, 31 + n_a, density=0.6), psh.sparse_set(wl, max(n_b, 1), 57 + n_b, rows=9, kmax=9, density=0.6)
    b = tuple(None if x is None else np.ascontiguousarray(x[..., :n_b]) for x in b)
    if n_a > 8:
        k = a[2].copy()
        k[[2, 5]] = [0, 17]                                    # two bad queries
        a = (a[0], a[1], k)
    if n_b > 8:
        k = b[2].copy()
        k[[1, 3]] = [0, 10]                                    # two bad obstacles (rows is 9)
        b = (b[0], b[1], k)
    seen_none = seen_win = 0
    for r in (0.0, 0.3, 1.0, 4.0, 50.0):
        for kw in ({}, dict(col_base=11), dict(flags=ref.SKIP_SELF, row_base=3, col_base=1)):
            got, want = ref.clearances(a, b, r, **kw), direct(a, b, r, **kw)
            assert ref.same(got, want).all(), (r, kw)
            assert got.tobytes() == want.tobytes() or (got["dist"] == 0).any()
            good = got["flags"] != cref.dref.BAD_PAIR
            seen_none, seen_win = seen_none + int((got["poly"][good] == NO_POLY).sum()), seen_win + int((got["poly"] != NO_POLY).sum())
            win = got["poly"] != NO_POLY
            assert ((got["hit"][win] == 1) | (got["dist"][win] <= F32(r))).all()
    assert (seen_none > 0 or n_a == 1) and (seen_win > 0 or n_b == 0)      # (the single query of the first case is hit)


def test_a_margin_over_every_nearest_neighbour_gives_the_clearances(wl):
    a, b = cases.scene(wl, n_a=60, n_b=90, extent=20.0)
    full = cref.clearances(a, b, col_base=4)
    assert (full["poly"] != NO_POLY).all() and (full["hit"] == 0).sum() > 10
    r = float(full["dist"].max())
    got = ref.clearances(a, b, r, col_base=4)
    assert got.tobytes() == full.tobytes()
    below = ref.clearances(a, b, float(np.nextafter(F32(r), F32(0))), col_base=4)
    far = full["dist"] == F32(r)
    assert (below["poly"][far] == NO_POLY).all() and ref.same(below[~far], full[~far]).all()
    # self-clearance of one set
    full = cref.clearances(a, a, flags=ref.SKIP_SELF)
    assert ref.clearances(a, a, float(full["dist"].max()), flags=ref.SKIP_SELF).tobytes() == full.tobytes()


def test_exact_cases_the_cut_is_the_records_own_compare():
    """squares on a 1/64 grid, face to face and at 3-4-5 corners: dist == max_dist gives the winner, max_dist one float below gives NONE"""
    a, b, steps = gh.exact_grid()
    for q, d in enumerate(steps):
        if d != int(d):
            continue                                       # (3, 5) and (12, 17): not exact
        at = F32(d / 64)
        got = ref.clearances(a, b, float(at))
        assert got["poly"][q] == q and got["dist"][q] == at and got["hit"][q] == 0
        got = ref.clearances(a, b, float(np.nextafter(at, F32(0))))
        assert got["poly"][q] == NO_POLY and got["flags"][q] == ref.NONE_FLAG and np.isinf(got["dist"][q])
    none = ref.clearances(a, b, 0.0)
    assert (none["poly"] == NO_POLY).all() and ref.clearances(a, b, -0.0).tobytes() == none.tobytes()
    everyone = ref.clearances(a, b, 21 / 64)
    assert np.array_equal(everyone["poly"], np.arange(len(steps)))


def test_hand_cases_of_the_clearance_contract_under_a_margin():
    """tests/clearance_cases.py's hand cases: at a margin beyond every distance the contract's own expectations hold, except that a
    pair without a usable candidate is considered only when it is hit; at margin 0 only hits and underflowed distances remain"""
    for name, (a, b, kw, expect) in cases.hand_cases().items():
        got = ref.clearances(a, b, 2000.0, **kw)
        if name.startswith("no_candidate_alone") or name == "two_no_candidates":
            assert (got["poly"] == NO_POLY).all() and (got["flags"] == ref.NONE_FLAG).all(), name
            continue
        for f, v in expect.items():
            assert np.array_equal(got[f], np.array(v, got[f].dtype)), (name, f, got[f], v)
        zero = ref.clearances(a, b, 0.0, **kw)
        keep = (got["hit"] == 1) | (got["dist"] == 0) | (got["poly"] == NO_POLY)
        assert ref.same(zero[keep], got[keep]).all() and (zero["poly"][~keep] == NO_POLY).all(), name


@pytest.mark.parametrize("form", gh.FORMS)
@pytest.mark.parametrize("n", gh.SIZES)
def test_the_scenes_margins_cut_between_winners_and_none(wl, n, form):
    """what test_gpu_clearances_grid.py relies on: the margins taken from the judge's own distances give both NONE records and
    winners in every scene, the median is met exactly by a record, and the filtered judge equals the judge's own route"""
    a, b, kw, margins, judge = gh.scene_with_margins(wl, n, form)
    none = win = 0
    for name in gh.MARGIN_NAMES:
        want = judge(margins[name])
        none, win = none + int((want["poly"] == NO_POLY).sum()), win + int((want["poly"] != NO_POLY).sum())
        if n >= 63 and name != "all":
            assert (want["poly"] == NO_POLY).any() and (want["poly"] != NO_POLY).any(), name
        if n <= 65:
            with np.errstate(all="ignore"):
                assert ref.clearances(a, a if b is None else b, margins[name], **kw).tobytes() == want.tobytes(), name
    if n == 1 and b is None:
        assert win == 0 and none == 4      # one polygon against itself under SKIP_SELF: the NONE record at every margin
        return
    assert none > 0 and win > 0
    at = judge(margins["median"])
    assert ((at["dist"] == F32(margins["median"])) & (at["hit"] == 0)).any(), "a record with dist == max_dist"
    below = judge(margins["below_median"])
    assert (below["poly"] == NO_POLY).sum() > (at["poly"] == NO_POLY).sum()


def test_some_scenes_have_a_winner_for_every_query_at_their_largest_margin(wl):
    """there the GPU test also compares with c2d_poly_set_clearances byte for byte"""
    full = [(n, form) for n in gh.SIZES for form in gh.FORMS
            if (lambda s: (s[4](s[3]["all"])["poly"] != NO_POLY).all())(gh.scene_with_margins(wl, n, form))]
    assert len(full) >= 6 and len({f for _, f in full}) == 3 and max(n for n, _ in full) >= 257, full


def test_the_free_order_constructions():
    a, b, tied = gh.shuffled_equidistant()
    ii, jj, rec = ref.considered(a, b, 8 / 64)
    assert len(ii) == 5 * 24 and (rec["dist"] == F32(8 / 64)).all() and (rec["hit"] == 0).all()
    for q in range(24):
        assert np.array_equal(np.sort(jj[ii == q]), tied[q])
    want = ref.clearances(a, b, 8 / 64)
    assert np.array_equal(want["poly"], tied.min(axis=1))
    assert (ref.clearances(a, b, float(np.nextafter(F32(8 / 64), F32(0))))["poly"] == NO_POLY).all()
    a, b = gh.overlapping_three()
    want = ref.clearances(a, b, 1.0)
    assert np.array_equal(want["poly"], 4 * np.arange(6) + 1) and (want["hit"] == 1).all()
    ii, jj, rec = ref.considered(a, b, 1.0)
    assert np.array_equal(np.bincount(ii), np.full(6, 4)) and (rec["hit"] == 1).sum() == 18 and (rec["dist"][rec["hit"] == 0] == F32(1 / 256)).all()


def test_near_ties_hold_two_d2_that_round_to_one_dist_with_the_nearer_behind():
    """clearance_cases.slid_near_ties, as built or reversed: some query's smallest dist is shared by two obstacles of which the one
    at the LARGER index has the smaller d2.  A reduction that compares d2 picks it; the contract picks the smaller index."""
    found = 0
    for theta in cases.NEAR_TIE_THETAS:
        for offset in cases.NEAR_TIE_OFFSETS:
            _, _, D = ch.near_tie_records(theta, offset)
            d2, bits = gh.record_d2(D), np.ascontiguousarray(D["dist"]).view(np.uint32)
            assert np.array_equal(np.sqrt(d2), D["dist"]), "the record's points give its own d2"
            for order in (np.arange(130), np.arange(130)[::-1]):
                b_, d_ = bits[:, order], d2[:, order]
                first = b_.argmin(axis=1)
                rows = np.arange(64)
                later_tied = (b_ == b_[rows, first][:, None]) & (np.arange(130)[None, :] > first[:, None]) & (d_ < d_[rows, first][:, None])
                found += int(later_tied.any(axis=1).sum())
    assert found >= 4, found
