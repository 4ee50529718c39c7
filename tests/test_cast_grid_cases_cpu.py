"""What the constructions of tests/cast_grid_harness.py promise, proved on the reference alone (cast_ref, sweep_ref): the sparse
scene holds enough of each kind of record, the tie scenes really tie and their winner really depends on the order of B's indices,
the station scene has winners on both sides of the walk's cap, and the shortcut reference of that scene is cast_ref.casts.  No GPU."""
import numpy as np
import pytest

import cast_cases as cases
import cast_grid_harness as cg
import cast_harness as ch
import cast_ref as ref
import sweep_threshold_cases as stc

F32 = np.float32


@pytest.mark.parametrize("reach", cg.REACHES)
def test_the_sparse_scene_holds_every_kind_of_record(wl, reach):
    """cast_cases.scene(wl, 257, 1031, extent=160.0, reach): misses, start overlaps and moving hits are each at least 5 % of the
    queries (73 / 18 / 8.6 % at reach 2, 64 / 18 / 17.5 % at reach 6), for two sets"""
    a, b, ma, mb, S = cg.sparse(wl, reach)
    assert S.shape == (257, 1031)
    full = ref.reduce(S, ref.bad_counts(a), ref.bad_counts(b))
    miss, start, moving = cg.shares(full)
    print(f"reach {reach}: misses {miss:.3f}, start overlaps {start:.3f}, moving hits {moving:.3f}")
    assert min(miss, start, moving) >= 0.05, (miss, start, moving)
    assert len(np.unique(full["poly"])) > 40, "many different winners"


def test_the_one_set_scene_holds_every_kind_of_record(wl):
    s, ms, S = cg.own_set(wl)
    bad = ref.bad_counts(s)
    own = ref.reduce(S, bad, bad, flags=ref.SKIP_SELF)
    miss, start, moving = cg.shares(own)
    print(f"one set under SKIP_SELF: misses {miss:.3f}, start overlaps {start:.3f}, moving hits {moving:.3f}")
    assert min(miss, start, moving) >= 0.05 and (own["poly"] != np.arange(257)).all()
    plain = ref.reduce(S, bad, bad)
    assert (plain["flags"] == cases.START_OVERLAP).all() and (plain["poly"] <= np.arange(257)).all(), "without the flag every polygon overlaps itself"


def test_the_shortcut_reference_is_the_reference(wl):
    """cast_grid_harness.reference_by_hits against cast_ref.casts: on a part of the sparse scene with bases and SKIP_SELF, on the wild
    scene, and with the prefilter of sweep_broad_ref forced on"""
    a, b, ma, mb, S = cg.sparse(wl, 6.0)
    sa, sb = cg.take(a, np.arange(64)), cg.take(b, np.arange(300))
    sma, smb = cg.take_motion(ma, np.arange(64)), cg.take_motion(mb, np.arange(300))
    for kw in ({}, dict(row_base=3, col_base=1, flags=ref.SKIP_SELF), dict(col_base=(1 << 32) - 300)):
        want = ref.reduce(S[:64, :300], ref.bad_counts(sa), ref.bad_counts(sb), **kw)
        assert cg.reference_by_hits(sa, sb, sma, smb, **kw).tobytes() == want.tobytes(), kw
    wa, wb, wma, wmb = cg.wild_scene(wl)
    with np.errstate(all="ignore"):
        want = ref.casts(wa, wb, wma, wmb)
    assert ref.same(cg.reference_by_hits(wa, wb, wma, wmb), want).all()
    assert (want["flags"][[60, 61, 62]] == cases.BAD_PAIR).all() and not np.isin(want["poly"], [63, 64, 65]).any()
    miss, start, moving = cg.shares(want)
    assert miss > 0.05 and start > 0.05 and moving > 0.05, (miss, start, moving)
    assert want["hit"][10] == 1 and want["toi"][10] == 0 and want["axis"][10] == ref.NONE16, "a NaN motion: a hit at +0 with no axis"


@pytest.mark.parametrize("theta", cases.NEAR_TIE_THETAS)
def test_the_permuted_near_ties_really_tie(theta):
    """moving_near_ties: for a majority of the queries the best is tied with, or within 4 ulp of, another obstacle; where it is exactly
    tied, dealing B's indices in another order moves the win to another obstacle of the tie, at the same time to the bit"""
    offset = cases.NEAR_TIE_OFFSETS[0]
    a, b, ma, S = ch.near_tie_records(theta, offset)
    close, _, _ = cases.near_tie_shares(S)
    assert close > 0.5, close
    bad_a, bad_b = ref.bad_counts(a), ref.bad_counts(b)
    fwd = ref.reduce(S, bad_a, bad_b)
    moved = 0
    for name, ib in cg.deals(130).items():
        got = ref.reduce(S[:, ib], bad_a, bad_b[ib])
        assert np.array_equal(got["toi"].view(np.uint32), fwd["toi"].view(np.uint32)), name
        moved += int((ib[got["poly"]] != fwd["poly"]).sum())          # the winner, as an obstacle of the set as built
    bits = np.ascontiguousarray(S["toi"]).view(np.uint32)
    exact = int(((bits == bits.min(axis=1)[:, None]).sum(axis=1) > 1).sum())
    print(f"theta {theta}: {close:.3f} within 4 ulp, {exact} queries exactly tied, {moved} wins moved by the deals")
    assert (exact > 0) == (moved > 0)
    if theta == cases.NEAR_TIE_THETAS[0]:
        assert exact > 0, "at least one scene has exact ties"


def test_in_the_permuted_grazes_the_graze_wins_over_the_later_hit():
    a, b, ma, mb, graze, miss, S = ch.graze_records()
    n = a[0].shape[1]
    bad_a, bad_b = ref.bad_counts(a), ref.bad_counts(b)
    fwd = ref.reduce(S, bad_a, bad_b)
    assert np.array_equal(fwd["poly"], graze) and (fwd["toi"] == 0.5).all(), "as built the graze wins over the hit behind it"
    for name, ib in cg.deals(3 * n).items():
        where = np.argsort(ib)                                        # where each original obstacle went
        got = ref.reduce(S[:, ib], bad_a, bad_b[ib])
        assert np.array_equal(got["poly"], np.minimum(where[graze], where[graze + 1])) and (got["toi"] == 0.5).all(), name
        assert not np.isin(got["poly"], where[miss]).any(), name
    rev = ref.reduce(S[:, ::-1], bad_a, bad_b[::-1])
    assert np.array_equal(3 * n - 1 - rev["poly"].astype(np.int64), graze + 1), "reversed, the later hit wins"


def test_overlaps_beside_a_later_hit_at_a_smaller_index():
    a, b, ma = cg.overlaps_beside_a_later_hit()
    n = a[0].shape[1]
    S = ref.pair_records(a, b, ma, None)
    q = np.arange(n)
    assert (S["hit"][q, 4 * q] == 1).all() and (S["toi"][q, 4 * q] == F32(1 / 256)).all(), "the smaller index is reached later"
    for r in (1, 2, 3):
        assert (S["flags"][q, 4 * q + r] == cases.START_OVERLAP).all() and (S["toi"][q, 4 * q + r] == 0).all()
    want = ref.reduce(S, ref.bad_counts(a), ref.bad_counts(b))
    assert np.array_equal(want["poly"], 4 * q + 1) and (want["toi"] == 0).all()
    # a kernel that compares times alone, or skips on gj >= K, names one of these instead
    assert ((S["hit"] == 1).sum(axis=1) == 4).all()


def test_ties_across_cells_tie_exactly():
    a, b, ma, tied = cg.ties_across_cells()
    n = a[0].shape[1]
    S = ref.pair_records(a, b, ma, None)
    q = np.arange(n)
    for side in (0, 1):
        assert (S["hit"][q, tied[:, side]] == 1).all() and (S["toi"][q, tied[:, side]] == 0.5).all() and (S["flags"][q, tied[:, side]] == 0).all()
    far = 9 * q + 3 - tied.sum(axis=1)                                # the third index of the station
    assert (S["hit"][q, far] == 1).all() and (S["toi"][q, far] == 0.75).all()
    assert ((S["hit"] == 1).sum(axis=1) == 3).all(), "a query reaches its own three obstacles and nothing else"
    want = ref.reduce(S, ref.bad_counts(a), ref.bad_counts(b))
    assert np.array_equal(want["poly"], tied.min(axis=1)) and (want["toi"] == 0.5).all()
    assert (tied[:, 0] > tied[:, 1]).sum() == 3 and (far < tied.min(axis=1)).sum() == 2, "both orders of the tie, and the later hit in front of both"
    # the cell size is 1: more than four boxes have an extent in [7/8, 1), none a larger one (the queries' swept boxes are 48 steps)
    extent = np.maximum(b[0][:4].max(axis=0) - b[0][:4].min(axis=0), b[1][:4].max(axis=0) - b[1][:4].min(axis=0))
    assert ((extent >= 0.875) & (extent < 0.99)).sum() > 4 and extent.max() < 0.99
    # R's and U's minimum corners are more than a cell apart in x and in y, R's in the lower cell row
    lo_x, lo_y = b[0][:4].min(axis=0), b[1][:4].min(axis=0)
    assert (lo_x[tied[:, 0]] - lo_x[tied[:, 1]] > 1.05).all() and (lo_y[tied[:, 1]] - lo_y[tied[:, 0]] > 1.05).all()


def test_the_station_scene_has_winners_on_both_sides_of_the_cap():
    """sweep_threshold_cases.moving_station_scene: probes whose walk is 1024 entries (the last the row kernel keeps) and 1025 (the
    list kernel), each with and without obstacles that it reaches; every winner is of the probe's own pile"""
    a, b, ma, info = stc.moving_station_scene()
    walked, hitters = info["h"] + info["c"], info["h"]
    want = cg.reference_by_hits(a, b, ma, None)
    won = want["poly"] != ref.NO_POLY
    assert np.array_equal(won, hitters > 0)
    assert (info["owner"][want["poly"][won]] == np.flatnonzero(won)).all()
    for cap_side in (cg.CANDIDATE_CAP, cg.CANDIDATE_CAP + 1):
        at = walked == cap_side
        assert (at & won).sum() >= 2 and (at & ~won).sum() >= 1, cap_side
    assert (want["toi"][won] > 0).all() and (want["toi"][won] < 1).all(), "every winner is reached in motion"
    covered = stc.moving_station_scene(covers=3)
    wc = cg.reference_by_hits(covered[0], covered[1], covered[2], None)
    assert (wc["flags"] == cases.START_OVERLAP).all() and (covered[3]["owner"][wc["poly"]] == -1).all(), "under covers every probe starts in overlap"
