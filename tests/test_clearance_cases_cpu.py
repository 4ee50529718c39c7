"""CPU proof of the constructions of tests/clearance_cases.py that the GPU tests of the clearance query lean on: the finalise pass of
c2d_poly_set_clearances recomputes the winner's record, so what the main kernel decided about a pair shows only in WHO wins, and
these inputs are built so that it always does.  Everything here is a condition on tests/clearance_ref.py alone: with it the GPU
tests cannot pass vacuously."""
import numpy as np
import pytest

import clearance_cases as cases
import clearance_harness as ch
import clearance_ref as ref
import contact_cases

F = np.float32
HARD_NAMES = ["clockwise", "clockwise_both", "repeated_vertices", "k1_k2", "touching", "equal_shapes", "equal_boxes", "scale_1e30", "scale_1e-30",
              "scale_1e-42", "scale_1e18", "scale_1e-18", "non_finite_vertex0", "non_finite_later_vertex", "overflowing_len2"]


def test_every_hard_batch_has_its_witness(wl):
    assert sorted(cases.witness_batches(wl)) == sorted(contact_cases.hard_poly_batches(wl)) == sorted(HARD_NAMES)


@pytest.mark.parametrize("name", HARD_NAMES)
def test_the_witness_is_a_hit_for_every_query(wl, name):
    """S = 4 c clamped to the largest float (the two non-finite batches hold 3e38: there 4 c overflows and the clamp decides); the
    witness is an axis-parallel box of that half side, and the reference calls it a hit for every query"""
    a, b, w, _ = cases.witness_batches(wl)[name]
    S = cases.witness_half_side(a, b)
    c = max(float(np.abs(x[np.isfinite(x)]).max()) for s in (a, b) for x in s[:2])
    assert np.isfinite(S) and S == float(F(min(4.0 * c, cases.FLT_MAX))) and (name.startswith("non_finite")) == (S == cases.FLT_MAX)
    assert w[2].tolist() == [4] and sorted(set(np.abs(w[0][:4, 0]).tolist() + np.abs(w[1][:4, 0]).tolist())) == [S]
    assert not ref.bad_counts(a).any() and not ref.bad_counts(b).any()
    D, DW = ch.witness_records(wl, name)
    assert DW.shape == (a[0].shape[1], 1) and (DW["hit"] == 1).all() and (DW["dist"] == 0).all()
    assert D.shape in ((48, 48), (100, 100)) and 0.005 < (D["hit"] == 1).mean() <= 1.0


@pytest.mark.parametrize("name", HARD_NAMES)
def test_the_winner_is_index_0_exactly_for_a_hit_or_dist_0(wl, name):
    """both layouts, every obstacle: poly == col_base  <=>  distance_ref says hit or dist == 0; otherwise the witness wins, as a hit"""
    a, b, w, layouts = cases.witness_batches(wl)[name]
    D, _ = ch.witness_records(wl, name)
    n_b = b[0].shape[1]
    for layout, (s, width) in layouts.items():
        assert width == cases.WITNESS_LAYOUTS[layout] + 1 and s[0].shape == (b[0].shape[0], width * n_b)
        for j in range(n_b):
            for p in range(3):      # the shard is [B_j x (width - 1), W], bit for bit (NaN included)
                assert s[p][..., width * j: width * j + width - 1].tobytes() == np.repeat(b[p][..., j:j + 1], width - 1, axis=-1).tobytes()
                assert s[p][..., width * j + width - 1].tobytes() == w[p][..., 0].tobytes()
            want = ch.witness_reference(wl, name, layout, j)
            first = (D["hit"][:, j] == 1) | (D["dist"][:, j] == 0)
            assert np.array_equal(want["poly"] == width * j, first), (layout, j)
            assert np.array_equal(want["poly"] == width * j + width - 1, ~first) and (want["hit"][~first] == 1).all(), (layout, j)
            assert np.array_equal(want["hit"] == 1, (D["hit"][:, j] == 1) | ~first)
    assert not ((D["hit"] == 0) & (D["dist"] == 0)).any(), "a separated pair at dist 0: say so in the docstrings before relying on it"


@pytest.mark.parametrize("theta", cases.NEAR_TIE_THETAS)
def test_slid_obstacles_tie_within_a_few_ulp(theta):
    """The shares the near-tie test needs, on the reference: at the origin at least a quarter of the queries have a runner-up
    1..4 ulp of dist behind their winner; at (100, -50) at least 60 % have their best exactly tied with another obstacle (the
    smallest index decides); no pair is a hit anywhere, and every distance is within 1e-4 of the exact 0.75."""
    for offset, least_near, least_tied in zip(cases.NEAR_TIE_OFFSETS, (0.25, 0.0), (0.0, 0.6)):
        a, b, D = ch.near_tie_records(theta, offset)
        assert a[0].shape == (16, 64) and b[0].shape == (16, 130) and D.shape == (64, 130)
        assert (D["hit"] == 0).all() and (D["flags"] & ref.dref.NO_CANDIDATE == 0).all() and np.abs(D["dist"] - F(0.75)).max() < 1e-4
        near, tied, beyond_tile_0 = cases.near_tie_shares(D["dist"])
        print(f"theta {theta}, offset {offset}: runner-up within 1..4 ulp {near:.3f}, exactly tied {tied:.3f}, winner beyond tile 0 {beyond_tile_0:.3f}")
        assert near >= least_near and tied >= least_tied, (theta, offset, near, tied)
        assert len(np.unique(D["dist"])) > 4      # (rounding really tells the obstacles apart)


def test_the_slides_keep_every_pentagon_over_its_slab():
    """in float64, before rotation: the pentagon's lowest vertex lies over the inside of every slab's top edge, 0.75 above it"""
    lo = min(x for x, _ in cases.PENTAGON) - 20.0
    hi = max(x for x, _ in cases.PENTAGON) + 20.0
    assert -30.0 + 3.0 < lo and hi < 30.0 - 3.0
    assert min(y for _, y in cases.PENTAGON) == 0.75 and max(y for _, y in cases.SLAB) == 0.0


def test_the_reference_indexed_by_query_is_the_reference(wl):
    """ch.indexed_reference picks once per distinct query beyond 2^22 pairs (the fuzzer's configurations between the strip
    extremes): the same records as the plain reduction, under SKIP_SELF with self pairs that are winners too"""
    a, b = cases.scene(wl, n_a=30, n_b=20, extent=6.0)
    rng = np.random.default_rng(9402)
    b = tuple(x.copy() for x in b)
    b[2][[3, 9]] = [0, 17]
    D = ref.pair_records(a, b)
    for n_a, n_b, rb, cb, flags in ((500, 90, 0, 0, 0), (500, 90, 0, 0, ref.SKIP_SELF), (300, 400, 7, 100, ref.SKIP_SELF), (200, 64, (1 << 32) - 200, (1 << 32) - 64, ref.SKIP_SELF)):
        ia, ib = rng.integers(0, 30, n_a), rng.integers(0, 20, n_b)
        kw = dict(row_base=rb, col_base=cb, flags=flags)
        plain = ch.indexed_reference(a, ia, b, ib, D=D, by_query=False, **kw)
        fast = ch.indexed_reference(a, ia, b, ib, D=D, by_query=True, **kw)
        assert plain.tobytes() == fast.tobytes(), (n_a, n_b, rb, cb, flags)
        assert ref.same(plain, ref.clearances(ch.take(a, ia), ch.take(b, ib), **kw)).all()
        if flags and n_b == 400:
            without = ch.indexed_reference(a, ia, b, ib, D=D, by_query=True, row_base=rb, col_base=cb)
            assert (without["poly"] != fast["poly"]).sum() > 0, "no self pair was a winner: the case does not bite"
