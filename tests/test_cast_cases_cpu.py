"""CPU proof of the constructions that the GPU tests of the shape casts lean on: the finalise pass of c2d_poly_set_casts recomputes
the winner's record, so a wrong `hit` or a wrong last bit of `toi` in the main kernel shows only in WHO wins, and these inputs are
built so that it does.  Everything here is a condition on tests/cast_ref.py alone: with it the GPU tests cannot pass vacuously."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cast_cases as cases  # noqa: E402
import cast_harness as ch  # noqa: E402
import cast_ref as ref  # noqa: E402
import clearance_cases  # noqa: E402
import contact_cases  # noqa: E402

F = np.float32
HARD_NAMES = ["clockwise", "clockwise_both", "repeated_vertices", "k1_k2", "touching", "equal_shapes", "equal_boxes", "scale_1e30", "scale_1e-30",
              "scale_1e-42", "scale_1e18", "scale_1e-18", "non_finite_vertex0", "non_finite_later_vertex", "overflowing_len2"]


def test_every_hard_batch_is_named(wl):
    assert sorted(clearance_cases.witness_batches(wl)) == sorted(contact_cases.hard_poly_batches(wl)) == sorted(HARD_NAMES)


@pytest.mark.parametrize("name", HARD_NAMES)
def test_the_static_witness_shows_every_pairs_hit_at_zero(wl, name):
    """W stands still and starts in overlap with every query (key (+0, width - 1)), so in the shard [B_j x (width - 1), W] the winner
    is index 0 exactly when S(i, j) is a hit at toi = +0, and W otherwise; the motions are twice the batch's scale and finite"""
    a, b, w, layouts = clearance_cases.witness_batches(wl)[name]
    S, SW, (ma, mb) = ch.witness_records(wl, name)
    assert all(np.isfinite(m).all() for m in ma + mb)
    assert (SW["hit"] == 1).all() and (SW["toi"] == 0).all() and (SW["flags"] == cases.START_OVERLAP).all()
    n_b = b[0].shape[1]
    for layout, (s, width) in layouts.items():
        for j in range(n_b):
            want = ch.witness_reference(wl, name, layout, j)
            first = (S["hit"][:, j] == 1) & (S["toi"][:, j] == 0)
            assert np.array_equal(want["poly"] == width * j, first), (layout, j)
            assert np.array_equal(want["poly"] == width * j + width - 1, ~first) and (want["hit"] == 1).all(), (layout, j)


def test_the_witness_batches_hold_moving_hits_and_misses_too(wl):
    """over all batches: pairs that start in overlap, pairs that touch later in the step, and pairs that never do"""
    S = np.concatenate([ch.witness_records(wl, name)[0].ravel() for name in HARD_NAMES])
    start, later, miss = (S["flags"] == cases.START_OVERLAP).mean(), ((S["hit"] == 1) & (S["toi"] > 0)).mean(), (S["hit"] == 0).mean()
    print(f"start overlap {start:.3f}, touch later {later:.3f}, miss {miss:.3f}")
    assert start > 0.02 and later > 0.02 and miss > 0.02


@pytest.mark.parametrize("theta", cases.NEAR_TIE_THETAS)
def test_moving_slabs_tie_within_a_few_ulp(theta):
    """all 8 320 pairs of each scene hit with flags = 0 at about 1/2; at least half of the queries have their best exactly tied with,
    or 1..4 ulp ahead of, another obstacle; at theta 2.9 and the origin at least 40 % have a runner-up 1..4 ulp behind"""
    for offset in cases.NEAR_TIE_OFFSETS:
        a, b, ma, S = ch.near_tie_records(theta, offset)
        assert S.shape == (64, 130) and (S["hit"] == 1).all() and (S["flags"] == 0).all() and np.abs(S["toi"] - F(0.5)).max() < 1e-4
        close, near, beyond_tile_0 = cases.near_tie_shares(S)
        print(f"theta {theta}, offset {offset}: tied or within 4 ulp {close:.3f}, runner-up within 1..4 ulp {near:.3f}, winner beyond tile 0 {beyond_tile_0:.3f}")
        assert close >= 0.5, (theta, offset, close)
        if theta == 2.9 and offset == cases.NEAR_TIE_OFFSETS[0]:
            assert near >= 0.4, near
        assert len(np.unique(S["toi"])) > 4      # (rounding really tells the obstacles apart)
        # reversed, the smallest index of the best moves: another obstacle of the tied ones wins wherever the best is tied
        rev = ref.reduce(S[:, ::-1], ref.bad_counts(a), ref.bad_counts(b))
        fwd = ref.reduce(S, ref.bad_counts(a), ref.bad_counts(b))
        assert np.array_equal(rev["toi"], fwd["toi"])


def test_grazes_and_misses_by_one_grid_step():
    """per query: the pass one grid step too high (a smaller index) misses, the exact pass is a hit with toi = 1/2 and wins, the pass
    one step lower hits at the same 1/2 behind it; a kernel that drops t_out, or compares t_in < t_out, names another winner"""
    a, b, ma, mb, graze, miss, S = ch.graze_records()
    n = a[0].shape[1]
    q = np.arange(n)
    assert n >= 64 and (S["hit"][q, miss] == 0).all() and (S["hit"][q, graze] == 1).all() and (S["toi"][q, graze] == 0.5).all()
    assert (S["hit"][q, graze + 1] == 1).all() and (S["toi"][q, graze + 1] == 0.5).all() and (miss < graze).all()
    want = ref.reduce(S, ref.bad_counts(a), ref.bad_counts(b))
    assert np.array_equal(want["poly"], graze) and (want["flags"] == 0).all()
    # nothing else of the scene is reached by a query: per row exactly the two hits
    assert ((S["hit"] == 1).sum(axis=1) == 2).all()
