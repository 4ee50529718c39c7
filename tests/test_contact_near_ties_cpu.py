"""CPU conditions on the near-tie inputs of the contact tests (tests/contact_cases.py near_tie_*; the GPU runs them in
tests/test_gpu_contact_ties.py): measured with the contract's own float32 terms (contact_ref.poly_axis_terms / rect_axis_terms) the
batches fill every band of relative gap between the two best axes, and a numpy model of the kernel's first-pass DECISION
(c2d_contact.hip FastPick::decided) shows that the polygon batch is sharp enough: the shipped margin decides a
good share of it and never wrongly, a margin of 0 names a wrong axis on some pairs.  The model is for the inputs and the proof
only; what the GPU computes is compared with contact_ref alone."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contact_cases as cases  # noqa: E402
import contact_ref as ref  # noqa: E402
from contact_bands import BAND_NAMES, SHIPPED, band_shares, fast_pick_model, relative_gap  # noqa: E402

F = np.float32


@pytest.fixture(scope="module")
def poly_batch():
    a, b = cases.near_tie_poly_sets()
    n = a[0].shape[1]
    idx = np.arange(n)
    return a, b, ref.poly_axis_terms(a, b, idx, idx), ref.poly_contacts(a, b, idx, idx)


def test_axis_terms_are_the_rules_own(poly_batch):
    """the helper's terms reproduce the contacts: the first smallest usable d is the depth, its axis the axis"""
    a, b, terms, want = poly_batch
    d = np.where(terms["usable"], terms["d"], F(np.inf))
    first = np.argmin(d, axis=1)
    rows = np.arange(len(d))
    assert np.array_equal(d[rows, first], want["depth"]) and np.array_equal(terms["axis"][rows, first], want["axis"])
    assert terms["d"].dtype == F and terms["o"].dtype == F and terms["len2"].dtype == F
    assert terms["o"].shape == (len(want), 32)
    assert np.array_equal(terms["usable"].sum(axis=1), a[2].astype(np.int64) + b[2])      # no degenerate edge in this batch
    empty = (np.zeros((16, 0), F), np.zeros((16, 0), F), np.zeros(0, np.uint8))
    assert ref.poly_axis_terms(empty, b, [0], [0])["usable"].shape == (1, 0)
    out = ref.poly_axis_terms(a, b, [0, -1, 1], [0, 0, a[0].shape[1]])
    assert out["usable"][0].any() and not out["usable"][1:].any()


def test_poly_batch_fills_every_band(poly_batch):
    """about 20 000 colliding pairs (depth > 0.05); each band of relative gap between the two best float32 d holds at least 2 %;
    the winner is the earlier axis in about half of the pairs and an axis of A in about half; the third axis is 1e-3 away"""
    a, b, terms, want = poly_batch
    assert len(want) >= 20_000 and (want["hit"] == 1).all() and (want["flags"] == 0).all() and (want["depth"] > 0.05).all()
    assert a[2].min() == 3 and a[2].max() == 16 and b[2].min() == 3 and b[2].max() == 16
    shares = band_shares(terms)
    print("polygon batch, share per band:", dict(zip(BAND_NAMES, np.round(shares, 4))))
    assert (shares >= 0.02).all(), shares
    d = np.where(terms["usable"], terms["d"], F(np.inf)).astype(np.float64)
    order = np.argsort(d, axis=1, kind="stable")
    rows = np.arange(len(d))
    assert ((d[rows, order[:, 2]] - d[rows, order[:, 0]]) >= 0.99e-3 * d[rows, order[:, 0]]).all()
    other = np.where(order[:, 0] == np.argmin(d, axis=1), order[:, 1], order[:, 0])
    winner = np.argmin(d, axis=1)
    assert 0.35 < (winner < other).mean() < 0.65, (winner < other).mean()
    assert 0.35 < (want["axis"] < a[2]).mean() < 0.65, (want["axis"] < a[2]).mean()
    assert ((winner < 16) != (other < 16)).mean() > 0.25       # the two best axes on different polygons, and on the same one
    # the two best axes are not parallel: |n1 x n2| > 0.3 for the unit normals of the float32 edges the two slots name
    unit = []
    for slot in (winner, other):
        s, e = np.where(slot < 16, 0, 1), slot % 16
        vx, vy, k = np.where(s == 0, a[0][:, rows], b[0][:, rows]), np.where(s == 0, a[1][:, rows], b[1][:, rows]), np.where(s == 0, a[2], b[2])
        e1 = np.where(e + 1 < k, e + 1, 0)
        nx, ny = -(vy[e1, rows].astype(np.float64) - vy[e, rows]), vx[e1, rows].astype(np.float64) - vx[e, rows]
        unit.append((nx / np.hypot(nx, ny), ny / np.hypot(nx, ny)))
    cross = np.abs(unit[0][0] * unit[1][1] - unit[0][1] * unit[1][0])
    assert (cross > 0.3 * (1 - 1e-6)).all(), cross.min()


def test_box_and_quad_batches_are_near_tied():
    """The box batch probes the many-way tie, not the bands: a box's parallel edges tie to within rounding, so the two best d are
    mostly equal (about half of the pairs fall into band 0) and the pair takes the second pass, where eight near-tied axes in two
    directions are ranked.  The quad batch is the rectangle call's counterpart of the polygon batch and fills every band."""
    (pa, pb), (ra, rb) = cases.near_tie_box_sets()
    n = ra.shape[1]
    idx = np.arange(n)
    for q in range(4):      # the same boxes in both forms
        assert np.array_equal(pa[0][q], ra[2 * q]) and np.array_equal(pa[1][q], ra[2 * q + 1]) and np.array_equal(pb[0][q], rb[2 * q])
    for name, terms in (("boxes as polygons", ref.poly_axis_terms(pa, pb, idx, idx)), ("boxes as rectangles", ref.rect_axis_terms(ra, rb, idx, idx))):
        gap = relative_gap(terms)
        shares = band_shares(terms)
        print(name, "share per band:", dict(zip(BAND_NAMES, np.round(shares, 4))))
        assert terms["usable"].sum(axis=1).min() == 8 and (gap <= 2.0 ** -14).all(), name
        # four axes per direction, and the two directions near-tied: all eight d within 2^-14 of the smallest
        d = np.sort(terms["d"].astype(np.float64), axis=1)
        assert (d[:, 0] > 0.03).all() and ((d[:, 7] - d[:, 0]) <= 2.0 ** -14 * d[:, 0]).all(), name
        assert ((d[:, 7] - d[:, 0]) > 2.0 ** -20 * d[:, 0]).mean() > 0.2, name      # not only exact ties
    qa, qb = cases.near_tie_quad_sets()
    idx = np.arange(qa.shape[1])
    terms = ref.rect_axis_terms(qa, qb, idx, idx)
    want = ref.rect_contacts(qa, qb, idx, idx)
    shares = band_shares(terms)
    print("quads, share per band:", dict(zip(BAND_NAMES, np.round(shares, 4))))
    assert (shares >= 0.02).all(), shares
    assert (want["hit"] == 1).all() and (want["depth"] > 0.05).all() and (terms["usable"].sum(axis=1) == 8).all()
    for q in (qa, qb):      # no two parallel edges: the near-tie is between two directions, not an edge and its opposite
        ex, ey = np.roll(q[0::2], -1, axis=0) - q[0::2], np.roll(q[1::2], -1, axis=0) - q[1::2]
        ln = np.hypot(ex, ey)
        for x, y in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            assert (np.abs(ex[x] * ey[y] - ey[x] * ex[y]) > 0.19 * ln[x] * ln[y]).all()


def test_the_batch_can_see_a_missing_margin(poly_batch):
    """Over four perturbation seeds of the approximate reciprocal square root: with the shipped constants the model decides at
    least 10 % of the polygon batch and every decided pair names the reference's axis; with no margin at all it names another
    axis on at least 20 pairs."""
    a, b, terms, want = poly_batch
    for seed in (1, 2, 3, 4, 5):
        decided, axis, _ = fast_pick_model(terms, *SHIPPED, seed)
        wrong = decided & (axis != want["axis"])
        print(f"seed {seed}: shipped margin decides {decided.mean():.4f}, wrong {int(wrong.sum())}")
        assert decided.mean() >= 0.10, decided.mean()
        assert not wrong.any(), f"seed {seed}: the model with the shipped margin names a wrong axis on pair {int(np.flatnonzero(wrong)[0])}"
        bare, axis0, _ = fast_pick_model(terms, 0.0, 0.0, seed)
        wrong0 = bare & (axis0 != want["axis"])
        print(f"seed {seed}: no margin decides {bare.mean():.4f}, wrong {int(wrong0.sum())}")
        assert wrong0.sum() >= 20, int(wrong0.sum())


def test_window_edge_batches_cross_each_window(oracle, wl):
    """The scaled batches of test_gpu_contact_ties.py test_window_edges: for each edge of the first pass's window (len2 = 2^-100,
    |o| = 2^60, len2 = 2^100) at least one exponent k leaves between 5 % and 95 % of its pairs with an axis outside the window, so
    the crossing happens inside a batch, pair by pair."""
    for name, (a, b, pairs, k), axis_terms in (("polygons", cases.window_edge_poly_batch(wl), ref.poly_axis_terms),
                                               ("rectangles", cases.window_edge_rect_batch(oracle, wl), ref.rect_axis_terms)):
        assert sorted(set(k.tolist())) == sorted(cases.WINDOW_EDGE_K) and len(pairs) == len(k)
        len2_out, o_out = cases.outside_window(axis_terms(a, b, pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)))
        for window, ks, out in (("len2 = 2^-100", range(-54, -45), len2_out), ("|o| = 2^60", range(26, 33), o_out), ("len2 = 2^100", range(46, 55), len2_out)):
            shares = {kk: float(out[k == kk].mean()) for kk in ks}
            print(name, window, {kk: round(s, 3) for kk, s in shares.items()})
            assert any(0.05 <= s <= 0.95 for s in shares.values()), (name, window, shares)


def test_mixed_scale_batch_mixes_kinds_in_every_wave(wl):
    a, b, pairs, k = cases.mixed_scale_poly_batch(wl)
    terms = ref.poly_axis_terms(a, b, pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64))
    len2_out, o_out = cases.outside_window(terms)
    hard = len2_out | o_out
    assert not hard[k == 0].any() and hard[np.abs(k) == 60].all() and 0.05 < hard[k == 29].mean() < 0.95
    full = len(pairs) // 64 * 64
    per_wave = hard[:full].reshape(-1, 64).sum(axis=1)
    assert per_wave.min() >= 8 and per_wave.max() <= 60, (per_wave.min(), per_wave.max())      # hard and fast lanes in every wave
    assert (np.diff(pairs[:, 0].astype(np.int64)) >= 0).all() and len(set(k[:64].tolist())) == 11
