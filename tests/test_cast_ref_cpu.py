"""CPU tests that pin tests/cast_ref.py — the numpy restatement of the shape-cast contract of include/c2d.h that the GPU tests compare
c2d_poly_set_casts with — on the hand cases of tests/cast_cases.py, whose expected values are exact in binary32, and on the
properties that make it "the reduction over sweep_ref.poly_sweeps and nothing else"."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cast_cases as cases  # noqa: E402
import cast_ref as ref  # noqa: E402
import sweep_ref  # noqa: E402

HAND = cases.hand_cases()


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(name):
    a, b, ma, mb, kw, expect = HAND[name]
    got = ref.casts(a, b, ma, mb, **kw)
    assert len(got) == a[0].shape[1] and (got["reserved0"] == 0).all()
    for f, v in expect.items():
        assert np.array_equal(got[f], np.array(v, got[f].dtype)), (name, f, got[f], v)


def test_the_cases_the_issue_names_are_all_there():
    assert len(HAND) >= 20 and {"no_obstacles", "only_the_self_pair", "bad_counts", "nan_motion", "all_misses", "the_diagonal_graze_is_a_hit",
                                "the_same_pass_a_little_steeper_misses", "b_moving_and_a_still"} <= set(HAND)


def test_the_record_is_the_winners_sweep_record(wl):
    """every winner's record is sweep_ref's record of the pair (i, winner), the winner is a hit, no considered hit has a smaller key,
    and a query without a winner has no considered hit at all"""
    a, b, ma, mb = cases.scene(wl, n_a=40, n_b=90, extent=40.0)
    b = tuple(x.copy() for x in b)
    b[2][[5, 50]] = [0, 17]
    for kw in ({}, dict(row_base=3, col_base=0, flags=ref.SKIP_SELF), dict(col_base=(1 << 32) - 90)):
        got = ref.casts(a, b, ma, mb, **kw)
        S = ref.pair_records(a, b, ma, mb)
        cb, rb = kw.get("col_base", 0), kw.get("row_base", 0)
        assert 0.1 < (got["hit"] == 1).mean() < 0.95
        for i in range(40):
            ok = ~ref.bad_counts(b) & (S["hit"][i] == 1)
            if kw.get("flags"):
                ok &= (rb + i) != cb + np.arange(90)
            if not ok.any():
                assert got[i].tolist() == (ref.NO_POLY, np.inf, 0.0, 0.0, ref.NONE16, 0, 0, 0)
                continue
            j = int(got["poly"][i]) - cb
            assert ok[j] and all(got[f][i].tobytes() == S[f][i, j].tobytes() for f in ref.COPIED)
            keys = [(float(S["toi"][i, c]), c) for c in np.flatnonzero(ok)]
            assert (float(S["toi"][i, j]), j) == min(keys)
    one = sweep_ref.poly_sweeps(a, b, [7], [int(got["poly"][7]) - ((1 << 32) - 90)], ma, mb)[0]
    assert one["toi"] == got["toi"][7] and one["axis"] == got["axis"][7]


def test_same_treats_the_two_zeros_alike_and_nothing_else():
    r = np.zeros(2, ref.CAST_DT)
    s = r.copy()
    s["nx"][0] = -0.0
    assert ref.same(r, s).all()
    s["toi"][1] = np.nextafter(np.float32(0), np.float32(1))
    assert ref.same(r, s).tolist() == [True, False]
    assert ref.CAST_DT.itemsize == 24 and ref.casts(cases.empty(), cases.polys(cases.box(0, 0))).shape == (0,)
