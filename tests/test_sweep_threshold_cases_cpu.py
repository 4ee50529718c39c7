"""CPU proof of the moving station scene (tests/sweep_threshold_cases.py) on the reference and on the numpy box rule alone: every
probe's row holds exactly its station's h hitters (plus the covers), none of them at t = 0; its swept box meets the boxes of exactly
the h + c objects of its pile (plus the covers), its box at rest meets none of them; and the stations are so far apart that the
cells a probe's query reads hold its own pile only."""
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sweep_broad_ref as ref  # noqa: E402
import sweep_threshold_cases as stc  # noqa: E402
import threshold_cases as tc  # noqa: E402

_spec = importlib.util.spec_from_file_location("poly_sweep_box", os.path.join(HERE, "tools", "poly_sweep_box.py"))
psb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(psb)


def meets(box, boxes):
    return (box[0] <= boxes[2]) & (boxes[0] <= box[2]) & (box[1] <= boxes[3]) & (boxes[1] <= box[3])


@pytest.mark.parametrize("covers", [0, 3])
def test_rows_sit_on_the_switches_through_motion_only(oracle, covers):
    a, b, ma, info = stc.moving_station_scene(covers=covers)
    h, c, owner = info["h"], info["c"], info["owner"]
    got = ref.pairs(a, b, ma, None)
    per_row = np.bincount(got[:, 0], minlength=len(h))
    assert np.array_equal(per_row, h + covers)
    assert (owner[got[:, 1]] == np.where(owner[got[:, 1]] < 0, -1, got[:, 0].astype(np.int64))).all(), "a probe reaches its own pile and the covers only"
    static = ref.static_pairs(oracle, a, b)
    assert (owner[static[:, 1]] == -1).all() and len(static) == covers * len(h), "at t = 0 a probe touches nothing but the covers"
    swept, ok_a = psb.poly_sweep_boxes(*a, ma)
    rest, _ = psb.poly_sweep_boxes(*a, None)
    boxes, ok_b = psb.poly_sweep_boxes(*b, None)
    assert ok_a.all() and ok_b.all()
    for s in range(len(h)):
        pile = owner == s
        assert meets(swept[:, s], boxes[:, pile]).all() and not meets(swept[:, s], boxes[:, owner >= 0][:, owner[owner >= 0] != s]).any()
        assert not meets(rest[:, s], boxes[:, owner >= 0]).any()
    assert int(pile.sum()) == h[-1] + c[-1]
    # the switches the rows straddle, and the isolation that makes "walked" the pile's size: a query reads at most three cells of at
    # most 1.25 box extents from its box's lower corner, far less than the distance to the next station
    assert {tc.SHORT_HITS, tc.SHORT_HITS + 1, tc.MID_HITS, tc.MID_HITS + 1} <= set(h.tolist())
    assert {tc.CANDIDATE_CAP, tc.CANDIDATE_CAP + 1} <= set((h + c).tolist())
    extent = float((swept[2] - swept[0]).max())
    d = info["centre"][:, :, None] - info["centre"][:, None, :]
    gap = np.hypot(d[0], d[1]) + np.eye(len(h)) * 1e9
    assert gap.min() > 4 * 1.25 * extent + stc.RUN
