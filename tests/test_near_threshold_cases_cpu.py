"""CPU proof of the near station scene (tests/near_threshold_cases.py) on the judge and on the numpy box rule alone: every probe's row
holds exactly its station's h neighbours (plus the covers), none of them a static hit; its box under the margin meets the boxes of
exactly the h + c objects of its pile; and the stations are so far apart that the cells a
probe's query reads hold its own pile only."""
import importlib.util
import os

import numpy as np
import pytest

import near_broad_ref as ref
import near_threshold_cases as ntc
import threshold_cases as tc

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("poly_near_box", os.path.join(HERE, "tools", "poly_near_box.py"))
pnb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(pnb)


def meets(box, boxes):
    return (box[0] <= boxes[2]) & (boxes[0] <= box[2]) & (box[1] <= boxes[3]) & (boxes[1] <= box[3])


@pytest.mark.parametrize("covers", [0, 3])
def test_rows_sit_on_the_switches_through_the_margin_only(covers):
    a, b, info = ntc.near_station_scene(covers=covers)
    h, c, owner = info["h"], info["c"], info["owner"]
    got = ref.pairs(a, b, ntc.MARGIN)
    per_row = np.bincount(got[:, 0], minlength=len(h))
    assert np.array_equal(per_row, h + covers)
    assert (owner[got[:, 1]] == np.where(owner[got[:, 1]] < 0, -1, got[:, 0].astype(np.int64))).all(), "a probe lists its own pile and the covers only"
    rec = ref.records(a, b, got[:, 0].astype(np.int64), got[:, 1].astype(np.int64))
    assert np.array_equal(rec["hit"] == 1, owner[got[:, 1]] < 0), "a probe hits nothing but the covers"
    assert len(ref.pairs(a, b, 0.0)) == covers * len(h), "without the margin a probe lists nothing but the covers"
    wide, ok_a = pnb.poly_near_boxes(*a, ntc.MARGIN)
    boxes, ok_b = pnb.poly_near_boxes(*b, ntc.MARGIN)
    assert ok_a.all() and ok_b.all()
    for s in range(len(h)):
        pile = owner == s
        assert meets(wide[:, s], boxes[:, pile]).all() and not meets(wide[:, s], boxes[:, owner >= 0][:, owner[owner >= 0] != s]).any()
    assert int(pile.sum()) == h[-1] + c[-1]
    assert {0, 1, 15, tc.SHORT_HITS, tc.SHORT_HITS + 1, tc.MID_HITS, tc.MID_HITS + 1} <= set(h.tolist())
    assert {tc.CANDIDATE_CAP - 1, tc.CANDIDATE_CAP, tc.CANDIDATE_CAP + 1, tc.CANDIDATE_CAP + 2} <= set((h + c).tolist())
    extent = float((wide[2] - wide[0]).max())
    d = info["centre"][:, :, None] - info["centre"][:, None, :]
    gap = np.hypot(d[0], d[1]) + np.eye(len(h)) * 1e9
    assert gap.min() > 4 * 1.25 * extent + 2 * ntc.MARGIN
