"""CPU self-test of the judge of tests/tools/near_broad_fuzz.py: configurations drawn by the fuzzer's own generator, the reference's
list taken as "what the GPU returned", and one fault planted at a time — a pair dropped, a separated pair dropped, an extra pair
whose distance lies within one ulp above the margin, two entries exchanged, a total that is off by one, a list cut short.  The judge
(pair_search_harness.compare) must accept the unmodified list and name every planted fault.  No GPU is involved."""
import importlib.util
import os

import numpy as np

import near_broad_harness as nh
import pair_search_harness as psh

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("near_broad_fuzz", os.path.join(HERE, "tools", "near_broad_fuzz.py"))
fz = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fz)
ref = fz.ref
F32 = np.float32


def test_the_judge_names_every_planted_fault():
    seen_apart = judged = 0
    for idx in range(16):
        c = fz.draw(np.random.default_rng([79, idx]), idx, small=True)
        want, a, b = c["want"], c["a"], c["b"]
        assert psh.compare(want.copy(), len(want), want) is None, c["what"]
        if idx < 8:
            again = fz.draw(np.random.default_rng([79, idx]), idx, small=True)
            assert again["what"] == c["what"] and np.array_equal(again["want"], want), "a configuration is a function of its seed"
        if len(want) < 2:
            assert psh.compare(want, len(want) + 1, want) is not None
            continue
        judged += 1
        rng = np.random.default_rng(idx)
        q = int(rng.integers(0, len(want)))
        dropped = np.delete(want, q, axis=0)
        assert "total" in psh.compare(dropped, len(dropped), want)             # a dropped pair changes the total, which is named first
        other = want[0:1] if q else want[1:2]                                  # the same total: the dropped pair's place taken by a repeat
        assert "1 pairs missing" in psh.compare(np.concatenate([dropped, other]), len(want), want)
        swapped = want.copy()
        swapped[[0, 1]] = swapped[[1, 0]]
        assert "another order" in psh.compare(swapped, len(want), want)
        assert "total" in psh.compare(want, len(want) + 1, want) and "total" in psh.compare(want, len(want) - 1, want)
        assert "written" in psh.compare(want[:-1], len(want), want)
        # a pair that is listed through the margin alone: the fault a broad phase on boxes without the margin would make
        ii, jj = want[:, 0].astype(np.int64), want[:, 1].astype(np.int64)
        with np.errstate(all="ignore"):
            apart = np.flatnonzero(ref.records(a, b, ii, jj)["hit"] == 0)
        if apart.size:
            seen_apart += 1
            m = int(apart[0])
            assert psh.compare(np.delete(want, m, axis=0), len(want) - 1, want) is not None
            assert "missing" in psh.compare(np.concatenate([np.delete(want, m, axis=0), want[m - 1:m] if m else want[1:2]]), len(want), want)
        # a pair the reference does not list
        listed = set(map(tuple, want.tolist()))
        n_a, n_b = a[0].shape[1], b[0].shape[1]
        extra = next(((i, j) for i in range(n_a) for j in range(n_b) if (i, j) not in listed), None)
        if extra is not None:
            plus = np.concatenate([want, np.array([extra], np.uint32)])
            plus = plus[np.lexsort((plus[:, 1], plus[:, 0]))]
            assert "total" in psh.compare(plus, len(plus), want)
            at = int(np.flatnonzero((plus == np.array(extra, np.uint32)).all(1))[0])
            swap = np.delete(plus, at - 1 if at else 1, axis=0)                # the same total: the extra pair in a listed pair's place
            assert "; 1 extra" in psh.compare(swap, len(want), want)
    assert judged >= 6 and seen_apart >= 3, (judged, seen_apart)


def test_an_extra_pair_one_ulp_beyond_the_margin_is_caught():
    """two squares 8 / 64 apart: listed at max_dist = 8 / 64, not listed at the float below it; a kernel that lists the pair there
    (comparing d2 with r * r, a rounded root, a box rule without strictness) returns a list the judge rejects as holding an extra pair"""
    a, b = nh.grid_boxes([(8, 0), (3, 4), (1, 0)])
    at = F32(8 / 64)
    below = np.nextafter(at, F32(0))
    want_at, want_below = ref.pairs(a, b, at), ref.pairs(a, b, below)
    assert [0, 0] in want_at.tolist() and [0, 0] not in want_below.tolist() and len(want_at) == len(want_below) + 1
    assert psh.compare(want_below, len(want_below), want_below) is None
    why = psh.compare(want_at, len(want_at), want_below)
    assert why is not None and "total" in why
    at = want_at.tolist().index([0, 0])
    why = psh.compare(np.delete(want_at, at + 1, axis=0), len(want_below), want_below)     # the same total, one pair exchanged for the extra one
    assert why is not None and "; 1 extra" in why
