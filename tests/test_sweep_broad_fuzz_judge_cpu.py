"""CPU self-test of the judge of tests/tools/sweep_broad_fuzz.py: configurations drawn by the fuzzer's own generator, the reference's
list taken as "what the GPU returned", and one fault planted at a time — a pair dropped, a pair that only touches in motion
dropped, a static pair added that never touches, two entries exchanged, a total that is off by one, a list cut short.  The judge
(pair_search_harness.compare) must accept the unmodified list and name every planted fault.  No GPU is involved."""
import importlib.util
import os

import numpy as np

import pair_search_harness as psh

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("sweep_broad_fuzz", os.path.join(HERE, "tools", "sweep_broad_fuzz.py"))
fz = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fz)
ref, sweep_ref = fz.ref, fz.sweep_ref


def test_the_judge_names_every_planted_fault():
    seen_moving = judged = 0
    for idx in range(16):
        c = fz.draw(np.random.default_rng([77, idx]), idx, small=True)
        want, a, b = c["want"], c["a"], c["b"]
        assert psh.compare(want.copy(), len(want), want) is None, c["what"]
        if idx < 8:
            again = fz.draw(np.random.default_rng([77, idx]), idx, small=True)
            assert again["what"] == c["what"] and np.array_equal(again["want"], want), "a configuration is a function of its seed"
        if len(want) < 2:
            assert psh.compare(want, len(want) + 1, want) is not None
            continue
        judged += 1
        rng = np.random.default_rng(idx)
        q = int(rng.integers(0, len(want)))
        dropped = np.delete(want, q, axis=0)
        assert "missing" in psh.compare(dropped, len(dropped), want) or "total" in psh.compare(dropped, len(dropped), want)
        assert "1 pairs missing" in psh.compare(np.concatenate([dropped, want[-1:]]), len(want), want) or q == len(want) - 1
        swapped = want.copy()
        swapped[[0, 1]] = swapped[[1, 0]]
        assert "another order" in psh.compare(swapped, len(want), want)
        assert "total" in psh.compare(want, len(want) + 1, want) and "total" in psh.compare(want, len(want) - 1, want)
        assert "written" in psh.compare(want[:-1], len(want), want)
        # a pair that is apart at t = 0 and touches in motion: the fault a broad phase on boxes at rest would make
        ii, jj = want[:, 0].astype(np.int64), want[:, 1].astype(np.int64)
        with np.errstate(all="ignore"):
            moving = np.flatnonzero((sweep_ref.poly_sweeps(a, b, ii, jj, c["ma"], c["mb"])["flags"] & sweep_ref.START_OVERLAP) == 0)
        if moving.size:
            seen_moving += 1
            m = int(moving[0])
            assert psh.compare(np.delete(want, m, axis=0), len(want) - 1, want) is not None
            assert "missing" in psh.compare(np.concatenate([np.delete(want, m, axis=0), want[m - 1:m] if m else want[1:2]]), len(want), want)
        # a pair the reference does not list
        listed = set(map(tuple, want.tolist()))
        n_a, n_b = a[0].shape[1], b[0].shape[1]
        extra = next(((i, j) for i in range(n_a) for j in range(n_b) if (i, j) not in listed), None)
        if extra is not None:
            plus = np.concatenate([want, np.array([extra], np.uint32)])
            plus = plus[np.lexsort((plus[:, 1], plus[:, 0]))]
            assert "extra" in psh.compare(plus[:len(want)], len(want), want) or "total" in psh.compare(plus, len(plus), want)
            assert psh.compare(plus, len(plus), want) is not None
    assert judged >= 6 and seen_moving >= 3, (judged, seen_moving)
