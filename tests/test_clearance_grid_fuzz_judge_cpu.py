"""CPU self-test of the judge of tests/tools/clearance_grid_fuzz.py, after tests/test_near_broad_fuzz_judge_cpu.py: configurations
drawn by the fuzzer's own generator, the reference's records taken as "what the GPU returned", and one fault planted at a time — a
winner swapped for an obstacle at the same distance with a larger index, a NONE record turned into a winner just beyond the margin,
one float field off by an ulp.  The judge must accept the unmodified records and name every planted fault.  No GPU is involved."""
import importlib.util
import os

import numpy as np

import clearance_grid_harness as gh
import clearance_grid_ref as ref
import distance_ref as dref

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("clearance_grid_fuzz", os.path.join(HERE, "tools", "clearance_grid_fuzz.py"))
fz = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fz)
F32 = np.float32
NO_POLY = 0xFFFFFFFF


def ulp_off(x):
    return np.nextafter(F32(x), F32(np.inf)) if np.isfinite(x) else F32(0)


def test_the_judge_names_every_planted_fault():
    judged = ulps = 0
    for idx in range(16):
        c = fz.draw(np.random.default_rng([83, idx]), idx, small=True)
        want = c["want"]
        assert fz.judge(want.copy(), want) is None, c["what"]
        if idx < 8:
            again = fz.draw(np.random.default_rng([83, idx]), idx, small=True)
            assert again["what"] == c["what"] and again["want"].tobytes() == want.tobytes(), "a configuration is a function of its seed"
        assert fz.judge(want[:-1], want) is not None
        win = np.flatnonzero(want["poly"] != NO_POLY)
        if len(win) == 0:
            continue
        judged += 1
        q = int(win[idx % len(win)])
        for f in ("dist", "ax", "ay", "bx", "by"):             # one float field off by an ulp
            if want["hit"][q] == 1 and f != "dist":
                continue                                       # (a hit's points are +0: one ulp above is the smallest subnormal, still a difference)
            wrong = want.copy()
            wrong[f][q] = ulp_off(want[f][q])
            why = fz.judge(wrong, want)
            assert why is not None and f"query {q}" in why and f"'{f}'" in why, (c["what"], f, why)
            ulps += 1
        for f, v in (("poly", want["poly"][q] + 1), ("hit", 1 - want["hit"][q]), ("flags", want["flags"][q] ^ 2), ("edge", want["edge"][q] ^ 1)):
            wrong = want.copy()
            wrong[f][q] = v
            assert f"'{f}'" in fz.judge(wrong, want), (c["what"], f)
    assert judged >= 8 and ulps >= 10, (judged, ulps)


def test_a_winner_swapped_for_an_equal_distance_larger_index_is_caught():
    """shuffled_equidistant: five obstacles at the same distance; the record of any other of them differs in `poly` (and, for the
    ones in another direction, in the points) and the judge says so"""
    a, b, tied = gh.shuffled_equidistant()
    want = ref.clearances(a, b, 8 / 64)
    assert fz.judge(want.copy(), want) is None
    for q in (0, 7, 23):
        for j in tied[q][1:]:
            rec = dref.poly_distances(a, b, np.array([q]), np.array([int(j)]))[0]
            assert rec["dist"] == want["dist"][q], "the same distance"
            wrong = want.copy()
            for f in ref.cref.COPIED:
                wrong[f][q] = rec[f]
            wrong["poly"][q] = j
            why = fz.judge(wrong, want)
            assert why is not None and f"query {q}" in why and "'poly'" in why, why


def test_a_none_turned_into_a_winner_just_beyond_the_margin_is_caught():
    """the exact grid: at the float below a pair's distance the query gets NONE; the record the contract gives one float higher
    (what comparing d2 with r * r, a rounded root or a box rule without strictness would return) is rejected"""
    a, b, steps = gh.exact_grid()
    at = F32(8 / 64)
    want_below, want_at = ref.clearances(a, b, float(np.nextafter(at, F32(0)))), ref.clearances(a, b, float(at))
    assert want_below["poly"][0] == NO_POLY and want_at["poly"][0] == 0 and want_at["dist"][0] == at
    assert fz.judge(want_below.copy(), want_below) is None
    wrong = want_below.copy()
    wrong[0] = want_at[0]
    why = fz.judge(wrong, want_below)
    assert why is not None and "query 0" in why and "'poly'" in why and "'flags'" in why
    # and the other way round: a winner at exactly max_dist dropped
    wrong = want_at.copy()
    wrong[0] = want_below[0]
    assert "query 0" in fz.judge(wrong, want_at)
