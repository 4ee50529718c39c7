"""CPU self-test of the judge of tests/tools/cast_grid_fuzz.py, after tests/test_clearance_grid_fuzz_judge_cpu.py: configurations drawn
by the fuzzer's own generator, the reference's records taken as "what the GPU returned", and one fault planted at a time — a winner
swapped for an obstacle reached at the same time with a larger index, a miss turned into a hit, one float field off by an ulp.  The
judge must accept the unmodified records and name every planted fault.  No GPU is involved."""
import importlib.util
import os

import numpy as np

import cast_cases as cases
import cast_harness as ch
import cast_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("cast_grid_fuzz", os.path.join(HERE, "tools", "cast_grid_fuzz.py"))
fz = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fz)
F32 = np.float32


def ulp_off(x):
    return np.nextafter(F32(x), F32(np.inf)) if np.isfinite(x) else F32(0)


def test_the_judge_names_every_planted_fault(wl):
    judged = ulps = turned = orders = movers = 0
    for idx in range(16):
        c = fz.draw(wl, np.random.default_rng([97, idx]), idx)
        want = c["want"]
        orders += "B as drawn" not in c["what"]
        movers += "movers 0 / 0" not in c["what"]
        assert fz.judge(want.copy(), want) is None, c["what"]
        if idx < 6:
            again = fz.draw(wl, np.random.default_rng([97, idx]), idx)
            assert again["what"] == c["what"] and again["want"].tobytes() == want.tobytes(), "a configuration is a function of its seed"
        assert fz.judge(want[:-1], want) is not None
        miss = np.flatnonzero((want["hit"] == 0) & (want["flags"] == 0))
        if len(miss):                                          # a miss turned into a hit
            q = int(miss[idx % len(miss)])
            wrong = want.copy()
            wrong[q] = (c["cb"], 0.5, 1.0, 0.0, 1, 1, 0, 0)
            why = fz.judge(wrong, want)
            assert why is not None and f"query {q}" in why and "'poly'" in why and "'hit'" in why and "'toi'" in why, (c["what"], why)
            turned += 1
        win = np.flatnonzero(want["hit"] == 1)
        if len(win) == 0:
            continue
        judged += 1
        q = int(win[idx % len(win)])
        for f in ref.FLOATS:                                   # one float field off by an ulp
            wrong = want.copy()
            wrong[f][q] = ulp_off(want[f][q])
            why = fz.judge(wrong, want)
            assert why is not None and f"query {q}" in why and f"'{f}'" in why, (c["what"], f, why)
            ulps += 1
        for f, v in (("poly", want["poly"][q] ^ 1), ("hit", 0), ("flags", want["flags"][q] ^ 1), ("axis", want["axis"][q] ^ 1), ("reserved0", 1)):
            wrong = want.copy()
            wrong[f][q] = v
            assert f"'{f}'" in fz.judge(wrong, want), (c["what"], f)
    assert judged >= 8 and ulps >= 24 and turned >= 4 and orders >= 4 and movers >= 4, (judged, ulps, turned, orders, movers)


def test_a_winner_swapped_for_an_equal_time_larger_index_is_caught():
    """the exactly tied near-ties and the hit behind the graze: the record of the other obstacle at the same toi differs in `poly` (and
    where its face differs, in the normal) and the judge says so"""
    a, b, ma, S = ch.near_tie_records(cases.NEAR_TIE_THETAS[0], cases.NEAR_TIE_OFFSETS[0])
    want = ref.reduce(S, ref.bad_counts(a), ref.bad_counts(b))
    assert fz.judge(want.copy(), want) is None
    bits = np.ascontiguousarray(S["toi"]).view(np.uint32)
    tied = np.flatnonzero((bits == bits.min(axis=1)[:, None]).sum(axis=1) > 1)
    assert len(tied) >= 3
    for q in tied[:8]:
        later = np.flatnonzero(bits[q] == bits[q].min())[1]
        assert later > want["poly"][q] and S["toi"][q, later] == want["toi"][q]
        wrong = want.copy()
        for f in ref.COPIED:
            wrong[f][q] = S[f][q, later]
        wrong["poly"][q] = later
        why = fz.judge(wrong, want)
        assert why is not None and f"query {q}" in why and "'poly'" in why, why
    a, b, ma, mb, graze, miss, S = ch.graze_records()
    want = ref.reduce(S, ref.bad_counts(a), ref.bad_counts(b))
    wrong = want.copy()
    for f in ref.COPIED:
        wrong[f][5] = S[f][5, graze[5] + 1]
    wrong["poly"][5] = graze[5] + 1
    assert wrong["toi"][5] == want["toi"][5] and "'poly'" in fz.judge(wrong, want)
