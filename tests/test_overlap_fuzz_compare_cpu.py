"""CPU test of the judge of tests/tools/overlap_fuzz.py — compare() of pair_list_fuzz.py on the row of tests/overlap_query.py — in
the manner of tests/test_fuzz_compare_cpu.py: it is fed a correct answer, which it must accept, and then one wrong bit in one answer
field at a time, each of which it must reject."""
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import contact_cases  # noqa: E402
import overlap_ref  # noqa: E402
from overlap_query import OVERLAPS  # noqa: E402


@pytest.fixture(scope="module")
def mf(pkg):
    spec = importlib.util.spec_from_file_location("pair_list_fuzz", os.path.join(HERE, "tools", "pair_list_fuzz.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def case(wl):
    """a reference answer with overlaps, misses and one bad entry"""
    a, b = contact_cases.dense_poly_sets(wl, n=40, extent=3.0)
    pairs = contact_cases.all_pairs(a[0].shape[1], b[0].shape[1])[::23].astype(np.int64)
    pairs[5, 0] = a[0].shape[1] + 2            # out of its set: BAD_PAIR
    want = overlap_ref.poly_overlaps(a, b, pairs[:, 0], pairs[:, 1])
    assert (want["area"] > 0).sum() > 5 and (want["hit"] == 0).sum() > 5 and ((want["flags"] & overlap_ref.BAD_PAIR) != 0).sum() == 1
    return want


def answer(mf, want, capacity, bound):
    w = want[:bound].copy()
    dt = OVERLAPS.dts[0]
    buf = np.frombuffer(bytes([mf.BAND]) * ((capacity + 2 * mf.GUARD) * dt.itemsize), dt).copy()
    buf[mf.GUARD: mf.GUARD + bound] = w
    return [buf, bool((w["flags"] & overlap_ref.BAD_PAIR).any()), True, w, capacity]


def judge(mf, args):
    return mf.compare(OVERLAPS, args[:1], args[1], args[2], args[3:4], args[4])


def test_judge_accepts_a_correct_answer(mf, case):
    n = len(case)
    for capacity, bound in ((n, n), (n + 3, n), (n, n - 9), (n, 5), (n, 0)):
        args = answer(mf, case, capacity, bound)
        assert args[1] == (bound > 5) and judge(mf, args) == []


@pytest.mark.parametrize("field", ["area", "iou", "cx", "cy", "area_a", "area_b", "hit", "flags", "pieces_a", "pieces_b", "reserved"])
def test_judge_rejects_one_wrong_bit(mf, case, field):
    """the lowest bit of one field of one record with a positive area (the floats: one ulp)"""
    n, G = len(case), mf.GUARD
    q = int(np.flatnonzero((case["area"] > 0) & (case["cx"] != 0) & (case["cy"] != 0))[0])
    args = answer(mf, case, n, n)
    assert judge(mf, args) == []
    one = args[0][field][G + q: G + q + 1]
    one.view(np.uint32 if one.dtype.itemsize == 4 else np.uint8)[0] ^= 1
    assert judge(mf, args) != [], field


def test_judge_rejects_a_signed_zero_a_band_byte_and_a_wrong_report(mf, case):
    n, G = len(case), mf.GUARD
    miss = int(np.flatnonzero(case["hit"] == 0)[0])

    def minus_zero(a):          # the records are compared byte for byte: -0 is not +0
        a[0]["area"][G + miss] = -0.0

    def band(record):
        def plant(a):
            a[0].view(np.uint8).reshape(len(a[0]), -1)[record, 3] = 0
        return plant

    for plant in [minus_zero, lambda a: a.__setitem__(1, False), lambda a: a.__setitem__(2, False)] + [band(r) for r in (0, G - 1, G + n, G + n + G - 1)]:
        args = answer(mf, case, n, n)
        assert judge(mf, args) == []
        plant(args)
        assert judge(mf, args) != [], plant
    args = answer(mf, case, n, n - 9)          # a record at the device count's bound
    band(G + n - 9)(args)
    assert judge(mf, args) != []
