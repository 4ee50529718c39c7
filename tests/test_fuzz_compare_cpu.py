"""CPU test of the judges of the differential fuzzers (compare() of tests/tools/cross_fuzz.py — shared by poly_cross_fuzz.py —
broad_fuzz.py and pair_list_fuzz.py, the one of the four list-driven tools; and clearance_ref.same, the judge of clearance_fuzz.py): each is fed a correct answer, which it must accept, and then one planted fault at a time, each
of which it must reject.  A judge that lets a fault pass would turn every leg that relies on it green for nothing."""
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import clearance_cases  # noqa: E402
import clearance_ref  # noqa: E402
import contact_cases  # noqa: E402
import contact_ref  # noqa: E402
import distance_ref  # noqa: E402
import manifold_ref  # noqa: E402
import pair_list_harness as h  # noqa: E402


def tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def cf(pkg):
    return tool("cross_fuzz")


@pytest.fixture(scope="module")
def bf(pkg):
    return tool("broad_fuzz")


@pytest.fixture(scope="module")
def mf(pkg):
    return tool("pair_list_fuzz")


# ---- the mask and list judge of the two cross fuzzers -------------------------------------------------------------------------------
N_A, N_B, LD, RB, CB = 9, 70, 3, 10, 7             # two mask words per row (58 tail bits), one padding word, a diagonal shifted by 3


def cross_answer(cf, capacity, report=False):
    """what correct calls leave behind for a fixed 9 x 70 result under the upper rule -> (args of compare() as a list, keywords)"""
    ref = np.random.default_rng(5).random((N_A, N_B)) < 0.3
    want = ref & (np.arange(N_B)[None, :] > np.arange(N_A)[:, None] + 3)        # (the rule restated, not cf.expected's own word)
    assert np.array_equal(want, cf.expected(ref, True, RB, CB)) and np.array_equal(ref, cf.expected(ref, False, RB, CB))
    total = int(want.sum())
    assert total > 40
    mask = np.full((N_A + 2, LD), cf.SENTINEL, np.uint64)
    bits = np.zeros((N_A, 128), np.uint8)
    bits[:, :N_B] = want
    mask[1:-1, :2] = np.packbits(bits, axis=-1, bitorder="little").view(np.uint64)
    pairs = None
    if capacity is not None:
        pairs = np.full((capacity + 2 * cf.GUARD, 2), 0xA5A5A5A5, np.uint32)
        listed = (np.argwhere(want) + (RB, CB)).astype(np.uint32)
        n = min(capacity, total)
        pairs[cf.GUARD: cf.GUARD + n] = listed[:n]
    return [mask, total, pairs, total, 2 if report else 0, True, want, N_B], dict(row_base=RB, col_base=CB, capacity=capacity, expect_report=report)


def test_expected_states_the_upper_rule(cf):
    ref = np.ones((4, 5), bool)
    assert np.array_equal(cf.expected(ref, True, 0, 0), np.triu(ref, 1))
    assert np.array_equal(cf.expected(ref, True, 2, 0), np.triu(ref, 3)) and np.array_equal(cf.expected(ref, True, 0, 2), np.triu(ref, -1))
    assert not cf.expected(ref, True, (1 << 32) - 4, 0).any() and cf.expected(ref, True, 0, (1 << 32) - 5).all()
    assert cf.expected(ref, False, 9, 0).all()


@pytest.mark.parametrize("capacity", [None, 0, 17, "total", "more"])
def test_cross_judge_accepts_a_correct_answer(cf, capacity):
    total = cross_answer(cf, None)[0][1]
    capacity = {"total": total, "more": total + 5}.get(capacity, capacity)
    for report in (False, True):
        args, kw = cross_answer(cf, capacity, report)
        assert cf.compare(*args, **kw) == []
    args, kw = cross_answer(cf, capacity, True)
    kw["expect_report"] = None          # (a bad count in no tested pair: reported or not)
    assert cf.compare(*args, **kw) == []
    args[4] = 0
    assert cf.compare(*args, **kw) == []


def cross_faults(cf):
    """name -> (capacity, a function that plants the fault into the args of compare())"""
    def at(capacity, plant):
        return capacity, plant

    def flip(word_row, word, bit):
        def plant(a):
            a[0][word_row, word] ^= np.uint64(1 << bit)
        return plant

    want = cross_answer(cf, None)[0][6]
    total = int(want.sum())
    set_bit, clear_bit = np.argwhere(want)[3], np.argwhere(~want[:, :64])[-1]
    G = cf.GUARD

    def swap(a):
        a[2][[G + 4, G + 5]] = a[2][[G + 5, G + 4]]

    def past_capacity(a):
        a[2][G + 17] = (RB + 8, CB + 69)

    def behind_total(a):
        a[2][G + total] = (0, 0)

    def missing_last(a):
        a[2][G + total - 1] = 0xA5A5A5A5

    def missing_shifted(a):
        a[2][G + 6: G + total - 1] = a[2][G + 7: G + total].copy()
        a[2][G + total - 1] = 0xA5A5A5A5

    def in_front(a):
        a[2][G - 1, 1] = 0

    def set_item(k, v):
        def plant(a):
            a[k] = v
        return plant

    return {
        "a set bit cleared": at(None, flip(1 + set_bit[0], set_bit[1] // 64, int(set_bit[1]) % 64)),
        "a clear bit set": at(None, flip(1 + clear_bit[0], 0, int(clear_bit[1]))),
        "a tail bit set": at(None, flip(4, 1, N_B - 64)),
        "the last tail bit set": at(None, flip(N_A, 1, 63)),
        "a padding word written": at(None, flip(2, 2, 0)),
        "the front guard row written": at(None, flip(0, 1, 5)),
        "the back guard row written": at(None, flip(N_A + 1, 0, 0)),
        "the mask count one too many": at(None, set_item(1, total + 1)),
        "the mask count one too few": at(None, set_item(1, total - 1)),
        "the list total one too few": at(total, set_item(3, total - 1)),
        "the total depends on the capacity": at(17, set_item(3, 17)),
        "two list entries exchanged": at(total, swap),
        "an entry past the capacity": at(17, past_capacity),
        "an entry behind the total": at(total + 5, behind_total),
        "the last entry missing": at(total, missing_last),
        "an entry missing, the rest moved up": at(total, missing_shifted),
        "written in front of the list": at(total, in_front),
        "a missing error report": at(total, set_item(4, 0)),
        "one report for two calls": at(total, set_item(4, 1)),
        "check_async not clean": at(total, set_item(5, False)),
    }


@pytest.mark.parametrize("name", ["a set bit cleared", "a clear bit set", "a tail bit set", "the last tail bit set", "a padding word written",
                                  "the front guard row written", "the back guard row written", "the mask count one too many",
                                  "the mask count one too few", "the list total one too few", "the total depends on the capacity",
                                  "two list entries exchanged", "an entry past the capacity", "an entry behind the total", "the last entry missing",
                                  "an entry missing, the rest moved up", "written in front of the list", "a missing error report",
                                  "one report for two calls", "check_async not clean"])
def test_cross_judge_rejects_a_planted_fault(cf, name):
    capacity, plant = cross_faults(cf)[name]
    args, kw = cross_answer(cf, capacity, report="report" in name)
    assert cf.compare(*args, **kw) == []
    plant(args)
    assert cf.compare(*args, **kw) != [], name


def test_cross_judge_rejects_a_spurious_report(cf):
    args, kw = cross_answer(cf, 17)
    for reported in (1, 2):
        args[4] = reported
        assert cf.compare(*args, **kw) != []


def test_the_polygon_form_uses_the_same_judge(pkg, cf):
    pcf = tool("poly_cross_fuzz")           # (it loads a copy of cross_fuzz.py of its own)
    assert pcf.compare is pcf.cf.compare and pcf.compare.__code__.co_filename == cf.compare.__code__.co_filename


# ---- the list judge of the broad-phase fuzzer ---------------------------------------------------------------------------------------
def broad_answer(bf, capacity, total=60):
    listed = np.stack([np.arange(total) // 7, np.arange(total) % 7 + 100], axis=1).astype(np.uint32)
    buf = np.full((capacity + 2 * bf.GUARD, 2), 0xA5A5A5A5, np.uint32)
    n = min(capacity, total)
    buf[bf.GUARD: bf.GUARD + n] = listed[:n]
    return [buf.copy(), total, buf.copy(), total, capacity]


@pytest.mark.parametrize("capacity", [0, 20, 60, 65])
def test_broad_judge_accepts_a_correct_answer(bf, capacity):
    assert bf.compare(*broad_answer(bf, capacity)) == []
    assert bf.compare(*broad_answer(bf, capacity, total=0)) == []


def test_broad_judge_rejects_planted_faults(bf):
    G = bf.GUARD

    def swap(a):
        a[0][[G + 4, G + 5]] = a[0][[G + 5, G + 4]]

    def past_capacity(a):
        a[0][G + 20] = (2, 106)

    def missing(a):
        a[0][G + 6: G + 59] = a[0][G + 7: G + 60].copy()
        a[0][G + 59] = 0xA5A5A5A5

    def missing_last(a):
        a[0][G + 59] = 0xA5A5A5A5

    def count(a):
        a[1] += 1

    def in_front(a):
        a[0][0, 0] = 1

    def one_field(a):
        a[0][G + 11, 1] += 1

    def cross_wrote_past(a):            # (the reference call is held to its capacity too)
        a[2][G + 20] = (2, 106)

    for capacity, plant in ((60, swap), (20, past_capacity), (60, missing), (60, missing_last), (60, count), (20, count), (60, in_front),
                            (60, one_field), (20, cross_wrote_past), (65, lambda a: a[0].__setitem__(G + 62, 7))):
        args = broad_answer(bf, capacity)
        assert bf.compare(*args) == []
        plant(args)
        assert bf.compare(*args) != [], plant


# ---- the record judge of the list-driven fuzzers: on the manifolds' two outputs, then on the distances' one --------------------------
def judge(mf, args, query=h.MANIFOLDS):
    """compare() on args = [the buffer of each output, reported, clean, the wanted records of each output, capacity]"""
    n = len(query.dts)
    return mf.compare(query, args[:n], args[n], args[n + 1], args[n + 2: 2 * n + 2], args[2 * n + 2])


@pytest.fixture(scope="module")
def manifold_case(wl):
    """a reference answer with two-point manifolds, misses and one bad entry"""
    a, b = contact_cases.dense_poly_sets(wl, n=40, extent=3.0)
    pairs = contact_cases.all_pairs(a[0].shape[1], b[0].shape[1])[::23].astype(np.int64)
    pairs[5, 0] = a[0].shape[1] + 2            # out of its set: BAD_PAIR
    want = manifold_ref.poly_manifolds(a, b, pairs[:, 0], pairs[:, 1])
    assert (want[1]["count"] == 2).sum() > 5 and (want[0]["hit"] == 0).any() and ((want[0]["flags"] & contact_ref.BAD_PAIR) != 0).sum() == 1
    return want


def manifold_answer(mf, want, capacity, bound, drop_bad=False):
    wc, wm = want[0][:bound].copy(), want[1][:bound].copy()
    if drop_bad:
        wc, wm = np.delete(wc, 5), np.delete(wm, 5)
        bound -= 1
    bad = bool((wc["flags"] & contact_ref.BAD_PAIR).any())
    bufs = []
    for w, dt in zip((wc, wm), h.MANIFOLDS.dts):
        buf = np.frombuffer(bytes([mf.BAND]) * ((capacity + 2 * mf.GUARD) * dt.itemsize), dt).copy()
        buf[mf.GUARD: mf.GUARD + bound] = w
        bufs.append(buf)
    return [bufs[0], bufs[1], bad, True, wc, wm, capacity]


def test_manifold_judge_accepts_a_correct_answer(mf, manifold_case):
    n = len(manifold_case[0])
    for capacity, bound in ((n, n), (n + 3, n), (n, n - 9), (n, 5), (n, 0)):
        args = manifold_answer(mf, manifold_case, capacity, bound)
        assert args[2] == (bound > 5) and judge(mf, args) == []
    assert judge(mf, manifold_answer(mf, manifold_case, n, n, drop_bad=True)) == []
    args = manifold_answer(mf, manifold_case, n, n)          # +0 and -0 are equal, a NaN equals a NaN of another payload
    q = int(np.flatnonzero(args[1]["x1"][mf.GUARD:] == 0)[0]) + mf.GUARD
    args[1]["x1"][q] = -0.0
    assert judge(mf, args) == []


def test_manifold_judge_rejects_planted_faults(mf, manifold_case):
    n, G = len(manifold_case[0]), mf.GUARD
    two = int(np.flatnonzero(manifold_case[1]["count"] == 2)[0])

    def ulp(field, k):
        def plant(a):
            v = a[k][field][G + two: G + two + 1]
            assert np.isfinite(v).all() and v[0] != 0
            v.view(np.uint32)[0] += 1
        return plant

    def flag(a):
        a[1]["flags"][G + two] ^= manifold_ref.P0_CLIPPED

    def contact_flag(a):
        a[0]["flags"][G + two] ^= contact_ref.NO_AXIS

    def field(name, k, delta=1):
        def plant(a):
            a[k][name][G + two] += delta
        return plant

    def byte(k, record, value=0):
        def plant(a):
            a[k].view(np.uint8).reshape(len(a[k]), -1)[record, 3] = value
        return plant

    faults = [ulp(f, 1) for f in manifold_ref.FLOATS] + [ulp(f, 0) for f in ("depth", "nx", "ny")]
    faults += [flag, contact_flag, field("feature", 1), field("count", 1), field("reserved", 1), field("axis", 0), field("hit", 0)]
    faults += [byte(k, r) for k in (0, 1) for r in (0, G - 1, G + n, G + n + G - 1)]              # the bands of both buffers
    faults += [lambda a: a.__setitem__(2, False), lambda a: a.__setitem__(3, False)]              # a missing report; one that stays
    for plant in faults:
        args = manifold_answer(mf, manifold_case, n, n)
        assert judge(mf, args) == []
        plant(args)
        assert judge(mf, args) != [], plant
    for k in (0, 1):                                                                              # a record at the device count's bound
        args = manifold_answer(mf, manifold_case, n, n - 9)
        byte(k, G + n - 9)(args)
        assert judge(mf, args) != []
        args = manifold_answer(mf, manifold_case, n, n - 9)
        args[k][G + n - 10] = args[k][G + n - 11]                                                 # the last record inside it: compared
        assert judge(mf, args) != []
    args = manifold_answer(mf, manifold_case, n, n, drop_bad=True)                                # a spurious report
    args[2] = True
    assert judge(mf, args) != []


@pytest.fixture(scope="module")
def distance_case(wl):
    """a reference answer of a query with one output: separated pairs with their closest points, hits and one bad entry"""
    a, b = contact_cases.dense_poly_sets(wl, n=40, extent=3.0)
    pairs = contact_cases.all_pairs(a[0].shape[1], b[0].shape[1])[::23].astype(np.int64)
    pairs[5, 0] = a[0].shape[1] + 2            # out of its set: BAD_PAIR
    want = distance_ref.poly_distances(a, b, pairs[:, 0], pairs[:, 1])
    assert (want["hit"] == 0).sum() > 5 and (want["hit"] == 1).any() and ((want["flags"] & distance_ref.BAD_PAIR) != 0).sum() == 1
    return want


def distance_answer(mf, want, capacity, bound):
    w = want[:bound].copy()
    dt = h.DISTANCES.dts[0]
    buf = np.frombuffer(bytes([mf.BAND]) * ((capacity + 2 * mf.GUARD) * dt.itemsize), dt).copy()
    buf[mf.GUARD: mf.GUARD + bound] = w
    return [buf, bool((w["flags"] & distance_ref.BAD_PAIR).any()), True, w, capacity]


def test_single_output_judge_accepts_a_correct_answer(mf, distance_case):
    n = len(distance_case)
    for capacity, bound in ((n, n), (n + 3, n), (n, n - 9), (n, 5), (n, 0)):
        args = distance_answer(mf, distance_case, capacity, bound)
        assert args[1] == (bound > 5) and judge(mf, args, h.DISTANCES) == []


def test_single_output_judge_rejects_planted_faults(mf, distance_case):
    n, G = len(distance_case), mf.GUARD
    far = int(np.flatnonzero((distance_case["hit"] == 0) & (distance_case["flags"] & distance_ref.BAD_PAIR == 0))[0])

    def band_byte(record):
        def plant(a):
            a[0].view(np.uint8).reshape(len(a[0]), -1)[record, 3] = 0
        return plant

    def ulp(a):
        v = a[0]["dist"][G + far: G + far + 1]
        assert np.isfinite(v).all() and v[0] != 0
        v.view(np.uint32)[0] += 1

    def reserved(a):
        a[0]["reserved1"][G + far] = 1

    faults = [band_byte(r) for r in (0, G - 1, G + n, G + n + G - 1)] + [ulp, reserved, lambda a: a.__setitem__(1, False), lambda a: a.__setitem__(2, False)]
    for plant in faults:      # a band byte on either side, a one-ulp float, a reserved field, a missing report, one that stays
        args = distance_answer(mf, distance_case, n, n)
        assert judge(mf, args, h.DISTANCES) == []
        plant(args)
        assert judge(mf, args, h.DISTANCES) != [], plant
    args = distance_answer(mf, distance_case, n, n - 9)          # a record at the device count's bound
    band_byte(G + n - 9)(args)
    assert judge(mf, args, h.DISTANCES) != []


# ---- the record judge of the clearance fuzzer: clearance_ref.same -------------------------------------------------------------------
@pytest.fixture(scope="module")
def clearance_case(wl):
    """a reference answer with separated winners and their closest points, hits, a query with a bad count and one with nothing to consider"""
    a, b = clearance_cases.scene(wl, n_a=60, n_b=40, extent=12.0)
    a = tuple(x.copy() for x in a)
    a[2][7] = 0
    want = clearance_ref.clearances(a, b, row_base=3, col_base=5)
    want[11] = clearance_ref.clearances(a, clearance_cases.empty())[11]
    assert (want["hit"] == 1).sum() > 5 and ((want["hit"] == 0) & (want["poly"] != clearance_ref.NO_POLY)).sum() > 5
    assert want["flags"][7] == distance_ref.BAD_PAIR and want["flags"][11] == clearance_ref.NONE_FLAG
    want.setflags(write=False)
    return want


def test_clearance_judge_accepts_a_correct_answer(clearance_case):
    want = clearance_case
    assert clearance_ref.same(want.copy(), want).all() and len(clearance_ref.same(want[:0].copy(), want[:0])) == 0
    got = want.copy()                      # +0 and -0 are equal in every float, a hit's zeros and a separated winner's alike
    for f in clearance_ref.FLOATS:
        zero = np.flatnonzero(got[f] == 0)
        assert len(zero) > 0
        got[f][zero] = -0.0
        assert np.signbit(got[f][zero]).all() and not np.signbit(want[f][zero]).any()
    assert clearance_ref.same(got, want).all() and clearance_ref.same(want, got).all()


def test_clearance_judge_rejects_planted_faults(clearance_case):
    want = clearance_case
    far = int(np.flatnonzero((want["hit"] == 0) & (want["poly"] != clearance_ref.NO_POLY) & (want["ax"] != 0) & (want["ay"] != 0) & (want["bx"] != 0) & (want["by"] != 0))[0])
    hit = int(np.flatnonzero(want["hit"] == 1)[0])

    def ulp(f, step):
        def plant(g):
            v = g[f][far: far + 1]
            assert np.isfinite(v).all() and v[0] != 0
            v.view(np.int32)[0] += step
        return plant

    def field(name, q, value):
        def plant(g):
            assert g[name][q] != value
            g[name][q] = value
        return plant

    faults = [ulp(f, step) for f in clearance_ref.FLOATS for step in (1, -1)]
    faults += [field("poly", far, int(want["poly"][far]) + 1), field("poly", hit, int(want["poly"][hit]) - 1), field("poly", 11, 0), field("poly", 7, 5)]
    faults += [field("edge", far, int(want["edge"][far]) ^ 1), field("vert", far, int(want["vert"][far]) ^ 1), field("edge", hit, 0), field("vert", hit, 0)]
    faults += [field("hit", far, 1), field("hit", hit, 0), field("flags", far, int(want["flags"][far]) ^ distance_ref.INTERIOR),
               field("flags", far, int(want["flags"][far]) ^ distance_ref.EDGE_ON_B), field("flags", 7, 0), field("flags", 11, 0)]
    faults += [field("reserved0", far, 1), field("reserved0", hit, 0x8000), field("dist", hit, np.float32(1e-45)), field("dist", 11, np.float32(3e38))]
    for plant in faults:
        got = want.copy()
        assert clearance_ref.same(got, want).all()
        plant(got)
        ok = clearance_ref.same(got, want)
        assert (~ok).sum() == 1, plant      # the planted record, and no other
    got = want.copy()                       # a NaN where a number belongs is a difference
    got["dist"][far] = np.nan
    assert not clearance_ref.same(got, want)[far]
