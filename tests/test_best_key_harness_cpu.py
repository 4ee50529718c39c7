"""CPU test of tests/best_key_harness.py itself, after tests/test_pair_search_harness_cpu.py: call(), twice(), the two comparisons, the
strip rule and the shared refusals carry the checks of all six best-key queries' tests, so a silent mistake there would remove that
coverage everywhere at once.  Planted faults on arrays of a few records; call() is driven by a stand-in engine whose device arrays
are numpy buffers and whose queries write records through the pointer they are handed."""
import ctypes as C
import re

import numpy as np
import pytest

import best_key_harness as best
import cast_ref
import clearance_ref
import pair_list_harness as h


class Status(Exception):
    status = -1


class HostArray:
    def __init__(self, eng, a):
        self.a, self.ptr, self.nbytes, self.freed = a, a.ctypes.data, a.nbytes, False
        eng.live.append(self)

    def get(self):
        return self.a.copy()

    def free(self):
        self.freed = True


def bytes_at(ptr, n):
    return np.frombuffer((C.c_ubyte * n).from_address(ptr), np.uint8)


def record(p, size):
    return (np.arange(size) + 7 * p) % 251


class HostEngine:
    """Its three queries write `n + more` records through `out`, a set being the number of its polygons.  reports: how many of the
    following synchronise / check_async calls raise status -1; stray: one more byte written that far from the output's begin;
    flip: the run (1, 2, ..) whose record 0 differs in one byte"""

    def __init__(self, reports=0, more=0, stray=None, flip=None):
        self.reports, self.more, self.stray, self.flip, self.live, self.runs = reports, more, stray, flip, [], 0

    def empty(self, shape, dtype):
        return HostArray(self, np.zeros(shape, dtype))

    def memset(self, d, value, nbytes):
        d.a.view(np.uint8).reshape(-1)[:nbytes] = value

    def synchronize(self):
        if self.reports:
            self.reports -= 1
            raise Status()

    check_async = synchronize

    def write(self, out, n, size):
        self.runs += 1
        for p in range(n + self.more):
            bytes_at(out + p * size, size)[:] = record(p, size)
        if self.stray is not None:
            bytes_at(out + self.stray, 1)[:] = 0
        if self.flip == self.runs:
            bytes_at(out + 3, 1)[:] ^= 1

    def poly_ray_casts(self, rays, n_rays, b, out, col_base=0):
        assert rays == "planes" and col_base == 9
        self.write(out, n_rays, 16)

    def poly_set_casts(self, a, b, a_motion=None, b_motion=None, row_base=0, col_base=0, flags=0, out=None):
        assert (a_motion, b_motion, col_base) == ("ma", None, 9)
        self.write(out, a, 24)

    def poly_set_clearances(self, a, b, out, row_base=0, col_base=0, flags=0):
        assert col_base == 9
        self.write(out, a, 32)


class Rays:
    ptrs = "planes"


N = 5
ARGS = {best.RAY_CASTS: (Rays, N, None), best.CASTS: (N, None, N, "ma"), best.CLEARANCES: (N, None, N)}     # the 16-, 24- and 32-byte record
THREE = sorted(ARGS, key=repr)


def run(q, eng, **kw):
    return best.call(q, eng, *ARGS[q], col_base=9, **kw)


@pytest.mark.parametrize("q", THREE, ids=repr)
def test_the_table_has_the_bindings_records(pkg, q):
    assert [x.dt.itemsize for x in best.QUERIES] == [16, 16, 32, 32, 24, 24] and q.dt.itemsize == {best.RAY_CASTS: 16, best.CASTS: 24, best.CLEARANCES: 32}[q]
    assert (best.RAY_CASTS.dt, best.CLEARANCES.dt, best.CASTS.dt) == (pkg.RAY_HIT_DT, pkg.CLEARANCE_DT, pkg.CAST_DT)
    for x in best.QUERIES:
        assert callable(getattr(pkg.Engine, x.method)) and (x.stats is None or callable(getattr(pkg.Engine, x.stats)))
        assert (x.sibling is None) == (x.stats is None) and (x.sibling is None or (x.sibling.dt, x.sibling.padded) == (x.dt, x.padded))


@pytest.mark.parametrize("q", THREE, ids=repr)
def test_a_clean_call_returns_the_records_between_the_bands(q):
    """the ray calls return the capacity's records and default to n; the others return the n records of max(n, 4)"""
    size = q.dt.itemsize
    for capacity in (None, N, N + 3):
        eng = HostEngine()
        got = run(q, eng, capacity=capacity)
        returned = N if q.padded or capacity is None else capacity
        raw = got.view(np.uint8).reshape(-1, size)
        assert got.dtype == q.dt and got.shape == (returned,) and (raw[N:] == h.BAND).all()
        assert all((raw[p] == record(p, size)).all() for p in range(N))
        assert len(eng.live) == 1 and eng.live[0].freed and eng.live[0].a.shape == ((N if capacity is None else capacity) + 2 * h.GUARD,)
    eng = HostEngine()
    args = (Rays, 1, None) if q is best.RAY_CASTS else (1, None, 1) + ARGS[q][3:]
    best.call(q, eng, *args, col_base=9)
    assert eng.live[0].a.shape == ((4 if q.padded else 1) + 2 * h.GUARD,)


@pytest.mark.parametrize("q", THREE, ids=repr)
def test_one_stray_write_raises_the_matching_assertion(q):
    size = q.dt.itemsize
    for fault, message in ((dict(stray=-1), "written outside the output"), (dict(stray=-size * h.GUARD), "written outside the output"),
                           (dict(stray=(N + 3) * size), "written outside the output"), (dict(stray=(N + 3 + h.GUARD) * size - 1), "written outside the output"),
                           (dict(more=1), "written at or beyond"), (dict(stray=(N + 3) * size - 1), "written at or beyond")):
        with pytest.raises(AssertionError, match=message):
            run(q, HostEngine(**fault), capacity=N + 3)
    with pytest.raises(AssertionError, match="written outside the output"):      # one record too many with no room behind n: the back band
        run(q, HostEngine(more=1), capacity=N)
    run(q, HostEngine(stray=N * size - 1), capacity=N + 3)                       # (a byte inside the n records is none)


@pytest.mark.parametrize("q", THREE, ids=repr)
def test_expect_error_wants_exactly_one_report(q):
    assert len(run(q, HostEngine(reports=1), expect_error=True)) == N
    with pytest.raises(pytest.fail.Exception, match="DID NOT RAISE"):            # a stand-in that reports nothing
        run(q, HostEngine(reports=0), expect_error=True)
    with pytest.raises(Status):                                                  # one that goes on reporting
        run(q, HostEngine(reports=2), expect_error=True)
    with pytest.raises(Status):                                                  # and without expect_error a report is an error
        run(q, HostEngine(reports=1))


@pytest.mark.parametrize("q", THREE, ids=repr)
def test_a_band_of_the_callers_is_refilled_checked_and_kept(q):
    eng = HostEngine()
    band = h.banded(eng, N + 3, q.dt)
    band.a.view(np.uint8)[:] = 0
    got = run(q, eng, capacity=N + 3, band=band)
    assert (band.a.view(np.uint8).reshape(-1, q.dt.itemsize)[h.GUARD + N:] == h.BAND).all() and len(got) == (N if q.padded else N + 3)
    assert not band.freed and len(eng.live) == 1
    with pytest.raises(AssertionError):                                          # a buffer of another capacity
        run(q, eng, capacity=N + 4, band=band)


@pytest.mark.parametrize("q", THREE, ids=repr)
def test_twice_reports_a_second_run_that_differs_in_one_byte(q):
    eng = HostEngine()
    assert best.twice(q, eng, *ARGS[q], "clean", col_base=9).tobytes() == run(q, HostEngine()).tobytes() and eng.runs == 2
    for flip in (1, 2):
        with pytest.raises(AssertionError, match="planted: two runs differ"):
            best.twice(q, HostEngine(flip=flip), *ARGS[q], "planted", col_base=9)


@pytest.mark.parametrize("q", best.QUERIES, ids=repr)
def test_assert_same_names_the_count_the_first_index_and_both_records(q):
    want = np.zeros(6, q.dt)
    want["poly"] = np.arange(6)
    best.assert_same(q, want.copy(), want, "equal")
    got = want.copy()
    got["hit"][[2, 5]] = 1
    with pytest.raises(AssertionError) as e:
        best.assert_same(q, got, want, "planted")
    first = "first at ray 2: " if q in (best.RAY_CASTS, best.RAY_CASTS_GRID) else "first at 2: "
    assert str(e.value) == f"planted: 2 of 6 records differ; {first}got {got[2]}, want {want[2]}"


@pytest.mark.parametrize("dt", [best.RAY_CASTS.dt, best.CASTS.dt, best.CLEARANCES.dt], ids=["16", "24", "32"])
def test_check_against_sibling(dt):
    full = np.frombuffer(np.random.default_rng(3).bytes(6 * dt.itemsize), dt)
    best.check_against_sibling(full.copy(), full, "equal", ("grid", "the sibling"))
    best.check_against_sibling(full[:0].copy(), full[:0], "empty", ("grid", "the sibling"))
    for q, byte in ((1, 0), (3, dt.itemsize - 1), (5, dt.itemsize - 1)):         # (the last byte of the last record too)
        got = full.copy()
        got.view(np.uint8).reshape(6, -1)[q:, byte] ^= 0x80                      # record q and every one behind it
        with pytest.raises(AssertionError) as e:
            best.check_against_sibling(got, full, "planted", ("grid", "the sibling"))
        assert str(e.value) == f"planted: the bytes differ from the sibling'; first at {q}: grid {got[q]}, the sibling {full[q]}"
    with pytest.raises(AssertionError, match="records"):
        best.check_against_sibling(full[:5].copy(), full, "shorter", ("grid", "the sibling"))


def test_strips_of_gives_what_the_gpu_tests_assert_by_hand():
    assert (best.TILE_ROWS, best.TILE_COLS, best.BLOCKS_PER_CU) == (256, 64, 8)
    for cus in (1, 64, 256, 304):
        for row_tiles in (8 * cus, 8 * cus + 3):                                 # the row tiles alone fill the device: one strip
            assert best.strips_of(cus, 256 * row_tiles, 513) == 1 and best.strips_of(cus, 256 * row_tiles - 255, 311) == 1
        for n_b in (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513):       # one row tile of a small B: a strip per column tile
            assert best.strips_of(cus, 64, n_b) == best.strips_of(cus, 1, n_b) == min(-(-n_b // 64), 8 * cus)
    assert best.strips_of(256, 257, 311) == 5 and best.strips_of(256, 4099, 311) == 5
    assert best.strips_of(256, 256 * 512, 513) == 4 and best.strips_of(256, 256 * 1024 - 251, 513) == 2     # between the two
    assert best.strips_of(1, 1 << 20, 1 << 20) == 1 and best.strips_of(304, 1, 1) == 1                      # the clamp at 1


# ---- the shared refusals ---------------------------------------------------------------------------------------------------------------
class PolySet:
    def __init__(self, rows, n, stride, vx, vy, k):
        self.rows, self.n, self.stride, self.vx, self.vy = rows, n, stride, vx, vy


CASES = ["a NULL set A", "a NULL set B", "a NULL output", "rows 0 in A", "rows 0 in B", "rows 0 in an empty B", "rows 17 in A", "rows 17 in B",
         "rows 17 in an empty B", "a misaligned plane of A", "a misaligned plane of B", "a NULL plane", "a misaligned output", "stride < n in A",
         "stride < n in B", "flags 2", "flags 4", "flags 16", "flags -1", "row_base + n_a > 2^32", "col_base + n_b > 2^32", "n_a == 0: a no-op", "exactly 2^32"]


class Library:
    """the checks of a two-set query in the library's order, on the stand-in struct; accepts: a case let through although it is wrong"""
    PLANE, OUT = 4096, 8192

    def __init__(self, accepts=None, symbol="c2d_poly_set_standin"):
        self.accepts, self.symbol, self.said, self.seen = accepts, symbol, b"", []

    def why(self, a, b, rb, cb, flags, o):
        if a is None or b is None or not o:
            return "NULL argument"
        if a.n == 0:
            return None
        for s, empty_ok in ((a, False), (b, True)):
            if not 1 <= s.rows <= 16:
                return "rows must be 1..16"
            if empty_ok and s.n == 0:
                continue
            if not s.vx or not s.vy:
                return "NULL plane"
            if (s.vx | s.vy) & 3:
                return "planes must be 4-byte aligned"
            if (s.stride or s.n) < s.n:
                return "stride < n"
        if o & 15:
            return "the output must be 16-byte aligned"
        if flags & ~1:
            return "unknown flag"
        if rb + a.n > 1 << 32 or cb + b.n > 1 << 32:
            return "row_base + n_a and col_base + n_b must not exceed 2^32"

    def fn(self, *args):
        self.seen.append(args)
        why = self.why(*args)
        if why is None or len(self.seen) - 1 == self.accepts:
            return 0
        self.said = f"{self.symbol}: {why}".encode()
        return -1

    def refused(self, **kw):
        return best.refused_set_arguments(self.fn, PolySet, self.PLANE, self.OUT, "c2d_poly_set_standin", lambda: self.said, **kw)


def test_refused_set_arguments_tries_every_case_once():
    lib = Library()
    assert lib.refused() == CASES and len(lib.seen) == len(CASES) == len(set(lib.seen)) == 23
    lib = Library()
    assert lib.refused(accepted=False, off=4) == CASES[:21] and len(lib.seen) == 21     # (off 4 misaligns a 16-byte output too)


@pytest.mark.parametrize("case", range(21))
def test_refused_set_arguments_names_a_case_that_is_accepted(case):
    with pytest.raises(AssertionError, match=re.escape(f"c2d_poly_set_standin, {CASES[case]}: status 0")):
        Library(accepts=case).refused()


def test_refused_set_arguments_wants_the_symbol_the_word_and_the_two_accepted_calls():
    with pytest.raises(AssertionError, match="a NULL set A: status -1"):         # a message that names another call
        Library(symbol="c2d_poly_set_other").refused()
    lib = Library()
    lib.why = lambda *args: "no"                                                 # refusals without the case's word, and nothing accepted
    with pytest.raises(AssertionError, match="a NULL set A: status -1"):
        lib.refused()
    lib = Library()
    why = lib.why
    lib.why = lambda a, b, *rest: why(a, b, *rest) or ("never" if a is not None and a.n == 0 else None)
    with pytest.raises(AssertionError, match="n_a == 0: a no-op: status -1"):
        lib.refused()
    lib = Library()
    lib.why = lambda a, b, rb, *rest: why(a, b, rb, *rest) or ("never" if rb else None)
    with pytest.raises(AssertionError, match=r"exactly 2\^32: status -1"):
        lib.refused()


# ---- the reference of a scene whose polygons repeat ------------------------------------------------------------------------------------
@pytest.mark.parametrize("ref", [clearance_ref, cast_ref], ids=["clearances", "casts"])
def test_reduce_by_query_equals_the_reduction_of_the_materialised_matrix(wl, ref):
    """5 x 7 queries and obstacles drawn with repeats from 3 and 4 distinct polygons of one small box (hits and separated pairs)"""
    a, b = wl.random_convex_polygon_set(3, seed=41, extent=2.0), wl.random_convex_polygon_set(4, seed=42, extent=2.0)
    motions = h.motions(43, 3, 4, 2.0) if ref is cast_ref else ()
    R = ref.pair_records(a, b, *motions)
    rng = np.random.default_rng(44)
    ia, ib = rng.integers(0, 3, 5), rng.integers(0, 4, 7)
    assert len(set(ia)) < 5 and len(set(ib)) < 7 and 0 < (R["hit"] == 1).sum() < R.size
    bad_a, bad_b = np.zeros(3, bool), np.array([False, False, True, False])[ib]
    seen = set()
    for flags in (0, ref.SKIP_SELF):
        for rb, cb in ((0, 0), (7, 5), (5, 7), (1 << 20, (1 << 20) + 2), ((1 << 32) - 5, (1 << 32) - 7)):
            kw = dict(row_base=rb, col_base=cb, flags=flags)
            got = best.reduce_by_query(ref, R, ia, ib, bad_a, bad_b, **kw)
            want = ref.reduce(R[np.ix_(ia, ib)], bad_a[ia], bad_b, **kw)
            assert got.tobytes() == want.tobytes(), kw
            seen.add(want.tobytes())
    assert len(seen) > 6                                                         # the bases and SKIP_SELF decide records here
