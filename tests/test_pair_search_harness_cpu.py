"""CPU test of tests/pair_search_harness.py itself, after tests/test_pair_list_harness_cpu.py: guard_fault() and run() carry the guard
entries of all six pair searches' tests and compare() is the judge of every one of their lists, so a silent mistake there would
remove that coverage everywhere at once.  Planted faults on arrays of a few entries; run() is driven by a stand-in engine whose
device arrays are numpy buffers and a stand-in search that writes pairs through the pointer it is handed."""
import ctypes as C

import numpy as np
import pytest

import pair_search_harness as psh

G = psh.GUARD


def buffer(capacity, listed=0):
    """what a correct call leaves behind: guard entries around a list of `capacity`, its first `listed` entries written"""
    buf = np.full((capacity + 2 * G, 2), 0xA5A5A5A5, np.uint32)
    buf[G:G + listed] = np.stack([np.arange(listed), np.arange(listed) + 100], axis=1)
    return buf


@pytest.mark.parametrize("capacity", [0, 1, 5])
def test_guard_check_accepts_a_clean_buffer(capacity):
    for listed in {0, capacity}:
        assert psh.guard_fault(buffer(capacity, listed), capacity) is None


@pytest.mark.parametrize("capacity", [0, 1, 5])
def test_guard_check_names_a_write_outside_the_list(capacity):
    """capacity 0: the list is empty and everything is guard"""
    for at, message in ((G - 1, "written in front of the list: 1 entries before it"), (0, f"written in front of the list: {G} entries before it"),
                        (G + capacity, f"written past the capacity: entry {capacity} of a list of {capacity}"),
                        (2 * G + capacity - 1, f"written past the capacity: entry {capacity + G - 1} of a list of {capacity}")):
        for field in (0, 1):                               # one index of the entry is enough
            buf = buffer(capacity, capacity)
            buf[at, field] = 7
            assert psh.guard_fault(buf, capacity).startswith(message), (at, field)
    with pytest.raises(AssertionError):                    # a buffer that is not the capacity's
        psh.guard_fault(buffer(capacity + 1), capacity)


def test_compare_accepts_equal_lists():
    want = buffer(5, 5)[G:G + 5]
    assert psh.compare(want.copy(), 5, want) is None
    assert psh.compare(np.zeros((0, 2), np.uint32), 0, np.zeros((0, 2), np.int64)) is None
    assert psh.compare(want.astype(np.int64), 5, want.tolist()) is None


def test_compare_names_each_planted_fault():
    want = buffer(6, 6)[G:G + 6]
    other = np.array([[9, 9]], np.uint32)
    assert psh.compare(want, 5, want) == "the total is 5, the reference has 6 pairs"
    assert psh.compare(want, 7, want).startswith("the total is 7")
    assert psh.compare(want[:5], 6, want) == "5 pairs written, the reference has 6"
    assert psh.compare(np.concatenate([want[:2], other, want[3:]]), 6, want) == "1 pairs missing, e.g. [(2, 102)]; 1 extra, e.g. [(9, 9)]"
    assert psh.compare(np.concatenate([want[:5], want[:1]]), 6, want).startswith("1 pairs missing, e.g. [(5, 105)]; 0 extra")   # one pair twice
    swapped = want[[0, 1, 3, 2, 4, 5]]
    assert psh.compare(swapped, 6, want) == "the same pairs in another order: first at position 2, got [3, 103], want [2, 102]"
    assert psh.compare(np.zeros((0, 2), np.uint32), 0, want).startswith("the total is 0")


# ---- run() on a stand-in engine -------------------------------------------------------------------------------------------------------
class C2DError(Exception):
    pass


class HostArray:
    def __init__(self, eng, a):
        self.a, self.ptr, self.nbytes, self.freed = a, a.ctypes.data, a.nbytes, False
        eng.live.append(self)

    def get(self):
        return self.a.copy()

    def free(self):
        self.freed = True


class HostEngine:
    """reports: how many of the following synchronise calls raise (a real engine: one after a call on a set with a bad count)"""

    def __init__(self, reports=0, error=C2DError):
        self.reports, self.error, self.live = reports, error, []

    def empty(self, shape, dtype):
        return HostArray(self, np.zeros(shape, dtype))

    def zeros(self, shape, dtype):
        return self.empty(shape, dtype)

    def memset(self, d, value, nbytes):
        d.a.view(np.uint8).reshape(-1)[:nbytes] = value

    def synchronize(self):
        if self.reports:
            self.reports -= 1
            raise self.error()


def search(eng, total, stray=None, reports=0):
    """the stand-in search: pair p = (p, p + 100) for p < min(capacity, total), the count incremented by the total; stray: one more
    entry written that many entries from the list's begin; reports: every call leaves that many reports with the engine"""
    def call(pairs, cap, cnt):
        eng.reports += reports
        cnt.a[0] += total
        if pairs is not None:
            n = min(cap, total)
            out = np.frombuffer((C.c_uint32 * (2 * (cap + 2 * G))).from_address(pairs - 8 * G), np.uint32).reshape(-1, 2)   # (from the front guard on)
            out[G:G + n] = np.stack([np.arange(n), np.arange(n) + 100], axis=1)
            if stray is not None:
                out[G + stray] = (1, 2)
    return call


@pytest.mark.parametrize("capacity", [None, 0, 3, 6, 9])
def test_run_returns_the_list_between_the_guards(capacity):
    eng = HostEngine()
    got, total = psh.run(eng, search(eng, 6), capacity)
    cap = 6 if capacity is None else capacity
    assert total == 6 and got.shape == (cap, 2), "the count is reset between the count-only call and the list call"
    n = min(cap, 6)
    assert np.array_equal(got[:n], buffer(6, 6)[G:G + n]) and (got[n:].view(np.uint64) == psh.SENTINEL).all()
    assert all(x.freed for x in eng.live) and len(eng.live) == 2


def test_run_raises_on_a_stray_entry():
    for stray, message in ((-1, "written in front of the list"), (-G, "written in front of the list"), (4, "written past the capacity"),
                           (4 + G - 1, "written past the capacity")):
        eng = HostEngine()
        with pytest.raises(AssertionError, match=message):
            psh.run(eng, search(eng, 6, stray=stray), 4)
    eng = HostEngine()
    psh.run(eng, search(eng, 6, stray=3), 4)               # (an entry inside the capacity is none)


def test_absent_wants_one_report_per_call():
    eng = HostEngine()
    assert psh.run(eng, search(eng, 6, reports=1), absent=True)[1] == 6          # the count-only call and the list call report once each
    eng = HostEngine()
    with pytest.raises(AssertionError, match="was not reported"):                # a search that reports nothing
        psh.run(eng, search(eng, 6), 6, absent=True)
    eng = HostEngine()
    with pytest.raises(C2DError):                                                # one that goes on reporting
        psh.run(eng, search(eng, 6, reports=2), 6, absent=True)
    eng = HostEngine()
    with pytest.raises(C2DError):                                                # and without `absent` a report is an error
        psh.run(eng, search(eng, 6, reports=1), 6)
    eng = HostEngine(error=ValueError)
    with pytest.raises(ValueError):                                              # another exception is not the report
        psh.run(eng, search(eng, 6, reports=1), 6, absent=True)
