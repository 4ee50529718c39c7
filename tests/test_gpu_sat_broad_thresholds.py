"""GPU tests of the broad-phase pair searches (c2d_sat_rect_broad_pairs, c2d_sat_poly_broad_pairs) with rows placed exactly on the
emit routes' switches (csrc/c2d_broad.hpp: kShortHits 16, kMidHits 512, kCandidateCap 1024): the station scene of
tests/threshold_cases.py, whose construction tests/test_threshold_cases_cpu.py proves on the oracle.  The tests cannot see which
route emitted a row; the scene guarantees it.  Every list must equal the cross list of the same call bit for bit (run / compare of
tests/pair_search_harness.py: guard entries, count first, then the exact capacity), and the two-set call the oracle's list as well."""
import numpy as np
import pytest

import pair_search_harness as psh
import threshold_cases as tc
from sat_cross_harness import rect_oracle_pairs, reference

pytestmark = pytest.mark.gpu
SHAPES = ["rect", "poly4", "poly16"]


class Side:
    """one set of the scene on the device, as rectangle planes ("rect") or as the same vertices as 4-gons in a layout of 4 or 16 vertex
    rows with NaN in the padded slots ("poly4", "poly16"): .search holds the adaptors of tests/pair_search_harness.py, .args is what
    they take for this set"""

    def __init__(self, eng, shape, planes):
        self.eng, self.n = eng, planes.shape[1]
        if shape == "rect":
            self.search = {"cross": psh.rect_cross, "broad": psh.rect_broad}
            self.d = eng.to_device(planes)
            self.args = ([self.d.row(k) for k in range(8)], self.n)
        else:
            self.search = {"cross": psh.poly_cross, "broad": psh.poly_broad}
            self.d = psh.DeviceSet(eng, tc.as_polygons(planes, int(shape[4:])), offset=1, stride=self.n + 3)
            self.args = (self.d,)

    def call(self, fn, other, upper):
        return self.search[fn](self.eng, *self.args, *other.args, upper)

    def run(self, fn, other, upper, capacity=None):
        """(pairs, total) of fn = "cross" / "broad" between guard entries, count first when capacity is None"""
        return psh.run(self.eng, self.call(fn, other, upper), capacity)

    def check(self, other=None, upper=False):
        """broad == cross, list and count, against `other` (itself when None); returns the list"""
        other = self if other is None else other
        got, _ = psh.same_as(self.eng, self.call("broad", other, upper), self.call("cross", other, upper))
        self.eng.check_async()
        return got

    def free(self):
        self.d.free()


@pytest.fixture(scope="module")
def scenes():
    """covers -> (a, b, info), built once and left unchanged"""
    return {covers: tc.station_scene(covers=covers, seed=1) for covers in (0, 3)}


@pytest.fixture(scope="module")
def oracle_lists(eng, oracle, scenes):
    """(shape kind, covers) -> the oracle's list of probes against piles, computed once.  The 4-row and the 16-row layout hold the
    same polygons, so one polygon list serves both."""
    out = {}
    for covers, (a, b, _) in scenes.items():
        out["rect", covers] = rect_oracle_pairs(oracle, a, b, False)
        out["poly", covers] = np.argwhere(reference(eng, oracle, tc.as_polygons(a, 4), tc.as_polygons(b, 4))).astype(np.uint32)
    return out


def per_row(pairs, n):
    return np.bincount(pairs[:, 0], minlength=n)


@pytest.mark.parametrize("covers", [0, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_two_sets(eng, oracle, scenes, oracle_lists, shape, covers):
    """probes against piles: a probe with h hitters has h hits (+ 3 through the wild tail with the covers)"""
    a, b, info = scenes[covers]
    A, B = Side(eng, shape, a), Side(eng, shape, b)
    got = A.check(B)                                   # broad == cross, list and count
    hits = per_row(got, A.n)
    assert np.array_equal(hits, info["h"] + covers)
    sides = {tc.SHORT_HITS - 1, tc.SHORT_HITS, tc.SHORT_HITS + 1, tc.MID_HITS - 1, tc.MID_HITS, tc.MID_HITS + 1}
    assert sides <= set(hits.tolist()) and hits.max() > tc.MID_HITS + 1
    assert np.array_equal(got, oracle_lists[shape[:4], covers]), "the list differs from the oracle"
    A.free()
    B.free()
    eng.check_async()


@pytest.mark.parametrize("covers", [0, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_transposed(eng, oracle, scenes, oracle_lists, shape, covers):
    """piles against probes: every pile object is a row with 0 or 1 hits, every cover a wild row that hits every probe"""
    a, b, info = scenes[covers]
    A, B = Side(eng, shape, a), Side(eng, shape, b)
    got = B.check(A)
    hits = per_row(got, B.n)
    assert set(hits[info["owner"] >= 0].tolist()) == {0, 1} and (hits[info["owner"] < 0] == A.n).all()
    want = oracle_lists[shape[:4], covers][:, ::-1]
    assert np.array_equal(got, want[np.lexsort((want[:, 1], want[:, 0]))]), "the list differs from the oracle's, transposed"
    A.free()
    B.free()
    eng.check_async()


@pytest.mark.parametrize("order", ["probes_first", "shuffled"])
@pytest.mark.parametrize("shape", SHAPES)
def test_self_upper(eng, oracle, scenes, shape, order):
    """the union against itself: pile rows hit each other, in cells with fewer and with more entries than the candidate cap"""
    a, b, _ = scenes[0]
    both = np.concatenate([a, b], axis=1)
    if order == "shuffled":
        both = both[:, tc.self_shuffle(a.shape[1], both.shape[1])]
    S = Side(eng, shape, both)
    got = S.check(upper=True)
    hits = per_row(got, S.n)
    assert (hits <= tc.SHORT_HITS).any() and ((hits > tc.SHORT_HITS) & (hits <= tc.MID_HITS)).any() and (hits > tc.MID_HITS).any()
    S.free()
    eng.check_async()


def route_probes(info, covers):
    """one probe on each route, by its hits and its walked entries: {name: station}"""
    hits, walked = info["h"] + covers, info["h"] + info["c"]

    def first(sel):
        return int(np.flatnonzero(sel)[0])

    return {
        "short path, 16 hits": first((hits == tc.SHORT_HITS) & (walked <= tc.CANDIDATE_CAP)),
        "wave path, 17 hits": first((hits == tc.SHORT_HITS + 1) & (walked <= tc.CANDIDATE_CAP)),
        "wave path, 512 hits": first((hits == tc.MID_HITS) & (walked <= tc.CANDIDATE_CAP)),
        "all columns, 513 hits": first((hits == tc.MID_HITS + 1) & (walked <= tc.CANDIDATE_CAP)),
        "crowded, 16 hits": first((hits == tc.SHORT_HITS) & (walked == tc.CANDIDATE_CAP + 1)),
    }


@pytest.mark.parametrize("covers", [0, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_capacity_inside_each_route(eng, scenes, shape, covers):
    """a capacity that ends in front of, one entry into, one entry short of and at the end of a row of each route: the list is the
    full list's prefix, the count the total, and nothing is written past the capacity (run checks the guard entries)"""
    a, b, info = scenes[covers]
    A, B = Side(eng, shape, a), Side(eng, shape, b)
    full, total = A.run("broad", B, False)
    assert total == len(full) == int((info["h"] + covers).sum())
    assert np.array_equal(full, A.run("cross", B, False)[0])
    row_off = np.searchsorted(full[:, 0], np.arange(A.n))
    cnt = per_row(full, A.n)
    for name, s in route_probes(info, covers).items():
        for cap in (row_off[s], row_off[s] + 1, row_off[s] + cnt[s] - 1, row_off[s] + cnt[s]):
            p, c = A.run("broad", B, False, capacity=int(cap))
            assert c == total, (name, cap)
            assert np.array_equal(p, full[:cap]), (name, cap)
    # the same call twice returns the same bytes
    cap = int(row_off[route_probes(info, covers)["wave path, 512 hits"]]) + tc.MID_HITS - 1
    p1, _ = A.run("broad", B, False, capacity=cap)
    p2, _ = A.run("broad", B, False, capacity=cap)
    assert p1.tobytes() == p2.tobytes() and np.array_equal(p1, full[:cap])
    A.free()
    B.free()
    eng.check_async()
