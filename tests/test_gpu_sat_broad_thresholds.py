"""GPU tests of the broad-phase pair searches (c2d_sat_rect_broad_pairs, c2d_sat_poly_broad_pairs) with rows placed exactly on the
emit routes' switches (csrc/c2d_broad.hpp: kShortHits 16, kMidHits 512, kCandidateCap 1024): the station scene of
tests/threshold_cases.py, whose construction tests/test_threshold_cases_cpu.py proves on the oracle.  The tests cannot see which
route emitted a row; the scene guarantees it.  Every list must equal the cross list of the same call bit for bit (run / check of
test_gpu_sat_broad.py and test_gpu_sat_poly_broad.py: guard entries, count first, then the exact capacity), and the two-set call
the oracle's list as well."""
import numpy as np
import pytest

import test_gpu_sat_broad as rect_tests
import test_gpu_sat_poly_broad as poly_tests
import threshold_cases as tc
from test_gpu_sat_poly_cross import Uploaded, reference

pytestmark = pytest.mark.gpu
SHAPES = ["rect", "poly4", "poly16"]


class Rects:
    """rectangle planes on the device, behind the interface the tests below use for either shape"""

    def __init__(self, eng, planes):
        self.eng, self.host, self.n = eng, planes, planes.shape[1]
        self.d = eng.to_device(planes)
        self.arg = rect_tests.planes_of(self.d)

    def run(self, fn, other, upper, capacity=None):
        return rect_tests.run(self.eng, fn, self.arg, self.n, other.arg, other.n, upper, capacity)

    def check(self, oracle, other=None, upper=False):
        return rect_tests.check(self.eng, oracle, self.host, None if other is None else other.host, upper=upper)

    def free(self):
        self.d.free()


class Polys:
    """the same vertices as 4-gons in a layout of `rows` vertex rows, NaN in the padded slots"""

    def __init__(self, eng, planes, rows):
        self.eng, self.host, self.n = eng, tc.as_polygons(planes, rows), planes.shape[1]
        self.up = Uploaded(eng, self.host, offset=1, stride=self.n + 3)

    def run(self, fn, other, upper, capacity=None):
        return poly_tests.run(self.eng, fn, self.up.set, other.up.set, upper, capacity)

    def check(self, oracle, other=None, upper=False):
        o = self if other is None else other
        return poly_tests.check(self.eng, oracle, self.host, None if other is None else o.host, upper=upper, ua=self.up, ub=o.up, use_oracle=False)

    def free(self):
        self.up.free()


def upload(eng, shape, planes):
    return Rects(eng, planes) if shape == "rect" else Polys(eng, planes, int(shape[4:]))


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
        out["rect", covers] = rect_tests.oracle_pairs(oracle, a, b, False)
        out["poly", covers] = np.argwhere(reference(eng, oracle, tc.as_polygons(a, 4), tc.as_polygons(b, 4))).astype(np.uint32)
    return out


def per_row(pairs, n):
    return np.bincount(pairs[:, 0], minlength=n)


@pytest.mark.parametrize("covers", [0, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_two_sets(eng, oracle, scenes, oracle_lists, shape, covers):
    """probes against piles: a probe with h hitters has h hits (+ 3 through the wild tail with the covers)"""
    a, b, info = scenes[covers]
    A, B = upload(eng, shape, a), upload(eng, shape, b)
    got = A.check(oracle, B)                                   # broad == cross, list and count
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
    A, B = upload(eng, shape, a), upload(eng, shape, b)
    got = B.check(oracle, A)
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
    S = upload(eng, shape, both)
    got = S.check(oracle, upper=True)
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
    A, B = upload(eng, shape, a), upload(eng, shape, b)
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
