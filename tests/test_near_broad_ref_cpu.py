"""CPU tests of the judge of c2d_poly_near_broad_pairs (tests/near_broad_ref.py): its prefiltered route for large scenes equals the
literal route, the exact grid cases sit on the compare (dist == max_dist is listed, one grid step more is not), the consequences the
header states hold on the judge, and absent polygons and the upper triangle are removed."""
import numpy as np
import pytest

import distance_ref
import near_broad_harness as nh
import near_broad_ref as ref
import pair_search_harness as psh

F32 = np.float32


@pytest.mark.parametrize("upper", [False, True])
@pytest.mark.parametrize("max_dist", [0.0, 0.25, 2.5, 25.0])
def test_prefiltered_route_equals_the_literal_one(wl, max_dist, upper):
    a = psh.sparse_set(wl, 150, 41)
    b = a if upper else psh.sparse_set(wl, 111, 42, rows=12, kmax=12)
    a = tuple(np.array(x) for x in a)
    if not upper:
        a[0][:, 5] *= F32(2.0 ** 55)              # not tame: never dropped by the prefilter
        a[0][2, 6] = np.nan
        a[2][[7, 8, 9]] = [1, 2, 0]               # a point, a segment, an absent polygon
        b = tuple(np.array(x) for x in b)
        b[2][[3, 4]] = [1, 13]
    literal = ref.pairs(a, b, max_dist, upper=upper, direct_limit=1 << 30)
    cache = {}
    assert np.array_equal(ref.pairs(a, b, max_dist, upper=upper, direct_limit=0, far_cache=cache), literal)
    assert np.array_equal(ref.pairs(a, b, max_dist, upper=upper, direct_limit=0, chunk=1 << 12, far_cache={}), literal)
    assert np.array_equal(ref.pairs(a, b, max_dist, upper=upper, direct_limit=0, far_cache=cache), literal), "the cached first-axis matrices"
    assert len(literal) > 50
    if not upper:
        assert not np.isin(literal[:, 0], [9]).any() and not np.isin(literal[:, 1], [4]).any(), "an absent polygon is in no pair"
    else:
        assert (literal[:, 1] > literal[:, 0]).all()


def test_the_bounds_decide_most_pairs_and_only_rightly(wl):
    """on a sparse scene at the GPU tests' largest margin the bounds are no dead code (most listed pairs are `near`, most others `apart`)
    and never contradict the judge"""
    a, b = psh.sparse_set(wl, 300, 43), psh.sparse_set(wl, 187, 44, rows=8, kmax=8)
    ii, jj = np.repeat(np.arange(300), 187), np.tile(np.arange(187), 300)
    tame_a, tame_b = ref._extent(a)[5], ref._extent(b)[5]
    rec = distance_ref.poly_distances(a, b, ii, jj)
    for r in (0.0, 0.25, 2.5, 25.0):
        near, apart = ref._bounds(a, b, ii, jj, tame_a, tame_b, r)
        want = rec["dist"] <= F32(r)
        assert not (near & ~want).any() and not (apart & want).any() and not (near & apart).any()
        if r >= 2.5:
            assert near.sum() > 0.8 * want.sum() > 100 and apart.sum() > 0.8 * (~want).sum() > 100, (r, near.sum(), apart.sum(), want.sum())


def test_candidate_d2_restates_the_distance_rule_bit_for_bit(wl):
    """the smallest candidate_d2 over every edge and vertex of both sides is the record's dist, squared root and all, where the pair is
    no hit: on a sparse scene, on near-degenerate slivers and with points and segments"""
    a, b = psh.sparse_set(wl, 60, 45), psh.sparse_set(wl, 50, 46, rows=12, kmax=12)
    a, b = tuple(np.array(x) for x in a), tuple(np.array(x) for x in b)
    a[1][:, :10] *= F32(1e-4)                      # slivers
    a[2][[11, 12]], b[2][[3, 4]] = [1, 2], [2, 1]
    ii, jj = np.repeat(np.arange(60), 50), np.tile(np.arange(50), 60)
    rec = distance_ref.poly_distances(a, b, ii, jj)
    ax, ay, bx, by = a[0][:, ii], a[1][:, ii], b[0][:, jj], b[1][:, jj]
    ka, kb = a[2][ii].astype(np.int64), b[2][jj].astype(np.int64)
    best = np.full(len(ii), np.inf, F32)
    with np.errstate(all="ignore"):
        for px, py, kp, qx, qy, kq in ((ax, ay, ka, bx, by, kb), (bx, by, kb, ax, ay, ka)):
            for e in range(px.shape[0]):
                for v in range(qx.shape[0]):
                    d2 = ref.candidate_d2(px, py, kp, np.where(e < kp, e, 0), qx[v], qy[v])
                    best = np.where((e < kp) & (v < kq) & (d2 < best), d2, best)
    miss = rec["hit"] == 0
    assert miss.sum() > 2000 and np.array_equal(np.sqrt(best)[miss], rec["dist"][miss])


def test_exact_grid_cases_sit_on_the_compare():
    """face to face with a gap of g grid steps: dist == g / 64 exactly; at the corners with 3-4-5 offsets: dist == 5 m / 64"""
    offsets = [(8, 0), (9, 0), (1, 0), (2, 0), (3, 4), (6, 8), (4, 3), (3, 5), (12, 16), (12, 17)]
    a, b = nh.grid_boxes(offsets)
    q = np.arange(len(offsets))
    rec = distance_ref.poly_distances(a, b, q, q)
    want = np.array([8, 9, 1, 2, 5, 10, 5, np.sqrt(34.0), 20, np.sqrt(433.0)]) / 64
    assert np.array_equal(rec["dist"], want.astype(F32)) and (rec["hit"] == 0).all()
    own = lambda p: set(int(i) for i, j in p.tolist() if i == j)      # noqa: E731
    assert own(ref.pairs(a, b, 8 / 64)) == {0, 2, 3, 4, 6, 7}          # 8, 1, 2, 5, 5 and sqrt(34) = 5.83 steps
    assert own(ref.pairs(a, b, 5 / 64)) == {2, 3, 4, 6}                # dist == max_dist is listed; sqrt(34) / 64 is one step further on one axis
    assert own(ref.pairs(a, b, np.nextafter(F32(5 / 64), F32(0)))) == {2, 3}
    assert own(ref.pairs(a, b, 20 / 64)) == {0, 1, 2, 3, 4, 5, 6, 7, 8}   # (12, 16) is listed, (12, 17) is not
    assert own(ref.pairs(a, b, 9 / 64)) == {0, 1, 2, 3, 4, 6, 7}
    assert own(ref.pairs(a, b, 0.0)) == set() and own(ref.pairs(a, b, -0.0)) == set()


def test_consequences_on_the_judge(wl):
    """the list contains the hit pairs, grows with max_dist, and holds exactly the pairs whose record passes the compare"""
    a, b = psh.sparse_set(wl, 120, 51), psh.sparse_set(wl, 90, 52)
    ii, jj = np.repeat(np.arange(120), 90), np.tile(np.arange(90), 120)
    rec = distance_ref.poly_distances(a, b, ii, jj)
    last = set()
    for r in (0.0, 0.3, 3.0):
        p = ref.pairs(a, b, r)
        keep = (rec["hit"] == 1) | (rec["dist"] <= F32(r))
        assert np.array_equal(p, np.stack([ii[keep], jj[keep]], axis=1).astype(np.uint32))
        s = set(map(tuple, p.tolist()))
        assert last <= s and len(s) > len(last)
        last = s
    hits = set(map(tuple, np.stack([ii, jj], axis=1)[rec["hit"] == 1].tolist()))
    assert hits and hits <= set(map(tuple, ref.pairs(a, b, 0.0).tolist()))
    nan = np.full((16, 1), np.nan, F32)                                   # a polygon of NaN: no axis separates it, so it is hit, and listed at margin 0
    assert len(ref.pairs((nan, nan, np.array([3], np.uint8)), b, 0.0)) == 90
