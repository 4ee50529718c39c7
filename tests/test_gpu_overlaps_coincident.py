"""GPU tests of the overlap queries where two edges of the two shapes lie nearly on one line (the families of tests/overlap_cases.py:
aligned and nested boxes, a triangle on an edge, equal shapes relisted and moved by a few binary32 steps, and their neighbours):
every record equals tests/overlap_ref.py byte for byte, `hit` equals the pairwise GPU path, the rectangle call gives the 4-gon's
bytes, and the device's own areas and IoUs of the box families lie within the asserted bound of the analytic values, so that a wrong
kernel fails here even if the reference were wrong the same way.  Every output sits between guard bands (h.run)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import overlap_cases as oc  # noqa: E402
import overlap_ref as ref  # noqa: E402
import pair_list_harness as h  # noqa: E402
from overlap_query import OVERLAPS as Q  # noqa: E402
from pair_list_harness import RectsOnDevice, Uploaded, local, pairwise_gpu, rect_pairwise_gpu  # noqa: E402

pytestmark = pytest.mark.gpu
C_AREA = 16.0          # the area constant of tests/test_overlap_ref_cpu.py
run, poly_call, rect_call, assert_same = Q.run, Q.poly_call, Q.rect_call, Q.assert_same
_WANT = {}


def wanted(name):
    """the family and the reference's records of its pairs, computed once"""
    if name not in _WANT:
        f = oc.families()[name]
        _WANT[name] = (f, ref.poly_overlaps(f.a, f.b, np.arange(f.n), np.arange(f.n)))
    return _WANT[name]


@pytest.mark.parametrize("name", list(oc._family_draws()))
def test_family(eng, name):
    f, want = wanted(name)
    pairs = h.diag(f.n)
    assert (want["hit"] == 1).mean() > 0.9 and (want["area"] > 0).mean() > 0.7
    ua, ub = Uploaded(eng, f.a), Uploaded(eng, f.b)
    got = run(eng, poly_call(eng, ua.set, ub.set), pairs)
    ua.free()
    ub.free()
    assert_same(got, want, name)
    assert np.array_equal(got["hit"], pairwise_gpu(eng, f.a, f.b, pairs)), "hit differs from c2d_sat_poly_pairs_rows"
    if f.planes is not None:
        da, db = RectsOnDevice(eng, f.planes[0]), RectsOnDevice(eng, f.planes[1])
        as_rects = run(eng, rect_call(eng, da, db), pairs)
        da.free()
        db.free()
        assert_same(as_rects, ref.rect_overlaps(*f.planes, *local(pairs)), name + " as planes")
        assert as_rects.tobytes() == got.tobytes()
        assert np.array_equal(as_rects["hit"], rect_pairwise_gpu(eng, *f.planes, pairs))
        for records, what in ((got, name + " as 4-gons, device"), (as_rects, name + " as planes, device")):
            assert ((records["flags"] & (ref.DEGENERATE | ref.NO_CENTROID | ref.BAD_PAIR)) == 0).all()          # (a nested box may be clamped to its own area by a last bit)
            oc.check_against_the_analytic_boxes(f, records, C_AREA, what)
    eng.check_async()


def test_all_families_mixed_in_one_list_and_short_lists(eng):
    """every family in one pair of sets and one list in a fixed shuffle, so that a wave holds pairs with edges on one line (which take
    the split behind the ballot) next to ordinary ones; and the first 1, 64 and 65 entries of that list"""
    parts = [wanted(name) for name in oc.families()]
    a = tuple(np.concatenate([f.a[c] for f, _ in parts], axis=-1) for c in range(3))
    b = tuple(np.concatenate([f.b[c] for f, _ in parts], axis=-1) for c in range(3))
    want = np.concatenate([w for _, w in parts])
    n = len(want)
    assert 3000 < n < 10000
    pairs = h.diag(n)[np.random.default_rng(2602).permutation(n)]
    want = want[pairs[:, 0]]
    ua, ub = Uploaded(eng, a), Uploaded(eng, b)
    got = run(eng, poly_call(eng, ua.set, ub.set), pairs)
    assert_same(got, want, "all families, shuffled")
    assert np.array_equal(got["hit"], pairwise_gpu(eng, a, b, pairs))
    for length in (1, 64, 65):
        assert_same(run(eng, poly_call(eng, ua.set, ub.set), pairs[:length]), want[:length], f"list of {length}")
    ua.free()
    ub.free()
    boxes = [wanted(name)[0] for name in oc.BOX_FAMILIES]
    ra, rb = (np.concatenate([f.planes[s] for f in boxes], axis=1) for s in (0, 1))
    m = ra.shape[1]
    rpairs = h.diag(m)[np.random.default_rng(2603).permutation(m)]
    rwant = ref.rect_overlaps(ra, rb, *local(rpairs))
    da, db = RectsOnDevice(eng, ra), RectsOnDevice(eng, rb)
    for length in (1, 64, 65, m):
        assert_same(run(eng, rect_call(eng, da, db), rpairs[:length]), rwant[:length], f"rectangle list of {length}")
    da.free()
    db.free()
    eng.check_async()
