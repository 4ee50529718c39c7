"""GPU tests of the polygon N x M mask (c2d_sat_poly_cross_mask) with a known number of undecided rows per wave and column: the wave
scene of tests/threshold_cases.py gives every wave one column for each count 0 .. 64, so phase 2 runs its lanes-over-axes form at
1, 2, 3 .. 15 undecided rows and its per-lane form from kPcSerialMin = 16 on (csrc/c2d_poly_cross.hip), with bars of 4, 5 and 7
vertices against rows of at most 3, 5 and 16.  tests/test_threshold_cases_cpu.py proves the collisions on the oracle and the undecided
counts on a numpy restatement of phase 1.  Every comparison is mask against mask or list against list (run_mask / mask_bits of tests/sat_cross_harness.py, run of
tests/pair_search_harness.py: guard rows and entries, count)."""
import numpy as np
import pytest

import pair_search_harness as psh
import threshold_cases as tc
from pair_search_harness import DeviceSet
from sat_cross_harness import check_mask, mask_bits, reference, run_mask

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene(eng, oracle):
    """(a, b, info, oracle mask), computed once and left unchanged"""
    a, b, info = tc.wave_count_scene(seed=1)
    ref = reference(eng, oracle, a, b)
    ref.setflags(write=False)
    return a, b, info, ref


def test_full_mask(eng, oracle, scene):
    a, b, info, ref = scene
    own = info["wave"][:, None] == info["col_wave"][None, :]
    for w, rows in enumerate(tc.WAVE_ROWS):      # from the oracle alone: wave w meets its own column m in min(m, rows)-many rows
        counts = (ref & own)[info["wave"] == w].sum(0)[info["col_wave"] == w]
        assert set(counts.tolist()) == set(range(rows + 1)) and not (ref & ~own).any()
    check_mask(eng, oracle, a, b, ref=ref)            # two plane placements; mask and count


@pytest.mark.parametrize("row_base,col_base", [(93, 100), (40, 10)])
def test_upper_with_a_shifted_diagonal(eng, scene, row_base, col_base):
    """col_base + j > row_base + i cuts through the staged words of waves 0 and 2: the tested bits differ from lane to lane, and the
    untested rows leave the wave's undecided count"""
    a, b, info, ref = scene
    n_a, n_b = a[0].shape[1], b[0].shape[1]
    tested = (np.arange(n_b)[None, :] + col_base) > (np.arange(n_a)[:, None] + row_base)
    for w in (0, 2):   # some of the wave's rows lose tested bits of their own columns' words, others keep them all
        block = tested[info["wave"] == w][:, (info["col_wave"] == w) & (np.arange(n_b) // 64 == np.flatnonzero(info["col_wave"] == w)[0] // 64)]
        assert block.any() and not block.all() and len({int(r.sum()) for r in block}) > 8
    ua, ub = DeviceSet(eng, a, offset=1, stride=n_a + 3), DeviceSet(eng, b, offset=2)
    m, c = run_mask(eng, ua.set, ub.set, upper=True, row_base=row_base, col_base=col_base)
    got = mask_bits(m, n_b)
    assert np.array_equal(got, ref & tested), f"{int((got != (ref & tested)).sum())} results differ"
    assert c == int(got.sum())
    ua.free()
    ub.free()
    eng.check_async()


def test_pair_list(eng, scene):
    a, b, _, ref = scene
    want = np.argwhere(ref).astype(np.uint32)
    ua, ub = DeviceSet(eng, a), DeviceSet(eng, b, offset=3, stride=b[0].shape[1] + 5)
    why = psh.compare(*psh.run(eng, psh.poly_cross(eng, ua, ub), len(want)), want)
    assert why is None, why
    ua.free()
    ub.free()
    eng.check_async()


def test_shuffled_columns(eng, oracle, scene):
    """B's columns in a fixed shuffle: one staged tile of 64 columns mixes many counts and all three bar sizes"""
    a, b, info, ref = scene
    perm = np.random.default_rng(3).permutation(b[0].shape[1])
    assert len(set(info["col_m"][perm[:64]].tolist())) > 32 and set(b[2][perm[:64]].tolist()) == {4, 5, 7}
    check_mask(eng, oracle, a, (b[0][:, perm], b[1][:, perm], b[2][perm]), ref=ref[:, perm])
