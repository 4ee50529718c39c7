"""GPU tests of the all-pairs rectangle entry points (c2d_sat_rect_cross_mask / _pairs): result (i, j) must be the
boolean of the pairwise path on (A_i, B_j), bit for bit.  The reference materialises the pairs (np.repeat / np.tile) and
runs the CPU oracle on them up to a few million pairs; above that the same pairs go through the pairwise bit-mask kernel
(c2d_sat_rect_pairs_verts_mask, itself checked against the oracle by test_gpu_sat.py) in chunks."""
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pair_search_harness as psh
from pair_search_harness import SENTINEL

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_PAIRS = 4_000_000       # above this the reference is the pairwise GPU kernel
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000, 4099]
FUZZ_SEED = 2026


def rect_set(oracle, wl, n, seed, extent=8.0):
    """f32[8][n]: rectangles from random poses (the first five pose planes of the generator)"""
    return oracle.rects_from_poses(*wl.random_obb_pose_planes(n, seed=seed, extent=extent)[:5])


def reference(eng, oracle, a, b):
    """bool [n_a][n_b]: result (i, j) of the pairwise path on (A_i, B_j)"""
    n_a, n_b = a.shape[1], b.shape[1]
    out = np.empty((n_a, n_b), bool)
    rows = max(1, min(n_a, (ORACLE_PAIRS if n_a * n_b <= ORACLE_PAIRS else 2_000_000) // n_b))
    for r0 in range(0, n_a, rows):
        r1 = min(n_a, r0 + rows)
        pairs = np.concatenate([np.repeat(a[:, r0:r1], n_b, axis=1), np.tile(b, r1 - r0)])
        if n_a * n_b <= ORACLE_PAIRS:
            res, _ = oracle.sat_rect_pairs_verts(pairs)
            out[r0:r1] = res.reshape(r1 - r0, n_b).astype(bool)
        else:
            n = pairs.shape[1]
            d = eng.to_device(pairs)
            d_mask = eng.zeros((n + 63) // 64, np.uint64)
            eng.sat_rect_pairs_verts_mask([d.row(k) for k in range(16)], n, d_mask)
            bits = np.unpackbits(d_mask.get().view(np.uint8), bitorder="little")[:n]
            out[r0:r1] = bits.reshape(r1 - r0, n_b).astype(bool)
            d.free()
            d_mask.free()
    return out


def upload(eng, planes, offset=0):
    """planes f32[8][n] on the device, every plane shifted by `offset` floats; returns (array, 8 plane pointers)"""
    n = planes.shape[1]
    host = np.zeros((8, n + 4), np.float32)
    host[:, offset:offset + n] = planes
    d = eng.to_device(host)
    return d, [d.row(k) + 4 * offset for k in range(8)]


def mask_bits(mask_words, n_b):
    """u64 [rows][words] -> bool [rows][n_b] (bit j & 63 of word j >> 6)"""
    bits = np.unpackbits(np.ascontiguousarray(mask_words).view(np.uint8), bitorder="little", axis=-1)
    return bits.reshape(mask_words.shape[0], -1)[:, :n_b].astype(bool)


def run_mask(eng, pa, n_a, pb, n_b, ld=None, upper=False, row_base=0, col_base=0, stream=0):
    words = (n_b + 63) // 64
    ld = words if ld is None else ld
    d_mask = eng.empty((n_a, ld), np.uint64)
    eng.memset(d_mask, 0xA5, d_mask.nbytes, stream)
    d_cnt = eng.zeros(1, np.uint64, stream)
    eng.sat_rect_cross_mask(pa, n_a, pb, n_b, d_mask, ld_words=ld, row_base=row_base, col_base=col_base, upper=upper, count=d_cnt, stream=stream)
    eng.synchronize(stream)
    m, c = d_mask.get(), int(d_cnt.get()[0])
    d_mask.free()
    d_cnt.free()
    return m, c


@pytest.fixture(scope="module")
def big_sets(eng, oracle, wl):
    """A and B of 4099 rectangles each (extent 40: about 1 % of the pairs collide) with the full reference"""
    a, b = rect_set(oracle, wl, 4099, 11, extent=40.0), rect_set(oracle, wl, 4099, 12, extent=40.0)
    return a, b, reference(eng, oracle, a, b)


def test_shape_of_the_call(eng, big_sets):
    """Every size pair of 1, 63, 64, 65, 255, 256, 257, 1000, 4099, planes shifted by 0 to 3 floats, every other call on a
    stream of its own: the mask is the reference's prefix block, the tail bits are 0 and the count is its popcount."""
    a, b, ref = big_sets
    assert 0.002 < ref.mean() < 0.05
    s = eng.stream_create()
    try:
        for ka, n_a in enumerate(SIZES):
            for kb, n_b in enumerate(SIZES):
                da, pa = upload(eng, a[:, :n_a], offset=(ka + kb) % 4)
                db, pb = upload(eng, b[:, :n_b], offset=(ka + 2 * kb + 1) % 4)
                m, c = run_mask(eng, pa, n_a, pb, n_b, stream=s if (ka + kb) % 2 else 0)
                want = ref[:n_a, :n_b]
                bits = np.unpackbits(m.view(np.uint8), bitorder="little", axis=-1).reshape(n_a, -1)
                assert np.array_equal(bits[:, :n_b].astype(bool), want), (n_a, n_b)
                assert not bits[:, n_b:].any(), (n_a, n_b)
                assert c == int(want.sum()), (n_a, n_b)
                da.free()
                db.free()
    finally:
        eng.stream_destroy(s)


def test_layout_padding_words_untouched(eng, oracle, wl):
    n_a, n_b = 300, 1000
    a, b = rect_set(oracle, wl, n_a, 21, 6.0), rect_set(oracle, wl, n_b, 22, 6.0)
    ref = reference(eng, oracle, a, b)
    da, pa = upload(eng, a)
    db, pb = upload(eng, b)
    words = (n_b + 63) // 64
    m, c = run_mask(eng, pa, n_a, pb, n_b, ld=words + 3)
    assert (m[:, words:] == SENTINEL).all(), "padding words were written"
    bits = np.unpackbits(m[:, :words].copy().view(np.uint8), bitorder="little", axis=-1).reshape(n_a, -1)
    assert not bits[:, n_b:].any(), "tail bits j >= n_b are not 0"
    assert np.array_equal(bits[:, :n_b].astype(bool), ref) and c == int(ref.sum())
    da.free()
    db.free()


def test_upper_mode_and_shards(eng, oracle, wl):
    """One set against itself: the strict upper triangle equals the full mask's, everything on or below the diagonal is 0,
    the count covers tested pairs only; row shards (row_base) and column tiles (col_base) reproduce the one-call answer."""
    n = 1000
    s = rect_set(oracle, wl, n, 31, 5.0)
    ds, ps = upload(eng, s, offset=1)
    full, full_c = run_mask(eng, ps, n, ps, n)
    full_bits = mask_bits(full, n)
    assert np.array_equal(full_bits, full_bits.T), "the test is symmetric"
    assert full_c == int(full_bits.sum()) and full_bits.diagonal().all()
    up, up_c = run_mask(eng, ps, n, ps, n, upper=True)
    up_bits = mask_bits(up, n)
    tri = np.triu(np.ones((n, n), bool), 1)
    assert not up_bits[~tri].any(), "bits on or below the diagonal"
    assert np.array_equal(up_bits[tri], full_bits[tri])
    assert up_c == int(up_bits.sum()) == (full_c - n) // 2
    # two row shards of the upper triangle, each with its global row base
    cut = 389
    parts = []
    for r0, r1 in ((0, cut), (cut, n)):
        m, c = run_mask(eng, [p + 4 * r0 for p in ps], r1 - r0, ps, n, upper=True, row_base=r0)
        parts.append(m)
        assert c == int(mask_bits(m, n).sum())
    assert np.array_equal(np.concatenate(parts), up)
    # a column tile that starts at 448 (a multiple of 64, so the words line up) and a block at an arbitrary offset
    m, _ = run_mask(eng, ps, n, [p + 4 * 448 for p in ps], n - 448, upper=True, col_base=448)
    assert np.array_equal(mask_bits(m, n - 448), up_bits[:, 448:])
    r0, c0, nr, nc = 301, 517, 200, 333
    m, c = run_mask(eng, [p + 4 * r0 for p in ps], nr, [p + 4 * c0 for p in ps], nc, upper=True, row_base=r0, col_base=c0)
    assert np.array_equal(mask_bits(m, nc), up_bits[r0:r0 + nr, c0:c0 + nc]) and c == int(up_bits[r0:r0 + nr, c0:c0 + nc].sum())
    # the same block without the flag: the full mask's block, whatever the bases
    m, _ = run_mask(eng, [p + 4 * r0 for p in ps], nr, [p + 4 * c0 for p in ps], nc, row_base=r0, col_base=c0)
    assert np.array_equal(mask_bits(m, nc), full_bits[r0:r0 + nr, c0:c0 + nc])
    ds.free()


def check_against_oracle(eng, oracle, a, b, min_rate=0.0):
    ref = reference(eng, oracle, a, b)
    assert ref.mean() >= min_rate
    n_a, n_b = a.shape[1], b.shape[1]
    for off in (0, 3):
        da, pa = upload(eng, a, offset=off)
        db, pb = upload(eng, b, offset=(off + 1) % 4)
        m, c = run_mask(eng, pa, n_a, pb, n_b)
        got = mask_bits(m, n_b)
        assert np.array_equal(got, ref), f"{int((got != ref).sum())} results differ"
        assert c == int(ref.sum())
        da.free()
        db.free()
    return ref


def test_touching_pairs(eng, oracle, wl):
    """Sets built from pose pairs made to touch (thin almost everywhere near the diagonal), crowded so that many off-diagonal
    pairs are close too."""
    n = 1500
    pp = wl.touching_pose_pairs(n, seed=41, scale=0.05)
    a, b = oracle.rects_from_poses(*pp[:5]), oracle.rects_from_poses(*pp[5:])
    ref = check_against_oracle(eng, oracle, a, b, min_rate=0.01)
    assert 0.2 < ref.diagonal().mean() < 0.9


@pytest.mark.parametrize("scale", [1e-30, 1e30, 1e-42])
def test_extreme_scales(eng, oracle, wl, scale):
    """Coordinates around 1e-30 and 1e30 and denormal ones (1e-42: every coordinate below 2^-126)."""
    n = 1200
    a, b = rect_set(oracle, wl, n, 51, 3.0), rect_set(oracle, wl, n, 52, 3.0)
    a, b = (a.astype(np.float64) * scale).astype(np.float32), (b.astype(np.float64) * scale).astype(np.float32)
    if scale < 1e-38:
        assert (np.abs(a[a != 0]) < 1.2e-38).all()
    check_against_oracle(eng, oracle, a, b)


def test_non_finite_vertices(eng, oracle, wl):
    """NaN / inf / +-3e38 coordinates, and NaN placed at vertex 0 (the axis then never separates) and at a later vertex (skipped)."""
    n = 1100
    a, b = rect_set(oracle, wl, n, 61, 2.0), rect_set(oracle, wl, n, 62, 2.0)
    fin = reference(eng, oracle, a, b)
    a = wl.inject_non_finite(a, seed=63, frac=0.2)
    b = wl.inject_non_finite(b, seed=64, frac=0.2)
    a[0, 10:20] = np.nan          # x0 of A_10 .. A_19
    a[5, 30:40] = np.nan          # y2 of A_30 .. A_39
    b[1, 50:60] = np.nan          # y0 of B_50 .. B_59
    b[6, 70:80] = np.nan          # x3 of B_70 .. B_79
    ref = check_against_oracle(eng, oracle, a, b)
    assert (ref != fin).mean() > 0.01, "the injected values no longer change results"
    assert ref[10:20].all(), "a NaN at vertex 0 of A reads 'collide' with every B"


def test_pair_list(eng, oracle, wl):
    """The list equals np.argwhere(mask) + (row_base, col_base) in the same order, full and upper; a capacity below the
    count gives exactly the row-major prefix with nothing written behind it and the full total; the same call twice gives
    the same bytes."""
    n_a, n_b = 700, 2100
    a, b = rect_set(oracle, wl, n_a, 71, 5.0), rect_set(oracle, wl, n_b, 72, 5.0)
    da, pa = upload(eng, a, offset=2)
    db, pb = upload(eng, b, offset=1)
    for upper, rb, cb in ((False, 0, 0), (False, 1000, 77), (True, 0, 0), (True, 500, 100)):
        m, total = run_mask(eng, pa, n_a, pb, n_b, upper=upper, row_base=rb, col_base=cb)
        want = (np.argwhere(mask_bits(m, n_b)) + (rb, cb)).astype(np.uint32)
        assert total == len(want) and total > 1000
        call = psh.rect_cross(eng, pa, n_a, pb, n_b, upper, rb, cb)
        p, c = psh.run(eng, call, total)            # (run checks the guard entries in front of the list and past the capacity)
        assert c == total and np.array_equal(p, want)
        cap = total // 3 + 1
        p, c = psh.run(eng, call, cap)
        assert c == total and np.array_equal(p, want[:cap])
        p2, _ = psh.run(eng, call, cap)
        assert p.tobytes() == p2.tobytes()
    # capacity 0 with no buffer: a count-only call
    d_cnt = eng.zeros(1, np.uint64)
    eng.sat_rect_cross_pairs(pa, n_a, pb, n_b, None, 0, d_cnt)
    assert int(d_cnt.get()[0]) == int(reference(eng, oracle, a, b).sum())
    # the host convenience
    got = eng.rect_cross_pairs_host(a, b)
    assert np.array_equal(got, np.argwhere(reference(eng, oracle, a, b)).astype(np.uint32))
    got = eng.rect_cross_pairs_host(a, a, upper=True)
    ref_self = reference(eng, oracle, a, a)
    assert np.array_equal(got, np.argwhere(np.triu(ref_self, 1)).astype(np.uint32))
    da.free()
    db.free()


def test_pair_list_several_passes(eng, oracle, wl):
    """A row of 2^23 + 1 columns takes just over 1 MiB of mask, so the 256-MiB scratch holds 255 rows per pass: 600 rows run
    in three passes, and the running base carried on the device between them must keep the order."""
    n_a, n_b, blk = 600, (1 << 23) + 1, 4099
    a = rect_set(oracle, wl, n_a, 81, 1.0)
    b = np.tile(rect_set(oracle, wl, blk, 82, 300.0), (1, n_b // blk + 1))[:, :n_b]
    da, pa = upload(eng, a)
    db, pb = upload(eng, b)
    ref_block = reference(eng, oracle, a, b[:, :blk])
    per_row = ref_block.sum(1) * (n_b // blk) + ref_block[:, : n_b % blk].sum(1)
    total = int(per_row.sum())
    assert total > 10_000
    p, c = psh.run(eng, psh.rect_cross(eng, pa, n_a, pb, n_b), total)
    assert c == total
    p = p.astype(np.int64)
    assert np.array_equal(np.bincount(p[:, 0], minlength=n_a), per_row)
    assert (np.diff(p[:, 0] * n_b + p[:, 1]) > 0).all(), "not in row-major order"
    assert ref_block[p[:, 0], p[:, 1] % blk].all()
    da.free()
    db.free()


def test_past_4_gib(eng, oracle, wl):
    """n_a, n_b about 190 000 (multiples of no tile): the mask passes 4 GiB and bit indices pass 2^32.  Whole rows against the
    oracle — the first, the last and those that straddle the 2^32-bit and the 4-GiB boundaries — and the count against a
    popcount of the whole mask."""
    n_a, n_b = 190_003, 190_011
    words = (n_b + 63) // 64
    assert n_a * words * 8 > 1 << 32
    a, b = rect_set(oracle, wl, n_a, 91, 300.0), rect_set(oracle, wl, n_b, 92, 300.0)
    da, pa = upload(eng, a, offset=1)
    db, pb = upload(eng, b)
    d_mask = eng.empty((n_a, words), np.uint64)
    d_cnt = eng.zeros(1, np.uint64)
    eng.sat_rect_cross_mask(pa, n_a, pb, n_b, d_mask, count=d_cnt)
    count = int(d_cnt.get()[0])
    row_bits, row_bytes = words * 64, words * 8
    rows = {0, 1, (1 << 32) // row_bits, (1 << 32) // row_bits + 1, (1 << 32) // row_bytes, (1 << 32) // row_bytes + 1, n_a - 2, n_a - 1}
    rows |= set(np.random.default_rng(93).integers(0, n_a, 8).tolist())
    rows = sorted(rows)
    assert max(rows) * row_bytes > 1 << 32
    sub = a[:, rows]
    ref = reference(eng, oracle, sub, b)
    for k, r in enumerate(rows):
        got = mask_bits(eng.read(d_mask.ptr + r * row_bytes, (1, words), np.uint64), n_b)[0]
        assert np.array_equal(got, ref[k]), f"row {r}"
    total = 0
    step = (256 << 20) // row_bytes
    for r0 in range(0, n_a, step):
        r1 = min(n_a, r0 + step)
        total += int(np.bitwise_count(eng.read(d_mask.ptr + r0 * row_bytes, ((r1 - r0) * words,), np.uint64)).sum())
    assert total == count > 0
    for x in (da, db, d_mask, d_cnt):
        x.free()


def test_argument_errors(eng, pkg, oracle, wl):
    import ctypes as C

    a = rect_set(oracle, wl, 100, 5, 3.0)
    da, pa = upload(eng, a)
    d_mask = eng.zeros((100, 4), np.uint64)
    d_cnt = eng.zeros(1, np.uint64)
    eng.sat_rect_cross_mask(pa, 0, pa, 100, d_mask)          # n_a == 0: a no-op
    eng.sat_rect_cross_mask(pa, 100, pa, 0, d_mask)          # n_b == 0: a no-op
    eng.sat_rect_cross_pairs(pa, 0, pa, 100, None, 0, None)
    planes = (C.c_void_p * 8)(*pa)
    raw = eng.lib.c2d_sat_rect_cross_mask
    assert raw(eng.h, None, 100, planes, 100, 0, 0, 0, d_mask.ptr, 2, None, None) == -1                   # NULL plane array
    assert raw(eng.h, planes, 100, planes, 100, 0, 0, 2, d_mask.ptr, 2, None, None) == -1                 # unknown flag
    assert raw(eng.h, planes, 100, planes, 100, 0, 0, -1, d_mask.ptr, 2, None, None) == -1
    bad = [
        lambda: eng.sat_rect_cross_mask(pa, 100, pa, 100, d_mask, ld_words=1),                          # ld_words < ceil(n_b / 64)
        lambda: eng.sat_rect_cross_mask(pa, 100, pa, 100, d_mask.ptr + 4),                               # mask not 8-byte aligned
        lambda: eng.sat_rect_cross_mask(pa, 100, pa, 100, None),
        lambda: eng.sat_rect_cross_mask(pa[:7] + [0], 100, pa, 100, d_mask),                              # a NULL plane
        lambda: eng.sat_rect_cross_pairs(pa, 100, pa, 100, d_mask, 10, None),                             # no count
        lambda: eng.sat_rect_cross_pairs(pa, 100, pa, 100, None, 10, d_cnt),                              # no buffer
        lambda: eng.sat_rect_cross_pairs(pa, 100, pa, 100, d_mask, 10, d_cnt, row_base=(1 << 32) - 99),   # row index 2^32
        lambda: eng.sat_rect_cross_pairs(pa, 100, pa, 100, d_mask, 10, d_cnt, col_base=(1 << 32) - 50),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(pkg.C2DError) as e:
            call()
        assert e.value.status == -1, k
    # the largest bases the u32 list allows are accepted
    eng.sat_rect_cross_pairs(pa, 100, pa, 100, d_mask, 10, d_cnt, row_base=(1 << 32) - 100, col_base=(1 << 32) - 100)
    eng.synchronize()
    for x in (da, d_mask, d_cnt):
        x.free()


def test_mask_form_graph_capture():
    """One capture of the mask form on a single stream, replayed: the same mask and count as the eager call
    (tests/cross_graph_check.py, its own process: torch has to be imported before libc2d.so)."""
    out = subprocess.run([sys.executable, os.path.join(HERE, "cross_graph_check.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "cross graph ok" in out.stdout


def test_fuzzer_configurations_at_a_fixed_seed(eng, oracle):
    """tests/tools/cross_fuzz.py at a fixed seed, each configuration from its own stream (seed, index): sixteen configurations, chosen so
    that they hold what the tool is for — the upper triangle with unequal bases, a list capacity below the total, a count-only call,
    A and B the same memory, a set with non-finite coordinates, ld_words beyond the row's words"""
    spec = importlib.util.spec_from_file_location("cross_fuzz", os.path.join(HERE, "tools", "cross_fuzz.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    seen, compared = [], 0
    for i in range(16):
        ok, (desc, n) = fz.one(eng, np.random.default_rng([FUZZ_SEED, i]), i, None, oracle)
        assert ok, desc
        seen.append(desc)
        compared += n
    assert any(re.search(r"upper True, bases \d+, \d+ \(unequal\)", d) for d in seen), seen           # a shifted diagonal
    assert any("below the total" in d for d in seen) and any("count-only list call" in d for d in seen), seen
    assert any("the same memory" in d for d in seen) and any("non-finite" in d for d in seen), seen
    assert any(re.search(r"ld_words \d+ > words", d) for d in seen), seen
    assert compared > 1000
    eng.check_async()
