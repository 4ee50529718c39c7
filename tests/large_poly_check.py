"""Maximum-size checks of the polygon entry points, run as a separate process by tests/test_gpu_large_poly.py (torch builds the
multi-GB device inputs and has to be imported before libc2d.so).

Every input is a host-generated block of B pairs (B prime: a read that is off by 2^32 bytes, or by any power of two, lands on
a different pair, not on an identical copy of the right one) tiled on the device to n pairs, the last copy partial.  The oracle
decides the block once; every boolean of the batch is compared with the tiled expectation and the count with its exact sum.
Each case names the size limit it crosses.  Cases run one at a time and free what they made; `python large_poly_check.py NAME
...` runs only the cases named.
TEST INFRASTRUCTURE: uses the oracle as the checker."""
import importlib.util
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
import importlib  # noqa: E402

wl = importlib.import_module("c2d_amd.workloads")
from oracle import cpu as oracle  # noqa: E402

_spec = importlib.util.spec_from_file_location("bin_layout", os.path.join(ROOT, "tests", "tools", "bin_layout.py"))
layout = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(layout)

B = 999_983                  # pairs per block (prime)
DEV = torch.device("cuda", 0)
MEM_CAP = 40e9               # device memory a case may hold at any moment
K_MAX_GRID = 1 << 24         # kMaxGrid (csrc/c2d_internal.hpp): blocks per launch
TILES_PER_LAUNCH = 2 * K_MAX_GRID  # c2d_sat_poly_pairs_binned: kMaxGrid waves of kTilesPerWave = 2 tiles
eng = None
_blocks = {}
peaks = {}
_case = None
_base_used = 0


def used():
    free, total = torch.cuda.mem_get_info()
    return total - free


def note():
    """device memory this case holds now (all of the device's, less what was in use when the check started)"""
    u = used() - _base_used
    peaks[_case] = max(peaks.get(_case, 0), u)
    assert u < MEM_CAP, (_case, u)


def block(rows, kmin, kmax, extent):
    """(vx, vy, k, ref) of one B-pair block, between 20 % and 80 % of its pairs colliding"""
    key = (rows, kmin, kmax, extent)
    if key not in _blocks:
        vx, vy, k = wl.random_convex_polygons(B, seed=4099 * rows + 31 * kmin + kmax, kmin=kmin, kmax=kmax, extent=extent, rows=rows)
        ref, cnt = oracle.sat_poly_pairs(vx, vy, k)
        assert int(ref.sum()) == cnt and 0.2 <= ref.mean() <= 0.8, (key, ref.mean())
        _blocks[key] = (vx, vy, k, ref)
    return _blocks[key]


def tile_into(dst, a):
    """dst: device [M, n] (rows may be strided), a: host [M, B] -> n pairs of copies of a, the last one partial"""
    n = dst.shape[-1]
    blk = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    R, tail = divmod(n, B)
    dst[:, :R * B].view(-1, R, B).copy_(blk[:, None, :].expand(-1, R, B))
    dst[:, R * B:] = blk[:, :tail]


def tiled(a, n):
    """host [..., B] -> device [..., n]"""
    t = torch.empty(a.shape[:-1] + (n,), dtype={np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8}[a.dtype], device=DEV)
    tile_into(t.view(-1, n), a.reshape(-1, B))
    return t


def check_out(out, ref, n):
    """every boolean of out[:n] against the tiled block result -> the exact expected count"""
    ref_t = torch.from_numpy(ref).to(DEV)
    R, tail = divmod(n, B)
    o = out[:R * B].view(R, B)
    wrong = 0
    for r0 in range(0, R, 256):   # (in slices: no n-sized temporary)
        wrong += int((o[r0:r0 + 256] != ref_t[None, :]).sum())
    wrong += int((out[R * B:n] != ref_t[:tail]).sum())
    assert wrong == 0, f"{wrong} booleans differ from the oracle's"
    return R * int(ref.sum()) + int(ref[:tail].sum())


def ptr(t):
    return t.data_ptr()


def free_all():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def run_rows(n, rows, kmin, kmax, extent, bad_last=False):
    """c2d_sat_poly_pairs_rows over n tiled pairs; bad_last: the last pair's B count is out of range (reads 0, error at the sync)"""
    vx, vy, k, ref = block(rows, kmin, kmax, extent)
    dvx, dvy, dk = tiled(vx, n), tiled(vy, n), tiled(k, n)
    if bad_last:
        dk[1, n - 1] = rows + 1
    out = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    note()
    if rows == wl.KMAX:
        eng.sat_poly_pairs(ptr(dvx), ptr(dvy), ptr(dk), n, ptr(out), ptr(cnt))
    else:
        eng.sat_poly_pairs_rows(ptr(dvx), ptr(dvy), ptr(dk), n, rows, ptr(out), ptr(cnt))
    if bad_last:
        try:
            eng.synchronize()
            raise AssertionError("a vertex count out of range was not reported")
        except pkg.C2DError as e:
            assert "vertex count" in str(e), e
        assert int(out[n - 1]) == 0
        want = check_out(out, ref, n - 1)
    else:
        eng.synchronize()
        want = check_out(out, ref, n)
    eng.check_async()
    assert int(cnt.item()) == want, (int(cnt.item()), want)
    del dvx, dvy, dk, out, cnt
    free_all()
    return want


# ---- the cases -----------------------------------------------------------------------------------------------------------

def case_poly16():
    """c2d_sat_poly_pairs (sat_poly_kernel<16, 5, true>): polygon B's rows lie past 4 GiB from vx; the last pair has a bad count"""
    n = 40_000_001
    assert 4 * 16 * n < 2**32 < 4 * 31 * n
    return run_rows(n, 16, 3, 16, 2.5, bad_last=True)


def case_rows8():
    """_rows, rows = 8 (sat_poly_kernel<8, 7, false>): the last row starts past 4 GiB"""
    n = 75_000_001
    assert 4 * 15 * n > 2**32
    return run_rows(n, 8, 3, 8, 2.0)


def case_rows4():
    """_rows, rows = 4, n % 4 == 0 (sat_poly4_kernel): f32x4 row offsets past 4 GiB"""
    n = 160_000_000
    assert n % 4 == 0 and 4 * 7 * n > 2**32
    return run_rows(n, 4, 3, 4, 1.5)


def case_rows2_grid_stride():
    """_rows, rows = 2, K in {1, 2} (sat_poly_kernel<4, 8, false>): more than 2^24 tiles, so the grid is capped at 2^24 waves
    that stride a second pass, and the two-level count sees 2^24 waves"""
    n = 1_080_000_001
    assert (n + 63) // 64 > K_MAX_GRID
    return run_rows(n, 2, 1, 2, 2.0)


def case_onebin_limit():
    """_rows, rows 9, 12, 15: at n_max = floor((2^32 - 1) / (4 rows)) the layout runs as one bin of the binned kernel with planes
    of 4 GiB less a few bytes (buffer offsets and num_records with the sign bit set); at n_max + 1 the generic instance"""
    total = 0
    for rows in (9, 12, 15):
        n_max = (2**32 - 1) // (4 * rows)
        assert 4 * rows * n_max <= 2**32 - 1 < 4 * rows * (n_max + 1)
        for n in (n_max, n_max + 1):
            total += run_rows(n, rows, 3, rows, 2.5)
    return total


def case_caller_bin_largest_plane():
    """c2d_poly_bins_create: one counted 16 / 16-row bin with stride 67 108 800, the largest legal plane (2^32 - 4096 bytes);
    buffer offsets of the later rows are >= 2^31"""
    stride = 67_108_800
    n = stride - 1
    assert 4 * 16 * stride == 2**32 - 4096 and 4 * 15 * stride >= 2**31
    vx, vy, k, ref = block(16, 3, 16, 2.5)
    planes = torch.empty((4, 16, stride), dtype=torch.float32, device=DEV)
    for i, src in enumerate((vx[0], vy[0], vx[1], vy[1])):
        tile_into(planes[i][:, :n], src)
    dk = tiled(k, n)
    out = torch.empty(n, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    note()
    bins = eng.poly_bins_create([dict(rows_a=16, rows_b=16, n=n, stride=stride, ax=ptr(planes[0]), ay=ptr(planes[1]), bx=ptr(planes[2]),
                                      by=ptr(planes[3]), ka=ptr(dk[0]), kb=ptr(dk[1]), out=ptr(out))])
    eng.sat_poly_pairs_binned(bins, ptr(cnt))
    eng.synchronize()
    eng.check_async()
    want = check_out(out, ref, n)
    assert int(cnt.item()) == want
    bins.close()
    del planes, dk, out, cnt
    free_all()
    return want


def case_binned_two_launches():
    """c2d_sat_poly_pairs_binned over 2200 caller bins that share one B-pair input block (every other one with A and B swapped),
    each with a result slice of its own: 2.2e9 pairs, more than 2^25 tiles, so two launches, one bin straddling them"""
    NB = 2200
    tiles_per_bin = (B + 63) // 64
    assert NB * tiles_per_bin > TILES_PER_LAUNCH and TILES_PER_LAUNCH % tiles_per_bin != 0
    straddler = TILES_PER_LAUNCH // tiles_per_bin
    assert straddler * tiles_per_bin < TILES_PER_LAUNCH < (straddler + 1) * tiles_per_bin and straddler < NB
    vx, vy, k, ref = block(16, 3, 16, 2.5)
    dvx, dvy, dk = (torch.from_numpy(a).to(DEV) for a in (vx, vy, k))
    out = torch.full((NB, B), 7, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    specs = []
    for i in range(NB):
        a, b = (0, 1) if i % 2 == 0 else (1, 0)
        specs.append(dict(rows_a=16, rows_b=16, n=B, ax=ptr(dvx[a]), ay=ptr(dvy[a]), bx=ptr(dvx[b]), by=ptr(dvy[b]), ka=ptr(dk[a]),
                          kb=ptr(dk[b]), out=ptr(out[i])))
    torch.cuda.synchronize()
    note()
    bins = eng.poly_bins_create(specs)
    eng.sat_poly_pairs_binned(bins, ptr(cnt))
    eng.synchronize()
    eng.check_async()
    want = check_out(out.view(-1), ref, NB * B)
    assert int(cnt.item()) == want == NB * int(ref.sum())
    bins.close()
    del dvx, dvy, dk, out, cnt
    free_all()
    return want


def case_create_plane_limit():
    """c2d_poly_bins_create (never launched): a 16-row plane of exactly 2^32 bytes is refused, 256 bytes less is accepted"""
    tiny = torch.zeros(64, dtype=torch.float32, device=DEV)
    out = torch.zeros(64, dtype=torch.uint8, device=DEV)
    spec = dict(rows_a=16, rows_b=16, n=1, ax=ptr(tiny), ay=ptr(tiny), bx=ptr(tiny), by=ptr(tiny), out=ptr(out))
    try:
        eng.poly_bins_create([dict(spec, stride=2**26)])
        raise AssertionError("a plane of 4 GiB was accepted")
    except pkg.C2DError as e:
        assert "exceeds 4 GiB" in str(e), e
    eng.poly_bins_create([dict(spec, stride=2**26 - 64)]).close()
    return 0


def run_from_padded(n, rows, g, kmin, kmax, extent, above_16gib):
    """c2d_poly_bins_from_padded + the binned test + c2d_poly_bins_results over n tiled pairs; the block's size comes from the
    layout mirror and must lie on the stated side of 16 GiB (poly_bin_move_kernel<uint32_t> below, <uint64_t> at and above)"""
    vx, vy, k, ref = block(rows, kmin, kmax, extent)
    R, tail = divmod(n, B)
    hist_blk = layout.class_histogram(k, rows, g)
    hist_tail = layout.class_histogram(k[:, :tail], rows, g)
    hist = {c: R * hist_blk[c] + hist_tail.get(c, 0) for c in hist_blk}
    bins_want, block_bytes = layout.from_padded_layout(hist, n, rows, g)
    assert (block_bytes >= 16 << 30) == above_16gib, block_bytes
    dvx, dvy, dk = tiled(vx, n), tiled(vy, n), tiled(k, n)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    note()
    bins = eng.poly_bins_from_padded(ptr(dvx), ptr(dvy), ptr(dk), n, rows, g)
    note()
    layout.assert_handle_matches(bins, bins_want)
    del dvx, dvy, dk
    free_all()
    out = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    eng.sat_poly_pairs_binned(bins, ptr(cnt))
    bins.results(ptr(out))
    eng.synchronize()
    eng.check_async()
    note()
    want = check_out(out, ref, n)
    assert int(cnt.item()) == want, (int(cnt.item()), want)
    bins.close()
    del out, cnt
    free_all()
    return len(bins_want), block_bytes


def case_from_padded_below_16gib():
    """from_padded, every polygon a 16-gon, g = 1: one class, n chosen so that the block lies just below 16 GiB —
    poly_bin_move_kernel<uint32_t> with element offsets near 2^32, planes just below 4 GiB (one bin)"""
    n = 65_000_000
    while layout.from_padded_layout({255: n + 64}, n + 64, 16, 1)[1] < 16 << 30:
        n += 64
    n_bins, nbytes = run_from_padded(n, 16, 1, 16, 16, 2.5, above_16gib=False)
    assert n_bins == 1 and nbytes > (16 << 30) - (1 << 20)
    return n


def case_from_padded_split_k16():
    """from_padded, every polygon a 16-gon, g = 1, n = 7e7 + 3: one class whose planes would exceed 4 GiB — split into bins
    (the pass refused such a batch before) — in a block above 16 GiB: poly_bin_move_kernel<uint64_t>"""
    n_bins, _ = run_from_padded(70_000_003, 16, 1, 16, 16, 2.5, above_16gib=True)
    assert n_bins == 3
    return n_bins


def case_from_padded_split_counted():
    """from_padded, K ~ U{3..16}, g = 16, n = 7e7 + 3: every pair in one counted 16-row class, split likewise"""
    n_bins, _ = run_from_padded(70_000_003, 16, 16, 3, 16, 2.5, above_16gib=True)
    assert n_bins == 3
    return n_bins


CASES = [case_poly16, case_rows8, case_rows4, case_rows2_grid_stride, case_onebin_limit, case_caller_bin_largest_plane,
         case_binned_two_launches, case_create_plane_limit, case_from_padded_below_16gib, case_from_padded_split_k16,
         case_from_padded_split_counted]


def main(names):
    global eng, _case, _base_used
    eng = pkg.Engine(0)
    torch.cuda.init()
    _base_used = used()
    t_all = time.time()
    for fn in CASES:
        name = fn.__name__[len("case_"):]
        if names and name not in names:
            continue
        _case = name
        t0 = time.time()
        r = fn()
        print(f"{name}: ok ({r}), {time.time() - t0:.1f} s, peak device memory {peaks.get(name, 0) / 1e9:.1f} GB", flush=True)
    print(f"large poly ok: {time.time() - t_all:.1f} s")


if __name__ == "__main__":
    main(sys.argv[1:])
