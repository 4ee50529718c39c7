"""What the tests of c2d_poly_near_broad_pairs share (test_gpu_near_broad.py, tools/near_broad_fuzz.py): the list call between guard
entries, the judge that compares a list with the reference (tests/near_broad_ref.py), and the scenes.  The device-side set (row
offset, stride, gaps of NaN) and the list comparison are tests/sweep_broad_harness.py's: a set at rest is a MovingSet without motion
planes.  The judge and the scenes are numpy only, so the CPU tests can reach them."""
import numpy as np

import near_broad_ref as ref
import sweep_broad_harness as sh

F32 = np.float32
SENTINEL = sh.SENTINEL
Set = sh.MovingSet
compare = sh.compare
nan_padded = sh.nan_padded
SIZE = 2.5                     # a polygon of the sparse scenes is about this far across


def sparse_scene(wl, n, seed, rows=16, kmax=16, density=1.0):
    """the sparse scene of the polygon broad phase's tests"""
    return sh.sparse_scene(wl, n, seed, rows=rows, kmax=kmax, density=density)[0]


def grid_boxes(offsets, step=1.0 / 64):
    """(a, b): per entry (ox, oy) of `offsets`, in grid steps, a square A of 32 steps and a square B to its right.  oy == 0: face to
    face, B at A's height, ox steps apart: dist = ox * step.  oy != 0: B's lower left corner at A's upper right corner + (ox, oy):
    dist = step * hypot(ox, oy), exact for 3-4-5 offsets.  Every coordinate is a multiple of 1/64 below 2^17, so every difference,
    product and sum of the distance rule is exact.  The pairs of interest are (q, q); the squares of different q are 1024 apart."""
    n = len(offsets)
    ax, ay, bx, by = (np.full((16, n), np.nan, F32) for _ in range(4))
    for q, (ox, oy) in enumerate(offsets):
        x0, s = 1024.0 * q, 32 * step
        ax[:4, q], ay[:4, q] = [x0, x0 + s, x0 + s, x0], [0, 0, s, s]
        # B to the right of A (ox > 0), face to face when oy == 0 (B spans A's height), else its lower left corner at A's upper right + (ox, oy)
        lx = x0 + s + ox * step
        ly = (0.0 if oy == 0 else s + oy * step)
        bx[:4, q], by[:4, q] = [lx, lx + s, lx + s, lx], [ly, ly, ly + s, ly + s]
    k = np.full(n, 4, np.uint8)
    return (ax, ay, k), (bx, by, k.copy())


def run(eng, A, B, max_dist, upper=False, capacity=None, stream=0, absent=False):
    """(pairs u32[capacity][2], total) of c2d_poly_near_broad_pairs on the Sets A, B; capacity None: count first, then exact.  The list
    sits between four guard entries in front and four (plus everything past the capacity) behind, which are checked.  absent: the sets
    hold a vertex count out of range, which every call must report."""
    d_cnt = eng.zeros(1, np.uint64)
    if capacity is None:
        eng.poly_near_broad_pairs(A.set, B.set, max_dist, None, 0, d_cnt, upper=upper, stream=stream)
        sh._synchronize(eng, absent)
        capacity = int(d_cnt.get()[0])
        eng.memset(d_cnt, 0, 8)
    d_pairs = eng.empty((capacity + 8, 2), np.uint32)
    eng.memset(d_pairs, 0xA5, d_pairs.nbytes)
    eng.poly_near_broad_pairs(A.set, B.set, max_dist, d_pairs.ptr + 32, capacity, d_cnt, upper=upper, stream=stream)
    sh._synchronize(eng, absent)
    p, c = d_pairs.get(), int(d_cnt.get()[0])
    d_pairs.free()
    d_cnt.free()
    assert (p[:4].view(np.uint64) == SENTINEL).all(), "written in front of the list"
    assert (p[4 + capacity:].view(np.uint64) == SENTINEL).all(), "written past the capacity"
    return p[4:4 + capacity], c


def check(eng, a, b, max_dist, upper=False, min_pairs=1, want=None, place_a=(1, 3), place_b=(2, 0), with_k=True, far_cache=None):
    """the list of a against b — b None: the set against itself, the same memory — equals the reference; returns (list, reference)"""
    A = Set(eng, a, None, offset=place_a[0], stride=a[0].shape[1] + place_a[1], with_k=with_k)
    B = A if b is None else Set(eng, b, None, offset=place_b[0], stride=b[0].shape[1] + place_b[1], with_k=with_k)
    try:
        got, total = run(eng, A, B, max_dist, upper)
    finally:
        A.free()
        if B is not A:
            B.free()
    if want is None:
        want = ref.pairs(a, a if b is None else b, max_dist, upper=upper, far_cache=far_cache)
    why = compare(got, total, want)
    assert why is None, why
    assert total >= min_pairs, total
    return got, want
