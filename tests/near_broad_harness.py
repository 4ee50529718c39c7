"""What belongs to c2d_poly_near_broad_pairs alone in its tests (test_gpu_near_broad.py, tools/near_broad_fuzz.py, the grid clearances'
tests): the size of a scene polygon, the exact grid squares, the wild scene, and check() against the reference
(tests/near_broad_ref.py).  The device set, the list call between guard entries and the judge are tests/pair_search_harness.py's.
numpy only."""
import numpy as np

import near_broad_ref as ref
import pair_search_harness as psh

F32 = np.float32
SIZE = 2.5                     # a polygon of the sparse scenes (pair_search_harness.sparse_set) is about this far across


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


def wild_scene(wl):
    """(a, b): a sparse scene with non-finite and huge coordinates, tiny and huge polygons, points, segments and absent polygons"""
    n = 900
    a = psh.sparse_set(wl, n, 5001, density=2.0)
    b = psh.sparse_set(wl, n - 150, 5002, rows=12, kmax=12, density=2.0)
    a, b = tuple(np.array(x) for x in a), tuple(np.array(x) for x in b)
    a[0][1, 10], a[1][0, 11], b[0][2, 20], b[1][1, 21] = np.nan, np.inf, -np.inf, np.nan            # non-finite live vertices
    a[0][:, 30] = a[0][:, 30] * F32(2.0 ** 50) + F32(2.0 ** 60)                                      # coordinates at 2^60
    a[1][:, 30] = a[1][:, 30] * F32(2.0 ** 50)
    b[0][:, 31] = b[0][:, 31] + F32(-2.0 ** 59.9)                                                    # just below: regular, huge box
    a[0][:, 32], a[1][:, 32] = a[0][:, 32] * F32(2.0 ** -110), a[1][:, 32] * F32(2.0 ** -110)       # below 2^-100, at the origin
    b[0][:, 33], b[1][:, 33] = b[0][:, 33] * F32(2.0 ** -110), b[1][:, 33] * F32(2.0 ** -110)
    b[0][:, 34], b[1][:, 34] = b[0][:, 34] * F32(2.0 ** -140), b[1][:, 34] * F32(2.0 ** -140)       # subnormal
    a[2][[40, 41, 42]], b[2][[43, 44, 45]] = [1, 2, 2], [1, 1, 2]                                    # points and segments
    a[0][:, 50], a[1][:, 50] = (a[0][:, 50] - np.nanmean(a[0][:, 50])) * F32(20.0), (a[1][:, 50] - np.nanmean(a[1][:, 50])) * F32(20.0)   # a huge polygon over the scene
    a[2][[60, 61, 62]], b[2][[63, 64, 65]] = [0, 17, 255], [0, 13, 200]                              # counts 0 and rows + 1
    return psh.nan_padded(a), psh.nan_padded(b)


def check(eng, a, b, max_dist, upper=False, min_pairs=1, want=None, place_a=(1, 3), place_b=(2, 0), with_k=True, far_cache=None):
    """the list of a against b — b None: the set against itself, the same memory — equals the reference; returns (list, reference)"""
    A = psh.DeviceSet(eng, a, offset=place_a[0], stride=a[0].shape[1] + place_a[1], with_k=with_k)
    B = A if b is None else psh.DeviceSet(eng, b, offset=place_b[0], stride=b[0].shape[1] + place_b[1], with_k=with_k)
    try:
        got, total = psh.run(eng, psh.near_broad(eng, A, B, max_dist, upper))
    finally:
        A.free()
        if B is not A:
            B.free()
    if want is None:
        want = ref.pairs(a, a if b is None else b, max_dist, upper=upper, far_cache=far_cache)
    why = psh.compare(got, total, want)
    assert why is None, why
    assert total >= min_pairs, total
    return got, want
