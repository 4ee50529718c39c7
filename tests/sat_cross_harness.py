"""What the tests of the SAT pair searches share beyond tests/pair_search_harness.py (test_gpu_sat_poly_cross.py, its wave-count and
threshold companions, test_gpu_sat_broad.py, test_gpu_sat_poly_broad.py): the oracle references on materialised pairs — never the code
under test — the polygon N x M mask call between guard rows, and the degenerate and touching scenes.  A plain module on numpy only."""
import numpy as np

from pair_search_harness import SENTINEL, DeviceSet

ORACLE_PAIRS = 4_000_000       # above this the polygon reference is the pairwise GPU kernel
CHUNK = 1_000_000              # materialised pairs per reference chunk (about 260 MB of host memory at 16 rows)


def rect_oracle_pairs(oracle, a, b, upper):
    """u32[total][2]: the oracle's colliding pairs of the rectangle planes a, b in row-major order"""
    n_a, n_b = a.shape[1], b.shape[1]
    res, _ = oracle.sat_rect_pairs_verts(np.concatenate([np.repeat(a, n_b, axis=1), np.tile(b, n_a)]))
    m = res.reshape(n_a, n_b).astype(bool)
    if upper:
        m &= np.triu(np.ones((n_a, n_b), bool), 1)
    return np.argwhere(m).astype(np.uint32)


def padded(s, rows):
    """the set (vx, vy, k) in a layout of `rows` vertex rows (zeros above its own)"""
    vx, vy, k = s
    if vx.shape[0] == rows:
        return s
    ox, oy = np.zeros((rows, vx.shape[1]), np.float32), np.zeros((rows, vx.shape[1]), np.float32)
    ox[:vx.shape[0]], oy[:vx.shape[0]] = vx, vy
    return ox, oy, k


def counts_of(s):
    return np.full(s[0].shape[1], s[0].shape[0], np.uint8) if s[2] is None else s[2]


def reference(eng, oracle, a, b, force_gpu=False, fe=None):
    """bool [n_a][n_b]: result (i, j) of the pairwise path on (A_i, B_j); `fe`: another build's engine for the GPU reference"""
    rows = max(a[0].shape[0], b[0].shape[0])
    (ax, ay, _), (bx, by, _) = padded(a, rows), padded(b, rows)
    ka, kb = counts_of(a), counts_of(b)
    n_a, n_b = ax.shape[1], bx.shape[1]
    out = np.empty((n_a, n_b), bool)
    use_gpu = force_gpu or n_a * n_b > ORACLE_PAIRS
    step = max(1, CHUNK // n_b)
    run = fe or eng
    for r0 in range(0, n_a, step):
        r1 = min(n_a, r0 + step)
        m = (r1 - r0) * n_b
        vx = np.stack([np.repeat(ax[:, r0:r1], n_b, axis=1), np.tile(bx, r1 - r0)])
        vy = np.stack([np.repeat(ay[:, r0:r1], n_b, axis=1), np.tile(by, r1 - r0)])
        k = np.stack([np.repeat(ka[r0:r1], n_b), np.tile(kb, r1 - r0)])
        if use_gpu:
            d_vx, d_vy, d_k = run.to_device(vx), run.to_device(vy), run.to_device(k)
            d_out = run.zeros(m, np.uint8)
            run.sat_poly_pairs_rows(d_vx, d_vy, d_k, m, rows, d_out)
            res = d_out.get()
            for x in (d_vx, d_vy, d_k, d_out):
                x.free()
        else:
            res, _ = oracle.sat_poly_pairs(vx, vy, k)
        out[r0:r1] = res.reshape(r1 - r0, n_b).astype(bool)
    return out


def mask_bits(mask_words, n_b):
    """u64 [rows][words] -> bool [rows][n_b] (bit j & 63 of word j >> 6)"""
    bits = np.unpackbits(np.ascontiguousarray(mask_words).view(np.uint8), bitorder="little", axis=-1)
    return bits.reshape(mask_words.shape[0], -1)[:, :n_b].astype(bool)


def run_mask(eng, a, b, ld=None, upper=False, row_base=0, col_base=0, stream=0):
    """(mask words u64 [n_a][ld], count) of c2d_sat_poly_cross_mask on the c2d_poly_sets a, b; the mask sits between two guard rows"""
    n_a, n_b = a.n, b.n
    ld = (n_b + 63) // 64 if ld is None else ld
    d_mask = eng.empty((n_a + 2, ld), np.uint64)
    eng.memset(d_mask, 0xA5, d_mask.nbytes, stream)
    d_cnt = eng.zeros(1, np.uint64, stream)
    eng.sat_poly_cross_mask(a, b, d_mask.ptr + 8 * ld, ld_words=ld, row_base=row_base, col_base=col_base, upper=upper, count=d_cnt, stream=stream)
    eng.synchronize(stream)
    m, c = d_mask.get(), int(d_cnt.get()[0])
    d_mask.free()
    d_cnt.free()
    assert (m[0] == SENTINEL).all() and (m[-1] == SENTINEL).all(), "written outside the mask"
    return m[1:-1], c


def check_mask(eng, oracle, a, b, ref=None, offsets=((0, 1), (3, 0))):
    """mask and count of a x b equal the reference, for two placements of the planes; returns the reference"""
    ref = reference(eng, oracle, a, b) if ref is None else ref
    for oa, ob in offsets:
        ua, ub = DeviceSet(eng, a, offset=oa, stride=a[0].shape[1] + oa), DeviceSet(eng, b, offset=ob)
        m, c = run_mask(eng, ua.set, ub.set)
        got = mask_bits(m, ub.n)
        assert np.array_equal(got, ref), f"{int((got != ref).sum())} results differ"
        assert c == int(ref.sum())
        ua.free()
        ub.free()
    eng.check_async()
    return ref


def degenerate_set(wl, n, seed):
    """points, segments, repeated vertices, collinear polygons, and ordinary ones, close together"""
    rng = np.random.default_rng(seed)
    vx, vy, k = wl.random_convex_polygon_set(n, seed=seed, extent=3.0)
    vx, vy, k = vx.copy(), vy.copy(), k.copy()
    kind = rng.integers(0, 6, n)
    k[kind == 0] = 1
    k[kind == 1] = 2
    rep = np.flatnonzero(kind == 2)          # repeated vertices: vertex 1 = vertex 0, vertex 3 = vertex 2
    vx[1, rep], vy[1, rep] = vx[0, rep], vy[0, rep]
    vx[3, rep], vy[3, rep] = vx[2, rep], vy[2, rep]
    col = np.flatnonzero(kind == 3)          # collinear: every vertex on one line through vertex 0
    tt = rng.uniform(-2, 2, (16, col.size)).astype(np.float32)
    dx, dy = rng.choice([0.0, 1.0, 0.5], col.size).astype(np.float32), rng.choice([1.0, 0.0, 0.25], col.size).astype(np.float32)
    vx[:, col], vy[:, col] = vx[0, col] + tt * dx, vy[0, col] + tt * dy
    return vx, vy, k


def touching_sets(n):
    """A_i and B_i are axis-aligned boxes (k = 4) built on an integer grid so that B_i shares an edge (i even) or exactly one
    vertex (i odd) with A_i, every coordinate exact in float32."""
    i = np.arange(n)
    x0, y0 = (3 * (i % 50)).astype(np.float32), (3 * (i // 50)).astype(np.float32)
    ax = np.stack([x0, x0 + 1, x0 + 1, x0])
    ay = np.stack([y0, y0, y0 + 1, y0 + 1])
    sx, sy = np.float32(1), np.where(i % 2 == 0, 0, 1).astype(np.float32)   # shifted right by 1 (edge) or right and up (vertex)
    k = np.full(n, 4, np.uint8)
    return (ax, ay, k), (ax + sx, ay + sy, k)
