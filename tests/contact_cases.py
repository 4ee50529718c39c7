"""Inputs shared by the contact tests (test_contact_ref_cpu.py, test_gpu_contacts.py) and tests/tools/contact_fuzz.py: seeded sets
and pair lists only, no expectations.  A polygon set is (vx f32[rows][n], vy, k u8[n]); a rectangle set is planes f32[8][n]."""
import numpy as np

F = np.float32
LIST_LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 1000, 4099]


def all_pairs(n_a, n_b):
    """the row-major enumeration of an N x M block as u32 [n_a * n_b][2]"""
    return np.stack([np.repeat(np.arange(n_a), n_b), np.tile(np.arange(n_b), n_a)], axis=1).astype(np.uint32)


def dense_poly_sets(wl, n=300, extent=4.0, rows_a=16, rows_b=16, seeds=(7101, 7102)):
    """two sets of about 300 polygons in a small box: about a fifth of all pairs overlap"""
    a = wl.random_convex_polygon_set(n, seed=seeds[0], kmin=min(3, rows_a), kmax=rows_a, extent=extent, rows=rows_a)
    b = wl.random_convex_polygon_set(n + 11, seed=seeds[1], kmin=min(3, rows_b), kmax=rows_b, extent=extent, rows=rows_b)
    return a, b


def well_conditioned_poly_sets(wl, n=120):
    """coordinates in [-8, 8], no degenerate polygon: near-regular polygons (full-bodied, no tiny edge) in a box of +-4"""
    rng = np.random.default_rng(7201)
    out = []
    for _ in range(2):
        vx, vy, k = np.zeros((16, n), F), np.zeros((16, n), F), rng.integers(3, 17, n).astype(np.uint8)
        for q in range(n):
            xs, ys = wl.near_regular_polygon(int(k[q]), rng, rng.uniform(0.5, 2.5), rng.uniform(0.5, 2.5), rng.uniform(0, 6.28))
            vx[:k[q], q], vy[:k[q], q] = xs + F(rng.uniform(-4, 4)), ys + F(rng.uniform(-4, 4))
        out.append((vx, vy, k))
    assert all(np.abs(s[0]).max() <= 8 and np.abs(s[1]).max() <= 8 for s in out)
    return out[0], out[1]


def translated(b, j, tx, ty):
    """polygons b[j] moved by (tx, ty) per pair: a set with one polygon per pair"""
    vx, vy, k = b
    return (vx[:, j] + tx[None, :].astype(F)).astype(F), (vy[:, j] + ty[None, :].astype(F)).astype(F), k[j]


def touching_poly_sets(n=100):
    """A_i and B_i are unit boxes on an integer grid; B_i shares an edge (i even) or exactly one vertex (i odd) with A_i"""
    i = np.arange(n)
    x0, y0 = (3 * (i % 10)).astype(F), (3 * (i // 10)).astype(F)
    ax, ay = np.stack([x0, x0 + 1, x0 + 1, x0]), np.stack([y0, y0, y0 + 1, y0 + 1])
    sy = np.where(i % 2 == 0, 0, 1).astype(F)
    k = np.full(n, 4, np.uint8)
    return (ax, ay, k), (ax + F(1), ay + sy, k)


def hard_poly_batches(wl):
    """name -> (a, b, pairs u32 [m][2], finite): one small batch per hard input class; `finite` says whether the batch is finite
    and free of overflow (the property hit == (depth >= 0) is promised there)"""
    rng = np.random.default_rng(7301)
    n = 48
    base_a = wl.random_convex_polygon_set(n, seed=7302, extent=3.0)
    base_b = wl.random_convex_polygon_set(n, seed=7303, extent=3.0)
    grid = all_pairs(n, n)
    out = {}

    def copy(s):
        return tuple(x.copy() for x in s)

    def reverse(s):
        vx, vy, k = copy(s)
        for q in range(vx.shape[1]):
            vx[:k[q], q], vy[:k[q], q] = vx[:k[q], q][::-1].copy(), vy[:k[q], q][::-1].copy()
        return vx, vy, k

    out["clockwise"] = (reverse(base_a), base_b, grid, True)
    out["clockwise_both"] = (reverse(base_a), reverse(base_b), grid, True)

    def repeated(s):
        vx, vy, k = copy(s)
        sel = np.flatnonzero(k >= 4)
        vx[1, sel], vy[1, sel] = vx[0, sel], vy[0, sel]
        vx[3, sel], vy[3, sel] = vx[2, sel], vy[2, sel]
        return vx, vy, k

    out["repeated_vertices"] = (repeated(base_a), repeated(base_b), grid, True)

    def small_counts(s, seed):
        vx, vy, k = copy(s)
        k[:] = np.random.default_rng(seed).choice([1, 1, 2, 2, 3, 5], len(k))
        return vx, vy, k

    out["k1_k2"] = (small_counts(base_a, 1), small_counts(base_b, 2), grid, True)
    ta, tb = touching_poly_sets(100)
    diag = np.stack([np.arange(100), np.arange(100)], axis=1).astype(np.uint32)
    out["touching"] = (ta, tb, np.concatenate([diag, all_pairs(12, 12)]), True)
    out["equal_shapes"] = (base_a, base_a, np.concatenate([np.stack([np.arange(n)] * 2, axis=1).astype(np.uint32), grid[::7]]), True)
    out["equal_boxes"] = (ta, ta, diag, True)
    for name, scale in (("scale_1e30", 1e30), ("scale_1e-30", 1e-30), ("scale_1e-42", 1e-42), ("scale_1e18", 1e18), ("scale_1e-18", 1e-18)):
        sa = ((base_a[0].astype(np.float64) * scale).astype(F), (base_a[1].astype(np.float64) * scale).astype(F), base_a[2])
        sb = ((base_b[0].astype(np.float64) * scale).astype(F), (base_b[1].astype(np.float64) * scale).astype(F), base_b[2])
        out[name] = (sa, sb, grid, False)

    def poison(s, row, seed):
        vx, vy, k = copy(s)
        r = np.random.default_rng(seed)
        sel = r.choice(vx.shape[1], vx.shape[1] // 3, replace=False)
        junk = r.choice(np.array([np.nan, np.inf, -np.inf, 3e38, -3e38], F), sel.size)
        rows = np.zeros(sel.size, np.int64) if row == 0 else r.integers(1, k[sel])
        plane = r.integers(0, 2, sel.size)
        for q, rr, p, v in zip(sel, rows, plane, junk):
            (vx, vy)[p][rr, q] = v
        return vx, vy, k

    out["non_finite_vertex0"] = (poison(base_a, 0, 11), poison(base_b, 0, 12), grid, False)
    out["non_finite_later_vertex"] = (poison(base_a, 1, 13), poison(base_b, 1, 14), grid, False)
    # one very long edge against small ones: len2 overflows on an axis whose overlap stays finite
    vx, vy, k = copy(base_a)
    vx[:, :8], vy[:, :8], k[:8] = 0, 0, 3
    vx[1, :8], vy[2, :8] = F(1e20), rng.uniform(1e-12, 1e-10, 8).astype(F)
    out["overflowing_len2"] = ((vx, vy, k), base_b, grid, False)
    return out


def rect_sets(oracle, wl, n=500, extent=8.0, seed=7401):
    """two sets of about 500 rectangles as vertex planes f32[8][n] (the rectangles of random_obb_pose_planes)"""
    poses = wl.random_obb_pose_planes(n, seed=seed, extent=extent)
    return oracle.rects_from_poses(*poses[:5]), oracle.rects_from_poses(*poses[5:])


def quad_sets(n=200, seed=7402):
    """non-rectangular quads (random convex-or-not quadrilaterals, some degenerate): the call treats them as the boolean does"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        c = rng.uniform(-5, 5, (2, n))
        q = np.empty((8, n), F)
        for v in range(4):
            q[2 * v] = c[0] + rng.uniform(-2, 2, n)
            q[2 * v + 1] = c[1] + rng.uniform(-2, 2, n)
        q[2:4, ::9] = q[0:2, ::9]      # a repeated vertex: a zero-length edge axis
        q[:, ::31] = np.tile(q[0:2, ::31], (4, 1))      # all four vertices one point: no usable axis of its own
        out.append(q)
    return out[0], out[1]
