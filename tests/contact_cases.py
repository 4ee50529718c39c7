"""Inputs shared by the tests of the list-driven queries (test_contact_ref_cpu.py, test_contact_near_ties_cpu.py, pair_list_harness.py
with its dense sets and hard batches, test_gpu_pair_list_contract.py, pair_list_graph_check.py, test_gpu_contacts.py,
test_gpu_contact_ties.py, test_gpu_manifolds.py, test_gpu_distances.py) and tests/tools/contact_fuzz.py: seeded sets and pair lists
only, no expectations.  A polygon set is (vx f32[rows][n], vy, k u8[n]); a rectangle set is planes f32[8][n]."""
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


# ---- near-ties: pairs whose two best axes are NOT parallel and 2^-26 .. 2^-15 apart (relative), where the first pass of the contact
# kernel has to tell "decided" from "too close to call" (DESIGN.md 5.11).  Everything below is float64 geometry rounded to float32
# at the end; the pair (A_i, B_i) is entry i of both sets.

def _depths64(A, ka, B, kb, edge_axes):
    """A, B f64 [m][K][2] with the slots at and beyond k holding vertex 0; -> unit axes [m][2K][2] (A's K edge slots, then B's), the
    overlap along each [m][2K] (+inf on a dead slot) and its rate of change [m][2K] (+-1) when B moves along the unit axis.
    edge_axes: the axis is the edge vector (rectangle entry point), otherwise the edge's normal (polygon entry point)."""
    K = A.shape[1]
    e = np.concatenate([np.roll(A, -1, axis=1) - A, np.roll(B, -1, axis=1) - B], axis=1)
    live = np.concatenate([np.arange(K)[None, :] < ka[:, None], np.arange(K)[None, :] < kb[:, None]], axis=1)
    n = e if edge_axes else np.stack([-e[..., 1], e[..., 0]], axis=-1)
    length = np.hypot(n[..., 0], n[..., 1])
    live &= length > 0
    u = n / np.where(live, length, 1.0)[..., None]
    o1, o2 = np.empty(length.shape), np.empty(length.shape)
    for s in range(0, len(A), 512):        # (in slices that stay in the cache)
        c = slice(s, s + 512)
        pa = A[c, :, None, 0] * u[c, None, :, 0] + A[c, :, None, 1] * u[c, None, :, 1]       # [pair][vertex][axis]
        pb = B[c, :, None, 0] * u[c, None, :, 0] + B[c, :, None, 1] * u[c, None, :, 1]
        o1[c], o2[c] = pa.max(axis=1) - pb.min(axis=1), pb.max(axis=1) - pa.min(axis=1)
    return u, np.where(live, np.minimum(o1, o2), np.inf), np.where(o1 <= o2, -1.0, 1.0)


def _random_convex64(rng, m, K, kmin, min_gap=0.0):
    """m convex counter-clockwise polygons of kmin..K vertices around the origin, f64 [m][K][2] padded with vertex 0, and k [m];
    min_gap > 0 (K == kmin only): consecutive angles at least that far apart"""
    k = rng.integers(kmin, K + 1, m)
    if min_gap > 0:
        cuts = np.sort(rng.uniform(0, 2 * np.pi - K * min_gap, (m, K)), axis=1) + min_gap * np.arange(K)[None, :]
        ang = cuts + rng.uniform(0, 2 * np.pi, (m, 1))
    else:
        ang = rng.uniform(0, 2 * np.pi, (m, K))
        ang[np.arange(K)[None, :] >= k[:, None]] = np.inf
        ang = np.sort(ang, axis=1)
    ang = np.where(np.isfinite(ang), ang, ang[:, :1])
    a, b, rot = rng.uniform(0.5, 2.0, (m, 1)), rng.uniform(0.5, 2.0, (m, 1)), rng.uniform(0, 2 * np.pi, (m, 1))
    x, y = a * np.cos(ang), b * np.sin(ang)
    return np.stack([np.cos(rot) * x - np.sin(rot) * y, np.sin(rot) * x + np.cos(rot) * y], axis=-1), k


def near_tie_gaps(rng, m, g_log2=(-26.0, -15.0)):
    """m relative gaps g: either sign, |g| log-uniform in 2^g_log2[0] .. 2^g_log2[1]"""
    return np.where(rng.random(m) < 0.5, -1.0, 1.0) * np.exp2(rng.uniform(g_log2[0], g_log2[1], m))


def _near_tie_pairs(rng, n, K, kmin, edge_axes, g_log2):
    """-> A, ka, B, kb (f32 coordinates in f64 arrays [n][K][2]): colliding convex pairs, depth d1 > 0.05 on their best axis n1; B is
    moved perpendicular to n1 until the best axis that is not parallel to n1 (|cross| > 0.3) has depth d1 * (1 + g); the pair is
    kept when, rounded to float32, those two axes are its best two and the third is at least 1e-3 (relative) further.  (Waiting
    for a random pair whose two best axes are already non-parallel gives the same pairs and rejects nine candidates in ten.)"""
    got, have = [], 0
    for _ in range(40):
        m = max(256, (n - have) * 9 // 4)
        A, ka = _random_convex64(rng, m, K, kmin, 0.35 if edge_axes else 0.0)
        B, kb = _random_convex64(rng, m, K, kmin, 0.35 if edge_axes else 0.0)
        A += rng.uniform(-1.5, 1.5, (m, 1, 2))
        turn, far = rng.uniform(0, 2 * np.pi, m), rng.uniform(0.0, 2.5, m)
        B += A.mean(axis=1, keepdims=True) + np.stack([far * np.cos(turn), far * np.sin(turn)], axis=-1)[:, None, :]
        g = near_tie_gaps(rng, m, g_log2)
        u, d, rate = _depths64(A, ka, B, kb, edge_axes)
        rows = np.arange(m)
        i1 = np.argmin(d, axis=1)
        u1, d1 = u[rows, i1], d[rows, i1]
        # the runner-up to be: the best axis that is not parallel to the best one
        across = np.abs(u1[:, None, 0] * u[..., 1] - u1[:, None, 1] * u[..., 0]) > 0.3
        i2 = np.argmin(np.where(across, d, np.inf), axis=1)
        u2, d2 = u[rows, i2], d[rows, i2]
        t = np.stack([-u1[:, 1], u1[:, 0]], axis=-1)
        along = np.einsum("mc,mc->m", t, u2)          # = cross(u1, u2)
        ok = (d1 > 0.05) & np.isfinite(d2) & across[rows, i2]
        if edge_axes:        # no two parallel edges inside a quad either
            for q in (A, B):
                ev = np.roll(q, -1, axis=1) - q
                ev /= np.hypot(ev[..., 0], ev[..., 1])[..., None]
                for x, y in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
                    ok &= np.abs(ev[:, x, 0] * ev[:, y, 1] - ev[:, x, 1] * ev[:, y, 0]) > 0.2
        step = (d1[ok] * (1 + g[ok]) - d2[ok]) / (rate[rows, i2][ok] * along[ok])
        A, ka, B, kb, i1, i2 = A[ok], ka[ok], B[ok], kb[ok], i1[ok], i2[ok]
        B = B + (step[:, None] * t[ok])[:, None, :]
        A, B = A.astype(F).astype(np.float64), B.astype(F).astype(np.float64)
        _, d, _ = _depths64(A, ka, B, kb, edge_axes)
        order = np.argpartition(d, 2, axis=1)[:, :3]
        low = np.sort(np.take_along_axis(d, order, axis=1), axis=1)
        best, second, third = low[:, 0], low[:, 1], low[:, 2]
        rows = np.arange(len(d))
        ok = np.maximum(d[rows, i1], d[rows, i2]) == second          # the two chosen axes are the best two
        ok &= (best > 0.05) & (second - best <= 4 * 2.0 ** g_log2[1] * best) & (third - best >= 1e-3 * best)
        got.append((A[ok], ka[ok], B[ok], kb[ok]))
        have += int(ok.sum())
        if have >= n:
            return tuple(np.concatenate(x)[:n] for x in zip(*got))
    raise RuntimeError("the near-tie construction keeps too few pairs")


def _as_poly_set(V, k, rows=16):
    vx, vy = np.zeros((rows, len(k)), F), np.zeros((rows, len(k)), F)
    real = np.arange(V.shape[1])[:, None] < k[None, :]
    vx[:V.shape[1]], vy[:V.shape[1]] = np.where(real, V[..., 0].T, 0), np.where(real, V[..., 1].T, 0)
    return vx, vy, k.astype(np.uint8)


def _as_planes(V):
    return np.ascontiguousarray(V[:, :4].reshape(len(V), 8).T.astype(F))


def near_tie_poly_sets(n=20000, seed=8101, g_log2=(-26.0, -15.0)):
    """polygon sets a, b of n polygons each, k in 3..16: (A_i, B_i) is a near-tied pair of the polygon entry point"""
    A, ka, B, kb = _near_tie_pairs(np.random.default_rng(seed), n, 16, 3, False, g_log2)
    return _as_poly_set(A, ka), _as_poly_set(B, kb)


def near_tie_quad_sets(n=4000, seed=8102, g_log2=(-26.0, -15.0)):
    """planes a, b f32[8][n] of convex quads without parallel edges, near-tied over the eight edge-VECTOR axes of rect_collide"""
    A, _, B, _ = _near_tie_pairs(np.random.default_rng(seed), n, 4, 4, True, g_log2)
    return _as_planes(A), _as_planes(B)


def near_tie_box_sets(n=4000, seed=8103, g_log2=(-26.0, -15.0)):
    """-> (a, b) as 4-gon polygon sets, (a, b) as planes f32[8][n]: boxes of unequal sizes that share a rotation (every fourth: angle 0
    and coordinates that are multiples of 1/64, up to the gap itself), overlapping by ex along one side and ex * (1 + g) along the
    other, each box starting at a random vertex: four near-tied axes per direction"""
    rng = np.random.default_rng(seed)
    plain = np.arange(n) % 4 == 0

    def pick(lo, hi):
        x = rng.uniform(lo, hi, n)
        return np.where(plain, np.round(x * 64) / 64, x)

    wa, ha, wb, hb = pick(0.5, 2.0), pick(0.5, 2.0), pick(0.5, 2.0), pick(0.5, 2.0)    # half sizes
    cx, cy, ex = pick(-2.0, 2.0), pick(-2.0, 2.0), pick(0.0625, 0.45)
    ey = ex * (1 + near_tie_gaps(rng, n, g_log2))
    dx, dy = (wa + wb - ex) * rng.choice([-1.0, 1.0], n), (ha + hb - ey) * rng.choice([-1.0, 1.0], n)
    rot = np.where(plain, 0.0, rng.uniform(0, 2 * np.pi, n))
    c, s = np.cos(rot), np.sin(rot)
    corner = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], np.float64)
    out = []
    for w, h, ox, oy in ((wa, ha, 0 * dx, 0 * dy), (wb, hb, dx, dy)):
        first = rng.integers(0, 4, n)
        lx = ox[:, None] + w[:, None] * corner[(first[:, None] + np.arange(4)[None, :]) % 4, 0]
        ly = oy[:, None] + h[:, None] * corner[(first[:, None] + np.arange(4)[None, :]) % 4, 1]
        out.append(np.stack([cx[:, None] + c[:, None] * lx - s[:, None] * ly, cy[:, None] + s[:, None] * lx + c[:, None] * ly], axis=-1))
    four = np.full(n, 4)
    return (_as_poly_set(out[0], four), _as_poly_set(out[1], four)), (_as_planes(out[0]), _as_planes(out[1]))


# ---- the first pass's window: len2 in [2^-100, 2^100] and |o| < 2^60 (c2d_contact.hip FastPick::add); outside it a pair is hard

WINDOW_EDGE_K = tuple(range(-54, -45)) + tuple(range(26, 33)) + tuple(range(46, 55))
MIXED_SCALE_K = (0, 29, 30, 49, 50, 51, -49, -50, -51, 60, -60)


def scaled_poly_set(s, k):
    """every coordinate times 2^k exactly (k: one exponent, or one per polygon)"""
    e = np.broadcast_to(np.asarray(k, np.int32), s[2].shape)[None, :]
    return np.ldexp(s[0], e).astype(F), np.ldexp(s[1], e).astype(F), s[2]


def window_edge_poly_batch(wl):
    """-> a, b, pairs, k_of_pair: the 48 x 48 batch of hard_poly_batches (seeds 7302, 7303; all 2304 pairs) once per k of
    WINDOW_EDGE_K, scaled by 2^k: polygons 48 q .. 48 q + 47 of both sets carry WINDOW_EDGE_K[q]"""
    base_a = wl.random_convex_polygon_set(48, seed=7302, extent=3.0)
    base_b = wl.random_convex_polygon_set(48, seed=7303, extent=3.0)
    sa, sb = [scaled_poly_set(base_a, k) for k in WINDOW_EDGE_K], [scaled_poly_set(base_b, k) for k in WINDOW_EDGE_K]
    a, b = (tuple(np.concatenate([s[p] for s in ss], axis=-1) for p in range(3)) for ss in (sa, sb))
    grid = all_pairs(48, 48)
    pairs = np.concatenate([grid + np.uint32(48 * q) for q in range(len(WINDOW_EDGE_K))])
    return a, b, pairs, np.repeat(np.array(WINDOW_EDGE_K), len(grid))


def window_edge_rect_batch(oracle, wl):
    """the same for 200 rectangles per set (rect_sets): every 17th of the 200 x 200 pairs, once per k"""
    ra, rb = rect_sets(oracle, wl, n=200)
    a = np.concatenate([np.ldexp(ra, k).astype(F) for k in WINDOW_EDGE_K], axis=1)
    b = np.concatenate([np.ldexp(rb, k).astype(F) for k in WINDOW_EDGE_K], axis=1)
    grid = all_pairs(200, 200)[::17]
    pairs = np.concatenate([grid + np.uint32(200 * q) for q in range(len(WINDOW_EDGE_K))])
    return a, b, pairs, np.repeat(np.array(WINDOW_EDGE_K), len(grid))


def mixed_scale_poly_batch(wl, n=1100):
    """-> a, b, pairs, k_of_pair: polygon i of both sets is scaled by 2^MIXED_SCALE_K[i % 11]; the list is the diagonal plus
    (i, i - 11) and (i, i + 11), row-major: every pair joins two polygons of one scale, and eleven scales alternate inside a wave"""
    a, b = dense_poly_sets(wl, n=n, extent=2.0, seeds=(8201, 8202))
    a, b = tuple(x[..., :n] for x in a), tuple(x[..., :n] for x in b)
    k = np.array(MIXED_SCALE_K)[np.arange(n) % len(MIXED_SCALE_K)]
    i = np.repeat(np.arange(n), 3)
    j = i + np.tile([-11, 0, 11], n)
    keep = (j >= 0) & (j < n)
    pairs = np.stack([i[keep], j[keep]], axis=1).astype(np.uint32)
    return scaled_poly_set(a, k), scaled_poly_set(b, k), pairs, k[i[keep]]


def outside_window(terms):
    """per pair: has a live axis (len2 != 0) with len2 outside [2^-100, 2^100]; has one with |o| >= 2^60 (or a NaN in either)"""
    live = terms["len2"] != 0
    with np.errstate(all="ignore"):
        len2_out = live & ~((terms["len2"] >= F(2.0 ** -100)) & (terms["len2"] <= F(2.0 ** 100)))
        o_out = live & ~(np.abs(terms["o"]) < F(2.0 ** 60))
    return len2_out.any(axis=1), o_out.any(axis=1)
