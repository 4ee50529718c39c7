"""Inputs shared by the manifold tests (test_manifold_ref_cpu.py, test_gpu_manifolds.py): seeded sets only, no expectations.
A polygon set is (vx f32[16][n], vy, k u8[n]), as in contact_cases.py."""
import numpy as np

import contact_ref

F = np.float32
BATCH = 4096


def random_colliding_batch(wl, n=BATCH, seed=9101):
    """-> a, b: sets of n polygons each, (A_i, B_i) the pairs: k ~ U{3..16}, every third polygon of either set clockwise, half
    axes 0.15 .. 2.5.  Three pairs in four collide (B placed anywhere within reach of A, kept under contact_ref's hit).  Every
    fourth is a corner-to-corner NEAR MISS, built, not drawn: on a colliding pair the deepest vertex of the incident polygon
    almost always lies inside the reference edge's slab (beyond an end of the edge, the neighbouring edge's axis tends to give a
    smaller depth: random colliding pairs alone gave P0_CLIPPED and OUTSIDE_SLAB shares of 0 %), so those two come from pairs
    whose closest features are two vertices — the speculative contacts the manifold call serves as well.  For a random direction t, B is moved until its lowest vertex along t sits
    0.02 .. 0.5 beyond A's highest vertex along t: each corner then lies in the other's corner region, outside both slabs."""
    rng = np.random.default_rng(seed)
    keep = [[], []]
    have = 0
    while have < n:
        m = 2 * (n - have) + 64
        sets = []
        for side in range(2):
            vx, vy, k = np.zeros((16, m), F), np.zeros((16, m), F), rng.integers(3, 17, m).astype(np.uint8)
            for q in range(m):
                xs, ys = wl.convex_polygon(int(k[q]), rng, rng.uniform(0.15, 2.5), rng.uniform(0.15, 2.5), rng.uniform(0, 2 * np.pi),
                                           clockwise=bool(rng.integers(0, 3) == 0))
                vx[:k[q], q], vy[:k[q], q] = xs, ys
            sets.append((vx, vy, k))
        reach = rng.uniform(0.0, 3.5, m)
        turn = rng.uniform(0, 2 * np.pi, m)
        cx, cy = rng.uniform(-3, 3, (2, m))
        ox, oy = [cx, cx + reach * np.cos(turn)], [cy, cy + reach * np.sin(turn)]
        # the near misses: corner against corner along (cos turn, sin turn)
        near = np.arange(m) % 4 == 0
        real = [np.arange(16)[:, None] < s[2][None, :] for s in sets]
        along = [np.where(real[side], sets[side][0] * np.cos(turn) + sets[side][1] * np.sin(turn), -np.inf if side == 0 else np.inf) for side in range(2)]
        va, vb = np.argmax(along[0], axis=0), np.argmin(along[1], axis=0)
        cols = np.arange(m)
        gap = rng.uniform(0.02, 0.5, m)
        ox[1] = np.where(near, cx + sets[0][0][va, cols] + gap * np.cos(turn) - sets[1][0][vb, cols], ox[1])
        oy[1] = np.where(near, cy + sets[0][1][va, cols] + gap * np.sin(turn) - sets[1][1][vb, cols], oy[1])
        for side, (vx, vy, k) in enumerate(sets):
            vx += np.where(real[side], ox[side].astype(F)[None, :], F(0))
            vy += np.where(real[side], oy[side].astype(F)[None, :], F(0))
        c = contact_ref.poly_contacts(sets[0], sets[1], np.arange(m), np.arange(m))
        take = np.where(near, c["hit"] == 0, c["hit"] == 1)
        for side in range(2):
            keep[side].append(tuple(x[..., take] for x in sets[side]))
        have += int(take.sum())
    a, b = (tuple(np.ascontiguousarray(np.concatenate([s[p] for s in keep[side]], axis=-1)[..., :n]) for p in range(3)) for side in range(2))
    return a, b


def shuffled(n=BATCH, seed=9102):
    """a fixed permutation of 0 .. n-1"""
    return np.random.default_rng(seed).permutation(n)
