"""The station scene of tests/threshold_cases.py for the proximity pair search: rows that sit exactly on the pair search's path switches
(16 / 17 and 512 / 513 listed pairs, 1024 / 1025 walked sorted entries) only THROUGH the margin.  Each probe of A is a diamond of
half-diagonal 1 on its station's centre.  The pile holds h neighbours, small squares whose centres lie at an L1 distance of 2 .. 3 from
the centre: separated from the diamond by at least 0.49, and within MARGIN of it; and c near misses about (+-4.6, +-4.6) from the centre:
their boxes meet the probe's (both are widened by MARGIN / 2), their distance from the diamond is above 5.5.  No expectations live
here: tests/test_near_threshold_cases_cpu.py proves the construction on the reference, tests/test_gpu_near_broad.py runs it."""
import numpy as np

import threshold_cases as tc

F32 = np.float32
MARGIN = 4.0
PITCH = 512.0              # stations sit this far apart: a probe's query sees one pile only
PER_ROW = 8


def station_plan():
    """[(h, c)]: neighbours and near misses of each station; a probe's query walks h + c sorted entries"""
    hs = [0, 1, 13, 15, 16, 17, 18, 64, 509, 511, 512, 513, 514, 700]
    plan = [(h, 0) for h in hs]
    for h in (0, 13, 16, 17, 512, 513):
        plan += [(h, walked - h) for walked in (1023, 1024, 1025, 1026)]
    return plan


def near_station_scene(plan=None, covers=0, seed=1):
    """(a, b, info): a, b polygon sets of 4-gons (vx, vy f32[4][n], k u8[n]).  info: h, c i64[stations]; centre f64[2][stations];
    owner i64[n_b] (the station of each object of B, -1 for a cover: a square of half-width 1e4 over the whole scene)."""
    plan = station_plan() if plan is None else plan
    assert len(plan) >= 5 and 0 <= covers <= 4      # (as threshold_cases.station_scene: the cell size must stay the probes')
    rng = np.random.default_rng(seed)
    t = np.arange(len(plan))
    h, c = np.array([p[0] for p in plan]), np.array([p[1] for p in plan])
    centre = np.stack([PITCH * (t % PER_ROW) + 0.37 * t, PITCH * (t // PER_ROW) + 0.61 * t])
    a = np.stack([centre[0] + 1, centre[1], centre[0], centre[1] + 1, centre[0] - 1, centre[1], centre[0], centre[1] - 1])
    piles, owner = [], []
    for s in t:
        n_h, n_c = int(h[s]), int(c[s])
        l1, share = rng.uniform(2.0, 3.0, n_h), rng.uniform(0.0, 1.0, n_h)
        near = tc._squares(centre[0, s] + rng.choice([-1.0, 1.0], n_h) * l1 * share, centre[1, s] + rng.choice([-1.0, 1.0], n_h) * l1 * (1 - share),
                           rng.uniform(0.05, 0.15, n_h))
        miss = tc._squares(centre[0, s] + rng.choice([-1.0, 1.0], n_c) * rng.uniform(4.5, 4.7, n_c),
                           centre[1, s] + rng.choice([-1.0, 1.0], n_c) * rng.uniform(4.5, 4.7, n_c), rng.uniform(0.05, 0.1, n_c))
        piles += [near, miss]
        owner.append(np.full(n_h + n_c, s))
    b, owner = np.concatenate(piles, axis=1), np.concatenate(owner)
    perm = rng.permutation(b.shape[1])
    b, owner = b[:, perm], owner[perm]
    mid = centre.mean(axis=1)
    cover = tc._squares(np.full(covers, mid[0]), np.full(covers, mid[1]), np.full(covers, 1e4))
    b, owner = np.concatenate([b, cover], axis=1), np.concatenate([owner, np.full(covers, -1)])
    return tc.as_polygons(a.astype(F32), 4), tc.as_polygons(b.astype(F32), 4), {"h": h, "c": c, "centre": centre, "owner": owner}
