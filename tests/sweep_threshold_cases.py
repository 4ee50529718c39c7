"""The station scene of tests/threshold_cases.py set in motion: rows that sit exactly on the pair search's path switches (16 / 17 and
512 / 513 hits, 1024 / 1025 walked sorted entries) only THROUGH their motion.  Each probe of A, a diamond of half-diagonal 1, starts
RUN to the left of its station and moves by (+RUN, 0): at t = 0 its box is far from every box of the station's pile, at t = 1 it sits
on the station's centre.  The pile holds h hitters around the centre, which the probe reaches, and c near misses up and to the right
of the centre and down and to the right: inside the probe's swept box, outside every position the diamond takes.  No expectations
live here: tests/test_sweep_threshold_cases_cpu.py proves the construction on the reference, tests/test_gpu_sweep_broad.py runs it."""
import numpy as np

import threshold_cases as tc

F32 = np.float32
RUN = 20.0                 # how far a probe travels; its swept box is RUN + 2 wide
PITCH = 512.0              # stations sit this far apart: a probe's query (three cells of about RUN + 2 .. 1.25 (RUN + 2)) sees one pile only
PER_ROW = 8


def station_plan():
    """[(h, c)]: hitters and near misses of each station; a probe's query walks h + c sorted entries"""
    hs = [0, 1, 13, 15, 16, 17, 18, 64, 509, 511, 512, 513, 514, 700]
    plan = [(h, 0) for h in hs]
    for h in (0, 13, 16, 17, 512, 513):
        plan += [(h, walked - h) for walked in (1023, 1024, 1025, 1026)]
    return plan


def moving_station_scene(plan=None, covers=0, seed=1):
    """(a, b, a_motion, info): a, b polygon sets of 4-gons (vx, vy f32[4][n], k u8[n]); a_motion (dx, dy) f32[n_a]; B stands still.
    info: h, c i64[stations]; centre f64[2][stations]; owner i64[n_b] (the station of each object of B, -1 for a cover)."""
    plan = station_plan() if plan is None else plan
    assert len(plan) >= 5 and 0 <= covers <= 4      # (as threshold_cases.station_scene: the cell size must stay the probes')
    rng = np.random.default_rng(seed)
    t = np.arange(len(plan))
    h, c = np.array([p[0] for p in plan]), np.array([p[1] for p in plan])
    centre = np.stack([PITCH * (t % PER_ROW) + 0.37 * t, PITCH * (t // PER_ROW) + 0.61 * t])
    sx = centre[0] - RUN                                                   # where the probes start
    a = np.stack([sx + 1, centre[1], sx, centre[1] + 1, sx - 1, centre[1], sx, centre[1] - 1])
    piles, owner = [], []
    for s in t:
        n_h, n_c = int(h[s]), int(c[s])
        hit = tc._squares(centre[0, s] + rng.uniform(-0.3, 0.3, n_h), centre[1, s] + rng.uniform(-0.3, 0.3, n_h), rng.uniform(0.05, 0.15, n_h))
        sy = rng.choice([-1.0, 1.0], n_c)
        miss = tc._squares(centre[0, s] + rng.uniform(0.75, 0.85, n_c), centre[1, s] + sy * rng.uniform(0.75, 0.85, n_c), rng.uniform(0.05, 0.1, n_c))
        piles += [hit, miss]
        owner.append(np.full(n_h + n_c, s))
    b, owner = np.concatenate(piles, axis=1), np.concatenate(owner)
    perm = rng.permutation(b.shape[1])
    b, owner = b[:, perm], owner[perm]
    mid = centre.mean(axis=1)
    cover = tc._squares(np.full(covers, mid[0]), np.full(covers, mid[1]), np.full(covers, 1e4))
    b, owner = np.concatenate([b, cover], axis=1), np.concatenate([owner, np.full(covers, -1)])
    motion = (np.full(len(plan), RUN, F32), np.zeros(len(plan), F32))
    return tc.as_polygons(a.astype(F32), 4), tc.as_polygons(b.astype(F32), 4), motion, {"h": h, "c": c, "centre": centre, "owner": owner}
