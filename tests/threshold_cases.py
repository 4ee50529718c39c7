"""Seeded scene builders that put rows and waves exactly on the pair searches' path switches.  No expectations live here:
tests/test_threshold_cases_cpu.py proves the constructions on the CPU oracle, tests/test_gpu_sat_broad_thresholds.py and
tests/test_gpu_sat_poly_cross_wave_counts.py run them through the kernels."""
import numpy as np

F32 = np.float32

# The constants the scenes straddle, and where each one lives.
SWITCHES = {
    "kShortHits": (16, "csrc/c2d_broad.hpp:26"),         # hits a row may have for the short emit path (one thread, LDS insertion sort)
    "kMidHits": (512, "csrc/c2d_broad.hpp:27"),          # hits a listed regular row may have for the wave path (hits[wave][511] is the last slot)
    "kCandidateCap": (1024, "csrc/c2d_broad.hpp:28"),    # sorted entries a row may walk before it is left to the all-columns walk
    "kPcSerialMin": (16, "csrc/c2d_poly_cross.hip:55"),  # undecided rows of a wave from which phase 2 runs one pair per lane
}
SHORT_HITS, MID_HITS, CANDIDATE_CAP, PC_SERIAL_MIN = (SWITCHES[k][0] for k in ("kShortHits", "kMidHits", "kCandidateCap", "kPcSerialMin"))

STATION_PITCH = 64.0      # stations sit this far apart
STATION_ROW = 8           # stations per grid row
COVER_HALF = 5e3          # a cover is a square of side 1e4


def station_plan():
    """[(h, c)]: hitters and near misses of each station; a probe's query walks h + c sorted entries"""
    # (12 and 508 put 15 and 511 hits into the run with three covers as well)
    hs = [0, 1] + list(range(12, 20)) + list(range(61, 68)) + list(range(508, 516)) + [700]
    plan = [(h, 0) for h in hs]
    for h in (0, 13, 16, 17, 512, 513):
        plan += [(h, walked - h) for walked in range(1021, 1028)]
    return plan


def _squares(cx, cy, half):
    """axis-aligned squares as rectangle planes f64[8][n], counter-clockwise from the lower left corner"""
    return np.stack([cx - half, cy - half, cx + half, cy - half, cx + half, cy + half, cx - half, cy + half])


def station_scene(plan=None, covers=0, seed=1):
    """(a f32[8][n_a], b f32[8][n_b], info).  A holds one probe per station: a diamond of half-diagonal 1.  B holds each station's
    pile, h hitters that collide with the probe and c near misses whose box meets the probe's box while the diamond's own edge
    normal separates them, shuffled by a fixed permutation, and then `covers` squares over the whole scene.
    info: h, c i64[stations]; centre f64[2][stations]; owner i64[n_b] (the station of each object of B, -1 for a cover)."""
    plan = station_plan() if plan is None else plan
    assert len(plan) >= 5, "with fewer probes the probes themselves lie above the cell size and turn wild"
    assert 0 <= covers <= 4, "more than four boxes above the probes' extent would move the cell size"
    rng = np.random.default_rng(seed)
    t = np.arange(len(plan))
    h, c = np.array([p[0] for p in plan]), np.array([p[1] for p in plan])
    # the incommensurate offsets make the probes straddle the cell borders differently
    centre = np.stack([STATION_PITCH * (t % STATION_ROW) + 0.37 * t, STATION_PITCH * (t // STATION_ROW) + 0.61 * t])
    a = np.stack([centre[0] + 1, centre[1], centre[0], centre[1] + 1, centre[0] - 1, centre[1], centre[0], centre[1] - 1])
    piles, owner = [], []
    for s in t:
        n_h, n_c = int(h[s]), int(c[s])
        hit = _squares(centre[0, s] + rng.uniform(-0.3, 0.3, n_h), centre[1, s] + rng.uniform(-0.3, 0.3, n_h), rng.uniform(0.05, 0.15, n_h))
        sx, sy = rng.choice([-1.0, 1.0], n_c), rng.choice([-1.0, 1.0], n_c)
        miss = _squares(centre[0, s] + sx * rng.uniform(0.75, 0.85, n_c), centre[1, s] + sy * rng.uniform(0.75, 0.85, n_c), rng.uniform(0.05, 0.1, n_c))
        piles += [hit, miss]
        owner.append(np.full(n_h + n_c, s))
    b, owner = np.concatenate(piles, axis=1), np.concatenate(owner)
    perm = rng.permutation(b.shape[1])   # key order, index order and the order inside a cell all differ
    b, owner = b[:, perm], owner[perm]
    mid = centre.mean(axis=1)
    cover = _squares(np.full(covers, mid[0]), np.full(covers, mid[1]), np.full(covers, COVER_HALF))
    b, owner = np.concatenate([b, cover], axis=1), np.concatenate([owner, np.full(covers, -1)])
    return a.astype(F32), b.astype(F32), {"h": h, "c": c, "centre": centre, "owner": owner}


def self_shuffle(n_a, n, seed=2):
    """The fixed order in which the union (probes 0 .. n_a - 1, then the piles) runs against itself with the probes shuffled in:
    order[p] is the object at index p.  The probes land, in a shuffled order of their own, on scattered indices of the first
    fifth, so that in the strict upper triangle a probe still sees at least four fifths of its pile; the piles fill the rest."""
    rng = np.random.default_rng(seed)
    order = np.empty(n, np.int64)
    at = np.sort(rng.choice(n // 5, n_a, replace=False))
    rest = np.ones(n, bool)
    rest[at] = False
    order[at] = rng.permutation(n_a)
    order[rest] = n_a + rng.permutation(n - n_a)
    return order


def as_polygons(planes, rows):
    """rectangle planes f32[8][n] -> the same vertices as 4-gons (vx, vy f32[rows][n], k u8[n]); padded slots hold NaN"""
    n = planes.shape[1]
    vx, vy = np.full((rows, n), np.nan, F32), np.full((rows, n), np.nan, F32)
    vx[:4], vy[:4] = planes[0::2], planes[1::2]
    return vx, vy, np.full(n, 4, np.uint8)


WAVE = 64
WAVE_ROWS = [64, 64, 64, 64, 64, 37]          # one full block of four waves, one full wave, one partial wave
WAVE_KINDS = [3, 5, 16, None, None, None]     # vertex counts of each wave's rows; None: mixed 3 .. 16
WAVE_LINE = 10_000.0                          # wave w lies on the line y = WAVE_LINE * w
SLOT_PITCH = 4.0                              # slot s of a wave sits at x = SLOT_PITCH * s
BAR_LEFT = -6.0                               # every bar starts here, left of slot 0's polygon
BAR_HALF_HEIGHT = 0.25


def bar_vertex_count(w, m):
    """4 for even m; 5 or 7 for odd m, alternating with m and with the wave"""
    return 4 if m % 2 == 0 else (5 if (m // 2 + w) % 2 == 0 else 7)


def wave_count_scene(seed=1):
    """(a, b, info): polygon sets (vx, vy f32[16][n], k u8[n]), NaN in padded slots.
    A: the rows of wave w are convex polygons inside the unit circle around (SLOT_PITCH * slot, WAVE_LINE * w) that contain its
    centre; a fixed permutation per wave deals the slots to the lanes.
    B: for every wave w and every m in 0 .. 64 a bar along the wave's line from BAR_LEFT to the middle of the gap behind slot m - 1:
    it meets exactly the rows of wave w whose slot is below m.  Column (w, m) is 65 w + m.
    info: wave i64[n_a], slot i64[n_a]; col_wave, col_m i64[n_b]."""
    rng = np.random.default_rng(seed)
    n_a = sum(WAVE_ROWS)
    ax, ay, ak = np.full((16, n_a), np.nan), np.full((16, n_a), np.nan), np.zeros(n_a, np.uint8)
    wave, slot = np.repeat(np.arange(len(WAVE_ROWS)), WAVE_ROWS), np.zeros(n_a, np.int64)
    i = 0
    for w, rows in enumerate(WAVE_ROWS):
        perm = rng.permutation(WAVE)
        for r in range(rows):
            k = WAVE_KINDS[w] or int(rng.integers(3, 17))
            # near-regular angles: the largest gap stays below 180 degrees, so the centre is strictly inside
            ang = 2 * np.pi * (np.arange(k) + rng.uniform(-0.15, 0.15, k)) / k + rng.uniform(0, 2 * np.pi)
            rad = rng.uniform(0.6, 1.0, k)
            ax[:k, i], ay[:k, i] = SLOT_PITCH * perm[r] + rad * np.cos(ang), WAVE_LINE * w + rad * np.sin(ang)
            ak[i], slot[i] = k, perm[r]
            i += 1
    n_b = len(WAVE_ROWS) * (WAVE + 1)
    bx, by, bk = np.full((16, n_b), np.nan), np.full((16, n_b), np.nan), np.zeros(n_b, np.uint8)
    col_wave, col_m = np.repeat(np.arange(len(WAVE_ROWS)), WAVE + 1), np.tile(np.arange(WAVE + 1), len(WAVE_ROWS))
    for j in range(n_b):
        w, m = int(col_wave[j]), int(col_m[j])
        y, right, up = WAVE_LINE * w, SLOT_PITCH * m - 2.0, BAR_HALF_HEIGHT
        k = bar_vertex_count(w, m)
        # Counter-clockwise from the lower right corner.  Both short ends stay flat and vertical: phase 1 tries the edge whose
        # (-ey, ex) points from the bar's mean towards the row, which for a counter-clockwise bar is the FAR end (the left one for a
        # row to the right), and that axis +-x must separate.  The extra vertices sit as a slight bulge on the long edges.
        left, mid, bulge = BAR_LEFT, (BAR_LEFT + right) / 2, 1.5 * up
        top = {4: [], 5: [(mid, y + bulge)], 7: [(right - 2.0, y + bulge), (left + 2.0, y + bulge)]}[k]
        bottom = [(mid, y - bulge)] if k == 7 else []
        pts = [(right, y - up), (right, y + up)] + top + [(left, y + up), (left, y - up)] + bottom
        xs, ys = [q[0] for q in pts], [q[1] for q in pts]
        bx[:k, j], by[:k, j], bk[j] = xs, ys, k
    info = {"wave": wave, "slot": slot, "col_wave": col_wave, "col_m": col_m}
    return (ax.astype(F32), ay.astype(F32), ak), (bx.astype(F32), by.astype(F32), bk), info
