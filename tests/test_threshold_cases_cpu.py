"""CPU proof of the scenes of tests/threshold_cases.py: the GPU tests cannot see which route a row or a wave took, so the scenes
guarantee it by construction, and these tests check the construction: hits on the oracle, boxes and cell size on the CPU models of
the kernels' boxes, and the undecided rows of a wave on a numpy restatement of the mask kernel's phase 1.  Every comparison is count
against count or mask against mask."""
import numpy as np
import pytest

import threshold_cases as tc
from test_broad_margin_cpu import broad_boxes
from test_poly_broad_margin_cpu import pbb


@pytest.fixture(scope="module", params=[0, 3])
def stations(request):
    return request.param, tc.station_scene(covers=request.param, seed=1)


def aabb(planes):
    return np.stack([planes[0::2].min(0), planes[1::2].min(0), planes[0::2].max(0), planes[1::2].max(0)]).astype(np.float64)


def meet(ba, bb, grow):
    """bool [n_a][n_b]: the boxes of a, each side moved outward by `grow`, meet the boxes of b"""
    ax0, ay0, ax1, ay1 = (ba[k][:, None] + s * grow for k, s in zip(range(4), (-1, -1, 1, 1)))
    return (ax0 <= bb[2]) & (bb[0] <= ax1) & (ay0 <= bb[3]) & (bb[1] <= ay1)


def rect_hits(oracle, a, b):
    n_a, n_b = a.shape[1], b.shape[1]
    res, _ = oracle.sat_rect_pairs_verts(np.concatenate([np.repeat(a, n_b, axis=1), np.tile(b, n_a)]))
    return res.reshape(n_a, n_b).astype(bool)


def poly_hits(oracle, a, b):
    """rows of a one at a time: (vx, vy, k) sets of equal layout"""
    n_b = b[0].shape[1]
    out = np.empty((a[0].shape[1], n_b), bool)
    for i in range(a[0].shape[1]):
        vx = np.stack([np.repeat(a[0][:, i:i + 1], n_b, axis=1), b[0]])
        vy = np.stack([np.repeat(a[1][:, i:i + 1], n_b, axis=1), b[1]])
        out[i] = oracle.sat_poly_pairs(vx, vy, np.stack([np.repeat(a[2][i], n_b), b[2]]))[0].astype(bool)
    return out


def test_plan_straddles_every_switch():
    plan = tc.station_plan()
    h = {p[0] for p in plan if p[1] == 0}
    for sw in (tc.SHORT_HITS, tc.MID_HITS):
        assert {sw - 1, sw, sw + 1} <= h and {sw - 4, sw - 3, sw - 2} <= h, "one below, at and one above the switch, with and without three covers"
    for hh in (0, 13, tc.SHORT_HITS, tc.SHORT_HITS + 1, tc.MID_HITS, tc.MID_HITS + 1):
        walked = {p[0] + p[1] for p in plan if p[0] == hh and p[1] > 0}
        assert {tc.CANDIDATE_CAP - 1, tc.CANDIDATE_CAP, tc.CANDIDATE_CAP + 1} <= walked, hh
    assert any(p[0] > tc.MID_HITS and p[0] + p[1] <= tc.CANDIDATE_CAP for p in plan), "many hits in a cell that is not crowded"
    assert any(p[0] <= tc.SHORT_HITS and p[0] + p[1] > tc.CANDIDATE_CAP for p in plan), "a crowded cell with few hits"
    assert tc.PC_SERIAL_MIN + 1 <= tc.WAVE


def test_station_rect_hits_are_the_plan(oracle, stations):
    covers, (a, b, info) = stations
    hits = rect_hits(oracle, a, b)
    assert np.array_equal(hits.sum(1), info["h"] + covers)
    own = info["owner"][None, :] == np.arange(a.shape[1])[:, None]
    assert not (hits & ~own & (info["owner"] >= 0)[None, :]).any(), "a probe hits another station's pile"
    assert hits[:, info["owner"] < 0].all(), "a cover misses a probe"


def test_station_polygon_hits_are_the_plan(oracle, stations):
    covers, (a, b, info) = stations
    for rows in (4, 16):
        hits = poly_hits(oracle, tc.as_polygons(a, rows), tc.as_polygons(b, rows))
        assert np.array_equal(hits.sum(1), info["h"] + covers), rows


def test_station_boxes_meet_the_whole_pile_and_nothing_else(stations):
    """box-meeting columns = h + c, for the vertices' boxes moved inward and outward by more than any widening of the kernel's box"""
    covers, (a, b, info) = stations
    ba, bb = aabb(a), aabb(b)
    pile = info["owner"] >= 0
    for grow in (-0.1, 0.0, 0.1):
        assert np.array_equal(meet(ba, bb[:, pile], grow).sum(1), info["h"] + info["c"]), grow
    # nothing but a probe's own pile within 8 units of it: more than the three cells of side 2.5 that its query covers each way
    own = info["owner"][None, :] == np.arange(a.shape[1])[:, None]
    near = meet(ba, bb[:, pile], 8.0)
    assert np.array_equal(near, own[:, pile])
    # The cell size, on the CPU models of the kernels' own boxes (rectangles: broad_boxes of test_broad_margin_cpu.py; polygons:
    # tests/tools/poly_broad_box.py).  The extent histogram's bins are the float's bits >> 21: [2.0, 2.5) is one bin.  Every probe's
    # box extent lies in it, only the covers (at most four) lie above it and more than four boxes lie above every pile box: the
    # cell size is that bin's upper edge, 2.5, no probe spans more than two cells, and a probe's three cell rows hold its pile.
    models = [broad_boxes(a) + broad_boxes(b)] + [pbb.poly_broad_boxes(*tc.as_polygons(a, r)) + pbb.poly_broad_boxes(*tc.as_polygons(b, r)) for r in (4, 16)]
    for box_a, ok_a, box_b, ok_b in models:
        assert ok_a.all() and ok_b.all()
        ext_a, ext_b = np.maximum(box_a[2] - box_a[0], box_a[3] - box_a[1]), np.maximum(box_b[2] - box_b[0], box_b[3] - box_b[1])
        edge = np.float32(2.5)
        assert (ext_a.view(np.uint32) >> 21 == np.float32(2.0).view(np.uint32) >> 21).all() and (ext_a < edge).all()
        assert (ext_b[pile] < 0.5).all() and a.shape[1] > 4 and (ext_b[~pile] > edge).all() and (~pile).sum() == covers <= 4
        assert np.array_equal(meet(box_a.astype(np.float64), box_b[:, pile].astype(np.float64), 0.0).sum(1), info["h"] + info["c"])
        # a pile object's key is the cell of its box's min corner: it lies inside the probe's box, so inside the probe's cells
        own_b = np.flatnonzero(pile)
        pa = box_a[:, info["owner"][own_b]]
        assert (box_b[0, own_b] >= pa[0]).all() and (box_b[0, own_b] <= pa[2]).all() and (box_b[1, own_b] >= pa[1]).all() and (box_b[1, own_b] <= pa[3]).all()


def test_station_scene_is_shuffled(stations):
    _, (_, b, info) = stations
    owner = info["owner"][info["owner"] >= 0]
    assert (np.diff(owner) < 0).sum() > owner.size // 4, "B lies in station order"


def test_self_scene_reaches_each_emit_class(oracle):
    """the union against itself, strict upper triangle: the stations do not interact, so the per-row counts come from one oracle
    call per station.  Rows with at most 16, 17 .. 512 and more than 512 hits exist with the probes in front and shuffled in."""
    a, b, info = tc.station_scene(covers=0, seed=1)
    n_a, n = a.shape[1], a.shape[1] + b.shape[1]
    both = np.concatenate([a, b], axis=1)
    owner = np.concatenate([np.arange(n_a), info["owner"]])
    members = [np.flatnonzero(owner == s) for s in range(n_a)]
    hits = [rect_hits(oracle, both[:, idx], both[:, idx]) for idx in members]
    for order in (np.arange(n), tc.self_shuffle(n_a, n)):
        at = np.empty(n, np.int64)
        at[order] = np.arange(n)          # object order[p] sits at index p
        per_row = np.zeros(n, np.int64)
        for idx, hh in zip(members, hits):
            per_row[at[idx]] = (hh & (at[idx][None, :] > at[idx][:, None])).sum(1)
        assert (per_row <= tc.SHORT_HITS).sum() > 100
        assert ((per_row > tc.SHORT_HITS) & (per_row <= tc.MID_HITS)).sum() > 100
        assert (per_row > tc.MID_HITS).sum() >= 1


@pytest.fixture(scope="module")
def waves():
    return tc.wave_count_scene(seed=1)


def test_wave_scene_shape(waves):
    a, b, info = waves
    assert a[0].shape[1] == sum(tc.WAVE_ROWS) and tc.WAVE_ROWS[:5] == [tc.WAVE] * 5 and 0 < tc.WAVE_ROWS[5] < tc.WAVE
    assert np.array_equal(info["wave"], np.arange(a[0].shape[1]) // tc.WAVE), "wave w of the scene is wave w of the kernel's block"
    for w, kind in enumerate(tc.WAVE_KINDS):
        k = a[2][info["wave"] == w]
        if kind:
            assert (k == kind).all()
        else:
            assert k.min() == 3 and k.max() == 16 and len(set(k.tolist())) > 8
    for s in (a, b):
        pad = np.arange(16)[:, None] >= s[2][None, :]
        assert np.isnan(s[0][pad]).all() and np.isnan(s[1][pad]).all() and np.isfinite(s[0][~pad]).all() and np.isfinite(s[1][~pad]).all()
    # vertex counts of the bars against the largest count of the wave's rows: 4, 5 and 7 against 3, 5 and 16
    for w in range(3):
        for m in (1, 2, 3, tc.PC_SERIAL_MIN - 1, tc.PC_SERIAL_MIN, tc.PC_SERIAL_MIN + 1):
            assert b[2][(tc.WAVE + 1) * w + m] == tc.bar_vertex_count(w, m)
        assert {int(b[2][(tc.WAVE + 1) * w + m]) for m in range(tc.PC_SERIAL_MIN)} == {4, 5, 7}
    for m in (1, 3, tc.PC_SERIAL_MIN - 1, tc.PC_SERIAL_MIN + 1):   # an odd count meets both odd bar sizes across the waves
        assert {tc.bar_vertex_count(w, m) for w in range(len(tc.WAVE_ROWS))} == {5, 7}


def test_wave_scene_counts(oracle, waves):
    """bar (w, m) collides with exactly the rows of wave w whose slot is below m and with no row of another wave"""
    a, b, info = waves
    hits = poly_hits(oracle, a, b)
    want = (info["wave"][:, None] == info["col_wave"][None, :]) & (info["slot"][:, None] < info["col_m"][None, :])
    assert np.array_equal(hits, want)
    for w, rows in enumerate(tc.WAVE_ROWS):
        cols = info["col_wave"] == w
        counts = hits[info["wave"] == w][:, cols].sum(0)
        assert set(counts.tolist()) == set(range(rows + 1))
        if rows == tc.WAVE:
            assert np.array_equal(counts, info["col_m"][cols])
        lanes = np.flatnonzero(hits[info["wave"] == w][:, cols][:, tc.PC_SERIAL_MIN])   # the rows of the bar with 16: scattered lanes
        assert rows < tc.WAVE or ((lanes < 32).any() and (lanes >= 32).any() and (np.diff(lanes) > 1).any())


def phase1_undecided(a, b):
    """bool [n_a][n_b]: the pairs that phase 1 of poly_cross_mask_kernel (csrc/c2d_poly_cross.hip) leaves undecided, restated in
    numpy with the kernel's float32 operations: slots >= k repeat vertex 0; edge normals (-ey, ex); each column's sector table
    (pc_sector_dir, flipped by the sign of the first corner's cross product, the first edge with the best normalised score); the
    direction from the column's vertex mean to the row's picks the sector (pc_sector), and that one axis of the column is compared
    with strict <.  The sets hold no NaN, so the NaN rules do not come into it."""
    F = np.float32

    def padded(s):
        use = np.arange(16)[:, None] < s[2][None, :]
        x, y = np.where(use, s[0], s[0][:1]).astype(F), np.where(use, s[1], s[1][:1]).astype(F)
        k = s[2].astype(F)
        extra = F(16) - k
        return x, y, (x.sum(0, dtype=F) - extra * x[0]) / k, (y.sum(0, dtype=F) - extra * y[0]) / k

    ax, ay, cax, cay = padded(a)
    bx, by, cbx, cby = padded(b)
    nx, ny = -(np.roll(by, -1, 0) - by), np.roll(bx, -1, 0) - bx                      # [16][n_b]
    own = nx[:, None, :] * bx[None, :, :] + ny[:, None, :] * by[None, :, :]           # [edge][vertex][n_b]
    lo, hi = own.min(1), own.max(1)
    cr = (bx[1] - bx[0]) * (by[2] - by[0]) - (by[1] - by[0]) * (bx[2] - bx[0])
    flip = np.where(np.signbit(cr), F(-1), F(1))
    sct = np.arange(16)
    c, sn = np.where(sct & 8, F(0.83146961), F(0.98078528)), np.where(sct & 8, F(0.55557023), F(0.19509032))
    u, v = np.where(sct & 4, sn, c), np.where(sct & 4, c, sn)
    u, v = np.where(sct & 1, -u, u).astype(F), np.where(sct & 2, -v, v).astype(F)
    with np.errstate(invalid="ignore", divide="ignore"):
        score = (nx[None] * (u[:, None, None] * flip) + ny[None] * (v[:, None, None] * flip)) / np.sqrt(nx * nx + ny * ny)[None]
    table = np.argmax(np.where(np.isnan(score), -np.inf, score), axis=1)               # [sector][n_b]: the first best edge
    dx, dy = cax[:, None] - cbx[None, :], cay[:, None] - cby[None, :]                  # [n_a][n_b]
    fx, fy = np.abs(dx), np.abs(dy)
    swap = fy > fx
    far = np.where(swap, fx, fy) > F(0.41421356) * np.where(swap, fy, fx)
    sector = np.signbit(dx) * 1 + np.signbit(dy) * 2 + swap * 4 + far * 8
    cols = np.arange(bx.shape[1])[None, :]
    e = table[sector, cols]                                                             # [n_a][n_b]
    px, py = nx[e, cols], ny[e, cols]
    proj = px[None] * ax[:, :, None] + py[None] * ay[:, :, None]                       # [vertex][n_a][n_b]
    sep = (hi[e, cols] < proj.min(0)) | (proj.max(0) < lo[e, cols])
    return ~sep, e


def test_wave_scene_undecided_counts(waves):
    """What the scene is for: after phase 1 the undecided rows of wave w for its own column m are exactly the rows whose slot is
    below m (m of them in a full wave, so every count 0 .. 64 occurs in every full wave, with both odd bar sizes at odd counts),
    and no row is undecided for another wave's column.  The axis tried is a flat short end of the bar within a wave."""
    a, b, info = waves
    undecided, edge = phase1_undecided(a, b)
    same = info["wave"][:, None] == info["col_wave"][None, :]
    want = same & (info["slot"][:, None] < info["col_m"][None, :])
    assert np.array_equal(undecided, want), f"{int((undecided != want).sum())} pairs differ"
    for w, rows in enumerate(tc.WAVE_ROWS):
        counts = undecided[info["wave"] == w][:, info["col_wave"] == w].sum(0)
        if rows == tc.WAVE:
            assert np.array_equal(counts, np.arange(tc.WAVE + 1))
        else:
            assert set(counts.tolist()) == set(range(rows + 1))
    # the edge tried for a row to the right of the bar is the left end: the edge in front of vertex (left, y - up)
    miss = same & ~want
    left_edge = ((b[2].astype(np.int64) + 1) // 2)[None, :] * np.ones_like(edge)          # 4-gon: 2, 5-gon: 3, 7-gon: 4
    assert miss.any() and np.array_equal(edge[miss], left_edge[miss])
    ex = np.take_along_axis(b[0], (left_edge[:1] + 1) % 16, 0) - np.take_along_axis(b[0], left_edge[:1], 0)
    assert (ex == 0).all(), "the left end is not vertical"
