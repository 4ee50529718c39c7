"""CPU tests of tests/clearance_ref.py, the numpy restatement of the clearance contract of include/c2d.h (c2d_poly_set_clearances): the
hand cases of tests/clearance_cases.py with the values the contract gives them, and the sparse clearance scene with the shares of
every kind of winner and a float64 brute force.  The GPU tests compare the kernels with this reference (tests/test_gpu_clearances.py)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import clearance_cases as cases  # noqa: E402
import clearance_ref as ref  # noqa: E402
import distance_ref  # noqa: E402


@pytest.mark.parametrize("name", sorted(cases.hand_cases()))
def test_hand_case(name):
    a, b, kw, expect = cases.hand_cases()[name]
    got = ref.clearances(a, b, **kw)
    assert len(got) == a[0].shape[1] and (got["reserved0"] == 0).all()
    for f, v in expect.items():
        assert np.array_equal(got[f], np.array(v, got[f].dtype)), (f, got[f], v)
    assert ref.same(got, got).all()


def test_the_reduction_is_the_distance_contracts():
    """every field of a winner's record is the same-named field of distance_ref's record of the pair (i, winner), and no considered
    polygon has a smaller key; the bases shift `poly` and the self pair only"""
    a, b, _, _ = cases.hand_cases()["nearest_to_the_right"]
    got = ref.clearances(a, b, row_base=5, col_base=100)
    assert got["poly"][0] == 101
    d = distance_ref.poly_distances(a, b, [0], [1])
    for f in ref.COPIED:
        assert got[f][0] == d[f][0]
    assert ref.CLEARANCE_DT.itemsize == 32 and [ref.CLEARANCE_DT.fields[f][1] for f in ref.CLEARANCE_DT.names] == [0, 4, 8, 12, 16, 20, 24, 26, 28, 29, 30]
    # +0 and -0 are equal in the floats; everything else is compared exactly
    x, y = got.copy(), got.copy()
    y["ax"] = -0.0 * np.ones(1, np.float32)
    x["ax"] = 0.0
    assert ref.same(x, y).all()
    y["poly"] += 1
    assert not ref.same(x, y).any()


# ---- the sparse clearance scene -----------------------------------------------------------------------------------------------------

# The reference's own float32-versus-float64 deviation on the scene's separated winners (measured by this file, which prints what it
# sees): the worst |dist - min_j dist64(i, j)| is 1.76e-6, with coordinates up to 65.5 (ulp 7.6e-6).  The brute force allows 4 x that.
DEV_ABS = 1.76e-6


def _verts64(s):
    """-> x, y f64 [n][16] with the slots at and beyond k repeating vertex 0"""
    vx, vy, k = s
    x, y = vx.T.astype(np.float64), vy.T.astype(np.float64)
    pad = np.arange(x.shape[1])[None, :] >= k.astype(np.int64)[:, None]
    return np.where(pad, x[:, :1], x), np.where(pad, y[:, :1], y)


def _distance64(xa, ya, xb, yb):
    """float64 brute force for every pair [n_a][n_b]: the smallest vertex-to-segment distance, both ways"""
    best = np.full((len(xa), len(xb)), np.inf)
    for (px, py), (qx, qy), flip in (((xa, ya), (xb, yb), False), ((xb, yb), (xa, ya), True)):
        x1, y1 = np.roll(px, -1, axis=1), np.roll(py, -1, axis=1)
        ex, ey = x1 - px, y1 - py
        len2 = np.where(ex * ex + ey * ey > 0, ex * ex + ey * ey, 1.0)
        for v in range(qx.shape[1]):
            ux, uy = qx[None, :, v, None] - px[:, None, :], qy[None, :, v, None] - py[:, None, :]          # [edge polygon][vertex polygon][edge]
            t = np.clip((ux * ex[:, None, :] + uy * ey[:, None, :]) / len2[:, None, :], 0.0, 1.0)
            d = np.hypot(ux - t * ex[:, None, :], uy - t * ey[:, None, :]).min(axis=2)
            best = np.minimum(best, d.T if flip else d)
    return best


@pytest.fixture(scope="module")
def scene(wl):
    a, b = cases.scene(wl)
    D = ref.pair_records(a, b)
    return a, b, D, ref.reduce(D, ref.bad_counts(a), ref.bad_counts(b))


def test_scene_covers_every_kind_of_winner(scene):
    """The shares of the committed seeds (200 queries against 500 polygons: 41.5 % of the queries hit something; of the separated
    winners side 1 27 %, regions 0 / 1 / 2 6 % / 28 % / 66 %; every k of 3..16 among the winners), each asserted at half its share"""
    a, b, D, c = scene
    assert len(c) == 200 and D.shape == (200, 500)
    sep = c["hit"] == 0
    assert (c["flags"] & (distance_ref.NO_CANDIDATE | distance_ref.BAD_PAIR | ref.NONE_FLAG) == 0).all() and np.isfinite(c["dist"]).all()
    assert (c["dist"][sep] > 0).all() and (c["dist"][~sep] == 0).all()
    side1 = (c["flags"][sep] & distance_ref.EDGE_ON_B) != 0
    interior = (c["flags"][sep] & distance_ref.INTERIOR) != 0
    win = c["poly"][sep].astype(np.int64)
    rows = np.flatnonzero(sep)
    # regions 0 and 1 are told apart by which end of the winning edge the closest point is
    ex = np.where(side1, b[0][c["edge"][sep], win], a[0][c["edge"][sep], rows])
    ey = np.where(side1, b[1][c["edge"][sep], win], a[1][c["edge"][sep], rows])
    cx, cy = np.where(side1, c["bx"][sep], c["ax"][sep]), np.where(side1, c["by"][sep], c["ay"][sep])
    region0 = ~interior & (cx == ex) & (cy == ey)
    shares = {"hit": 1 - sep.mean(), "separated": sep.mean(), "side 1": side1.mean(), "region 0": region0.mean(), "region 1": (~interior & ~region0).mean(),
              "region 2": interior.mean()}
    print("shares:", {k: round(float(v), 4) for k, v in shares.items()}, "k of the winners:", np.bincount(b[2][c["poly"]], minlength=17)[3:])
    for name, share in SHARES:
        assert shares[name] >= share / 2, (name, shares[name])
    assert set(np.unique(b[2][c["poly"]])) == set(range(3, 17))
    # the winner's key is the smallest of its row, and a hit winner is the first hitting polygon
    key = (np.ascontiguousarray(D["dist"]).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(500, dtype=np.uint64)[None, :]
    assert np.array_equal(key.argmin(axis=1), c["poly"])
    assert np.array_equal(c["poly"][~sep], (D["hit"] == 1).argmax(axis=1)[~sep])


SHARES = (("hit", 0.415), ("separated", 0.585), ("side 1", 0.27), ("region 0", 0.06), ("region 1", 0.28), ("region 2", 0.66))


def test_scene_against_a_float64_brute_force(scene):
    a, b, D, c = scene
    sep = c["hit"] == 0
    xa, ya = _verts64(a)
    xb, yb = _verts64(b)
    d64 = _distance64(xa[sep], ya[sep], xb, yb)
    err = np.abs(c["dist"][sep] - d64.min(axis=1))
    print("float32 reference against float64 brute force over", int(sep.sum()), "separated queries: worst absolute", float(err.max()),
          "; largest |coordinate|", float(max(np.abs(a[0]).max(), np.abs(b[0]).max())))
    assert (err <= 4 * DEV_ABS).all()
    # the float64 winner is the reference's, or as near as the deviation allows
    assert (d64[np.arange(sep.sum()), c["poly"][sep]] <= d64.min(axis=1) + 8 * DEV_ABS).all()
