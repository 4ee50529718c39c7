"""GPU tests of the broad-phase rectangle pair search (c2d_sat_rect_broad_pairs): on every input its list and count must equal
c2d_sat_rect_cross_pairs' (row_base = col_base = 0), bit for bit — the cross list is itself checked against the pairwise path
by test_gpu_sat_cross.py.  Up to a few million pairs the CPU oracle is checked directly as well."""
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pair_search_harness as psh
from sat_cross_harness import rect_oracle_pairs

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_PAIRS = 3_000_000
FUZZ_SEED = 2026


def rect_set(oracle, wl, n, seed, extent):
    return oracle.rects_from_poses(*wl.random_obb_pose_planes(n, seed=seed, extent=extent)[:5])


def planes_of(d):
    return [d.row(k) for k in range(8)]


def check(eng, oracle, a, b=None, upper=False, min_pairs=0):
    """broad == cross (and == oracle below ORACLE_PAIRS) on a (self when b is None) against b; returns the list"""
    n_a = a.shape[1]
    da = eng.to_device(a)
    db = da if b is None else eng.to_device(b)
    n_b = n_a if b is None else b.shape[1]
    pa, pb = planes_of(da), planes_of(db)
    got, wc = psh.same_as(eng, psh.rect_broad(eng, pa, n_a, pb, n_b, upper), psh.rect_cross(eng, pa, n_a, pb, n_b, upper))
    if n_a * n_b <= ORACLE_PAIRS:
        assert np.array_equal(got, rect_oracle_pairs(oracle, a, a if b is None else b, upper))
    assert wc >= min_pairs, wc
    da.free()
    if b is not None:
        db.free()
    return got


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 4099, 65536])
def test_random_scenes(eng, oracle, wl, n):
    """self (upper) and two sets with n_b != n_a; sparse (about one neighbour each) and dense extents"""
    sparse = 400.0 * np.sqrt(max(n, 64) / 32768)
    dense = 8.0 if n <= 4099 else 64.0
    for k, extent in enumerate((sparse, dense)):
        a = rect_set(oracle, wl, n, 1000 + n + k, extent)
        b = rect_set(oracle, wl, n // 2 + 37, 2000 + n + k, extent)
        check(eng, oracle, a, upper=True)
        check(eng, oracle, a, b)
        check(eng, oracle, b, a, upper=True)


def test_mid_density(eng, oracle, wl):
    """about 15 (self) and 30 (two sets) hits per object: most rows go past the short path's 16 hits to the wave path"""
    n = 20_000
    a = rect_set(oracle, wl, n, 88, 50.0)
    b = rect_set(oracle, wl, 15_000, 89, 50.0)
    check(eng, oracle, a, upper=True, min_pairs=5 * n)
    check(eng, oracle, a, b, min_pairs=10 * n)


def test_million_self(eng, oracle, wl):
    """10^6 rectangles of the sparse bench scene against themselves (cross takes about a second here)"""
    n = 1_000_000
    a = rect_set(oracle, wl, n, 77, 400.0 * np.sqrt(n / 32768))
    check(eng, oracle, a, upper=True, min_pairs=n // 10)


def touching_set(scale, angle, n, seed):
    """n pairs of w x h rectangles at `angle`, the second one's centre at the touching distance along the frame's x axis moved by
    -4 .. 4 ulps; the pairs sit in a row 4 * scale apart"""
    rng = np.random.default_rng(seed)
    F = np.float32
    w = (rng.uniform(0.5, 1.0, n) * scale).astype(F)
    h = (rng.uniform(0.5, 1.0, n) * scale).astype(F)
    c, s = np.cos(angle), np.sin(angle)
    base = np.arange(n) * 4.0 * scale
    d = (w.astype(np.float64) * (1 + rng.integers(-4, 5, n) * 2.0 ** -23))
    pose_a = [base.astype(F), np.zeros(n, F), w, h, np.full(n, angle, F)]
    pose_b = [(base + d * c).astype(F), (d * s).astype(F), w, h, np.full(n, angle, F)]
    return pose_a, pose_b


@pytest.mark.parametrize("scale", [1e-20, 1e-6, 1.0, 1e6, 1e15])
def test_touching_pairs(eng, oracle, wl, scale):
    for angle in (0.0, np.pi / 4, np.pi / 2, 1e-6):
        pa, pb = touching_set(scale, angle, 600, int(angle * 1e6) + 5)
        a, b = oracle.rects_from_poses(*pa), oracle.rects_from_poses(*pb)
        both = np.concatenate([a, b], axis=1)
        check(eng, oracle, both, upper=True)
        check(eng, oracle, a, b)
    pp = wl.touching_pose_pairs(1500, seed=43, scale=scale)
    check(eng, oracle, oracle.rects_from_poses(*pp[:5]), oracle.rects_from_poses(*pp[5:]))


def odd_shapes(n, seed, extent=6.0):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-extent, extent, (2, n))
    th = rng.uniform(0, 2 * np.pi, n)
    u = np.stack([np.cos(th), np.sin(th)])
    v = np.stack([-u[1], u[0]])
    w, h = rng.uniform(0.1, 2, n), rng.uniform(0.1, 2, n)
    ang = np.exp(rng.uniform(np.log(1e-4), np.log(0.5), n))
    e1 = np.stack([np.cos(th + ang), np.sin(th + ang)])
    kind = rng.integers(0, 8, n)
    shapes = [
        [c - w * u - h * v, c + w * u - h * v, c + w * u + h * v, c - w * u + h * v],             # rectangle
        [c - w * u, c + w * u, c + w * u + h * e1, c - w * u + h * e1],                          # sheared, acute at vertex 0
        [c - w * u, c + w * u, c + w * u - 2 * w * e1, c + h * v],                               # kite, acute at vertex 1
        [c - w * u - h * v, c + w * u + h * v, c + w * u - h * v, c - w * u + h * v],             # bow-tie
        [c - w * u + h * v, c + w * u + h * v, c + w * u - h * v, c - w * u - h * v],             # reversed winding
        [c - w * u, c, c + w * u, c + 2 * w * u],                                                  # collinear
        [c, c, c, c],                                                                              # zero area, one point
        [c - w * u, c - w * u, c + h * v, c + h * v],                                              # repeated vertices
    ]
    out = np.empty((8, n), np.float64)
    for k in range(8):
        sel = kind == k
        for q in range(4):
            out[2 * q:2 * q + 2, sel] = shapes[k][q][:, sel]
    return out.astype(np.float32)


def test_odd_shapes(eng, oracle):
    a, b = odd_shapes(1700, 1), odd_shapes(1300, 2)
    check(eng, oracle, a, upper=True, min_pairs=1000)
    check(eng, oracle, a, b, min_pairs=1000)
    big = odd_shapes(40_000, 3, extent=300.0)
    check(eng, oracle, big, upper=True)


def test_non_finite_and_extreme(eng, oracle, wl):
    n = 1500
    a, b = rect_set(oracle, wl, n, 61, 20.0), rect_set(oracle, wl, n - 300, 62, 20.0)
    for k in range(8):                          # NaN, +inf, -inf in each plane
        a[k, 10 * k:10 * k + 3] = [np.nan, np.inf, -np.inf]
        b[k, 10 * k + 5:10 * k + 8] = [np.inf, np.nan, -np.inf]
    a = wl.inject_non_finite(a, seed=63, frac=0.02)
    big = np.float32(2.0 ** 61)
    for j, val in enumerate((big, np.nextafter(big, np.float32(0)), np.nextafter(big, np.float32(np.inf)), np.float32(2.0 ** 60))):
        b[:, 900 + 4 * j:904 + 4 * j] = b[:, 900 + 4 * j:904 + 4 * j] * np.float32(1e-3) + val   # near +-2^61, 2^60
        a[:, 300 + 4 * j:304 + 4 * j] = -val + a[:, 300 + 4 * j:304 + 4 * j] * np.float32(1e-3)
    tiny = rect_set(oracle, wl, 40, 64, 1.0) * np.float32(1e-40)      # subnormal sizes and coordinates
    a[:, 1400:1440] = tiny
    b[:, 1100:1140] = tiny
    check(eng, oracle, a, b)
    check(eng, oracle, a, upper=True)
    check(eng, oracle, b, a, upper=True)


def test_outliers(eng, oracle, wl):
    n = 100_000
    a = rect_set(oracle, wl, n, 71, 400.0 * np.sqrt(n / 32768))
    far = a.copy()
    far[:, 777] += np.float32(1e30)             # one rectangle at 1e30
    check(eng, oracle, far, upper=True, min_pairs=n // 10)
    cover = a.copy()
    cover[:, 4242] = [-1e4, -1e4, 1e4, -1e4, 1e4, 1e4, -1e4, 1e4]     # one rectangle over the whole scene
    got = check(eng, oracle, cover, upper=True, min_pairs=n)
    assert ((got[:, 0] == 4242) | (got[:, 1] == 4242)).sum() == n - 1


def test_identical_rectangles(eng, oracle, wl):
    """N identical rectangles: N^2 hits (every row over the short path's limit)"""
    n = 2000
    a = np.repeat(rect_set(oracle, wl, 1, 81, 1.0), n, axis=1)
    got = check(eng, oracle, a, upper=True)
    assert len(got) == n * (n - 1) // 2
    assert len(check(eng, oracle, a, a[:, :1500])) == n * 1500


def test_capacity_and_determinism(eng, oracle, wl):
    n = 20_000
    a = rect_set(oracle, wl, n, 91, 80.0)
    b = rect_set(oracle, wl, 12_345, 92, 80.0)
    da, db = eng.to_device(a), eng.to_device(b)
    pa, pb = planes_of(da), planes_of(db)
    for upper in (False, True):
        full, total = psh.run(eng, psh.rect_broad(eng, pa, n, pb, 12_345, upper))
        assert total > 10_000
        d_cnt = eng.zeros(1, np.uint64)             # capacity 0, no buffer: count only
        eng.sat_rect_broad_pairs(pa, n, pb, 12_345, None, 0, d_cnt, upper=upper)
        assert int(d_cnt.get()[0]) == total
        eng.sat_rect_broad_pairs(pa, n, pb, 12_345, None, 0, d_cnt, upper=upper)
        assert int(d_cnt.get()[0]) == 2 * total, "d_count is incremented, not set"
        d_cnt.free()
        for cap in (1, total // 3 + 1, total - 1):
            p, c = psh.run(eng, psh.rect_broad(eng, pa, n, pb, 12_345, upper), capacity=cap)
            assert c == total and np.array_equal(p, full[:cap])
        p1, _ = psh.run(eng, psh.rect_broad(eng, pa, n, pb, 12_345, upper), capacity=total // 2)
        p2, _ = psh.run(eng, psh.rect_broad(eng, pa, n, pb, 12_345, upper), capacity=total // 2)
        assert p1.tobytes() == p2.tobytes()
    got = eng.rect_broad_pairs_host(a, b)
    assert np.array_equal(got, psh.run(eng, psh.rect_cross(eng, pa, n, pb, 12_345))[0])
    got = eng.rect_broad_pairs_host(a, upper=True)
    assert np.array_equal(got, psh.run(eng, psh.rect_cross(eng, pa, n, pa, n, True))[0])
    da.free()
    db.free()


def test_argument_errors(eng, pkg, oracle, wl):
    a = rect_set(oracle, wl, 100, 5, 3.0)
    da = eng.to_device(a)
    pa = planes_of(da)
    d_pairs = eng.zeros((16, 2), np.uint32)
    d_cnt = eng.zeros(1, np.uint64)
    eng.sat_rect_broad_pairs(pa, 0, pa, 100, None, 0, None)      # n_a == 0: a no-op
    eng.sat_rect_broad_pairs(pa, 100, pa, 0, None, 0, None)
    bad = [
        lambda: eng.sat_rect_broad_pairs(pa, 100, pa, 100, d_pairs, 16, None),                    # no count
        lambda: eng.sat_rect_broad_pairs(pa, 100, pa, 100, None, 16, d_cnt),                      # no buffer
        lambda: eng.sat_rect_broad_pairs(pa[:7] + [0], 100, pa, 100, d_pairs, 16, d_cnt),         # a NULL plane
        lambda: eng.sat_rect_broad_pairs(pa, (1 << 32) + 1, pa, 100, d_pairs, 16, d_cnt),         # index past u32
    ]
    for k, call in enumerate(bad):
        with pytest.raises(pkg.C2DError) as e:
            call()
        assert e.value.status == -1, k
    import ctypes as C
    planes = (C.c_void_p * 8)(*pa)
    assert eng.lib.c2d_sat_rect_broad_pairs(eng.h, planes, 100, planes, 100, 2, d_pairs.ptr, 16, d_cnt.ptr, None) == -1
    eng.synchronize()
    assert int(d_cnt.get()[0]) == 0
    for x in (da, d_pairs, d_cnt):
        x.free()


def test_graph_capture():
    """replay after a warm-up equals the direct call, two-set and self; a capture that would have to grow the scratch is refused
    (tests/pair_search_graph_check.py, its own process: torch has to be imported before libc2d.so)"""
    out = subprocess.run([sys.executable, os.path.join(HERE, "pair_search_graph_check.py"), "rect_broad"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-1500:]
    assert "broad graph ok" in out.stdout


def test_fuzzer_configurations_at_a_fixed_seed(eng, oracle):
    """tests/tools/broad_fuzz.py at a fixed seed, each configuration from its own stream (seed, index): sixteen configurations, chosen so
    that they hold what the tool is for — a pile whose rows pass 512 hits, wild objects, self mode"""
    spec = importlib.util.spec_from_file_location("broad_fuzz", os.path.join(HERE, "tools", "broad_fuzz.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    seen, compared = [], 0
    for i in range(16):
        ok, (desc, n) = fz.one(eng, np.random.default_rng([FUZZ_SEED, i]), i, None, oracle)
        assert ok, desc
        seen.append(desc)
        compared += n
    assert any(int(m) > 512 for d in seen for m in re.findall(r"pile (\d+)", d)), seen
    assert any(re.search(r"wild [1-9]", d) for d in seen) and any("self mode" in d for d in seen), seen
    assert compared > 1000
    eng.check_async()
