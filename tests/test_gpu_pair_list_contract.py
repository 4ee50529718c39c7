"""GPU tests of what every list-driven query promises of its list (csrc/c2d_pair_list.hpp: `listed_pairs`, the host checks), once
for each entry of pair_list_harness.QUERIES: the device count bounds the work, a bad entry reads nothing and is reported once, a bad
argument is refused before anything is written, and a captured call follows the count on the device.  The values themselves are
each query's own file's: test_gpu_contacts.py, test_gpu_manifolds.py, test_gpu_distances.py, test_gpu_sweeps.py.  A query whose sets
carry more than vertices (the sweeps: a motion per set, pair_list_harness.Extras) has it on both sets in every test here."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import contact_cases as cases  # noqa: E402
import manifold_ref  # noqa: E402
import pair_list_harness as h  # noqa: E402

pytestmark = pytest.mark.gpu
each_query = pytest.mark.parametrize("q", h.QUERIES, ids=repr)


@each_query
def test_device_count_bounds_the_work(eng, wl, q):
    """n_pairs = capacity with the count on the device: smaller (only that many records are written), equal, larger (clamped to
    n_pairs), and no count at all.  run() checks the guard bands and every record of every output beyond the bound.
    Counts 0, 1, 63, 64, 137, 299, 300, 301 and 2^64 - 1 with capacity 300, and count 300 with capacity 1000, were in all four
    per-query copies of this test; 2^40 and None in the contacts, distances and sweeps copies."""
    a, b, pairs, want = h.dense(wl, q)
    ua, ub, x = h.Uploaded(eng, a), h.Uploaded(eng, b), h.Extras(eng, h.dense_extras(q))
    sel = np.arange(len(pairs))[q.count_cut][:300]
    call = q.poly_call(eng, ua.set, ub.set, **x.kw)
    for n_dev in (0, 1, 63, 64, 137, 299, 300, 301, 1 << 40, (1 << 64) - 1, None):
        got = q.run(eng, call, pairs[sel], capacity=300, n_dev=n_dev)
        bound = 300 if n_dev is None else min(300, n_dev)
        q.assert_same(q.cut(got, slice(bound)), q.cut(want, sel[:bound]), f"device count {n_dev}")
    # a capacity above the list, as a caller passes it: the count says where the list ends
    got = q.run(eng, call, pairs[sel], capacity=1000, n_dev=300)
    q.assert_same(q.cut(got, slice(300)), q.cut(want, sel), "capacity 1000, count 300")
    eng.check_async()
    for z in (ua, ub, x):
        z.free()


@each_query
def test_bad_pairs_read_nothing_and_are_reported_once(eng, wl, q):
    """Indices equal to n, 0xFFFFFFFF and below the base, in either column, and polygons with a vertex count of 0 and 17: those
    entries carry BAD_PAIR (and the empty manifold), every other entry is correct, and the error is reported once by the next
    synchronise.  The vertex planes and the motion planes end where their allocations end; the guard (c2d_pair_list.hpp: `ranged`,
    `valid`) lets no such index reach a load.  The nine bad entries at positions 0, 1, 63, 64, 65, 200, 255, 256 and the last, the
    two bad counts and the clean call afterwards were in all four per-query copies of this test; the rectangle list in the contacts,
    distances and sweeps copies (the queries that have the call; the sweeps with A moving and B without planes), the empty manifolds
    in the manifolds copy, the clean call's flags in contacts, distances and sweeps."""
    n_a, n_b, rb, cb = 50, 64, 1000, 5
    a = wl.random_convex_polygon_set(n_a, seed=8001, extent=2.5)
    b = wl.random_convex_polygon_set(n_b, seed=8002, kmax=8, extent=2.5, rows=8)
    kb = b[2].copy()
    kb[[3, 40]] = [0, 17]
    b = (b[0], b[1], kb)
    x = q.extras(9801, n_a, n_b, 2.5)
    d = [eng.to_device(v) for v in (*a, *b)]        # exact allocations: nothing behind the last plane row
    dx = h.Extras(eng, x, apart=True)               # (of the motion planes as well)
    sa, sb = eng.poly_set(d[0], d[1], d[2], n_a, 16), eng.poly_set(d[3], d[4], d[5], n_b, 8)
    good = cases.all_pairs(n_a, n_b)[::7].astype(np.int64) + (rb, cb)
    bad = np.array([[rb + n_a, cb], [0xFFFFFFFF, cb + 1], [rb - 1, cb + 2], [rb + 1, cb + n_b], [rb + 2, 0xFFFFFFFF], [rb + 3, cb - 1],
                    [0, 0], [0xFFFFFFFF, 0xFFFFFFFF], [rb + n_a + 70, cb + 3]], np.int64)
    listed = good.copy()
    at = np.array([0, 1, 63, 64, 65, 200, 255, 256, len(good) - 1])
    listed[at] = bad
    want = q.poly_ref(a, b, listed[:, 0] - rb, listed[:, 1] - cb, *x)
    is_bad = h.outputs(want)[0]["flags"] == q.bad_pair
    assert is_bad[at].all() and is_bad.sum() > len(at) and (~is_bad).sum() > 300          # (the bad counts as well)
    eng.check_async()
    call = q.poly_call(eng, sa, sb, row_base=rb, col_base=cb, **dx.kw)
    got = q.run(eng, call, listed.astype(np.uint32), expect_error=True)
    q.assert_same(got, want, "list with bad pairs")
    if q is h.MANIFOLDS:
        none = manifold_ref.empty(int(is_bad.sum())).tobytes()
        assert want[1][is_bad].tobytes() == none and got[1][is_bad].tobytes() == none
    if q.rect:      # the same with rectangles (no absent objects there: only the indices)
        ra = np.ascontiguousarray(np.concatenate([a[0][:4], a[1][:4]])[[0, 4, 1, 5, 2, 6, 3, 7]])
        da = h.RectsOnDevice(eng, ra)
        only_a = x[:1] + (None,) * len(x[1:])       # extras on A alone: B goes without
        want = q.rect_ref(ra, ra, listed[:, 0] - rb, listed[:, 1] - cb, *only_a)
        kw = {k: v for k, v in dx.kw.items() if k.startswith("a_")}
        got = q.run(eng, q.rect_call(eng, da, da, row_base=rb, col_base=cb, **kw), listed.astype(np.uint32), expect_error=True)
        q.assert_same(got, want, "rectangle list with bad pairs")
        da.free()
    # a clean call afterwards reports nothing
    sound = good[(kb[good[:, 1] - cb] >= 1) & (kb[good[:, 1] - cb] <= 8)][:10]
    clean = q.run(eng, call, sound.astype(np.uint32))
    assert (h.outputs(clean)[0]["flags"] & q.bad_pair == 0).all()
    eng.check_async()
    for z in d + [dx]:
        z.free()


@each_query
def test_argument_errors(eng, pkg, wl, q):
    """Every refused form returns -1 and writes nothing.  All four per-query copies of this test had the polygon forms (a missing
    and a misaligned output once per output) except n_pairs beyond 2^62, which was the distances and sweeps copies'; the contacts,
    distances and sweeps copies had the rectangle forms.  (What a query refuses of its extras is its own file's.)"""
    a = wl.random_convex_polygon_set(100, seed=5, extent=3.0)
    ua = h.Uploaded(eng, a)
    S = ua.set
    d_pairs = eng.zeros((16, 2), np.uint32)
    d_outs = [eng.zeros(16, dt) for dt in q.dts]
    d_n = eng.zeros(1, np.uint64)
    x = h.Extras(eng, q.extras(5, 100, 100, 1.0))
    mk = lambda **kw: eng.poly_set(kw.get("vx", ua.px), kw.get("vy", ua.py), ua.dk, kw.get("n", 100), kw.get("rows", 16), kw.get("stride", 0))  # noqa: E731
    planes = [ua.px] * 8
    raw = getattr(eng.lib, "c2d_" + q.poly)
    ptrs = [x.ptr for x in d_outs]
    assert raw(eng.h, None, C.byref(S), *x.raw, d_pairs.ptr, 16, None, 0, 0, *ptrs, None) == -1
    assert raw(eng.h, C.byref(S), None, *x.raw, d_pairs.ptr, 16, None, 0, 0, *ptrs, None) == -1
    poly = functools.partial(getattr(eng, q.poly), **x.kw)
    without = lambda k, v: [v if o == k else x for o, x in enumerate(d_outs)]  # noqa: E731   (the outputs, output k replaced by v)
    bad = [
        lambda: poly(mk(vx=0), S, d_pairs, 16, *d_outs),                           # a NULL plane
        lambda: poly(S, mk(vy=0), d_pairs, 16, *d_outs),
        lambda: poly(mk(rows=0), S, d_pairs, 16, *d_outs),                         # rows 0 or 17
        lambda: poly(S, mk(rows=17), d_pairs, 16, *d_outs),
        lambda: poly(mk(stride=99), S, d_pairs, 16, *d_outs),                      # stride < n
        lambda: poly(mk(vx=ua.px + 2), S, d_pairs, 16, *d_outs),                   # a misaligned plane
        lambda: poly(S, S, None, 16, *d_outs),                                     # no list
        lambda: poly(S, S, d_pairs.ptr + 2, 15, *d_outs),                          # list not 4-byte aligned
        lambda: poly(S, S, d_pairs, 16, *d_outs, n_pairs_dev=d_n.ptr + 4),         # count not 8-byte aligned
        lambda: poly(S, S, d_pairs, 1 << 62 | 1, *d_outs),                         # n_pairs beyond 2^62
        lambda: poly(S, S, d_pairs, 16, *d_outs, row_base=1 << 62),                # bases beyond 2^62
        lambda: poly(S, S, d_pairs, 16, *d_outs, col_base=1 << 62),
    ]
    for k in range(len(d_outs)):
        bad += [lambda k=k: poly(S, S, d_pairs, 16, *without(k, None)),                    # any output missing
                lambda k=k: poly(S, S, d_pairs, 15, *without(k, d_outs[k].ptr + 8))]       # any output not 16-byte aligned
    if q.rect:
        rect = functools.partial(getattr(eng, q.rect), **x.kw)
        bad += [
            lambda: rect(planes[:7] + [0], 100, planes, 100, d_pairs, 16, *d_outs),
            lambda: rect(planes, 100, planes[:7] + [0], 100, d_pairs, 16, *d_outs),
            lambda: rect(planes, 100, planes, 100, None, 16, *d_outs),
            lambda: rect(planes, 100, planes, 100, d_pairs, 16, None),
            lambda: rect(planes, 100, planes, 100, d_pairs, 15, d_outs[0].ptr + 4),
            lambda: rect(planes, 100, planes, 100, d_pairs, 16, *d_outs, col_base=1 << 62),
        ]
    for n, call in enumerate(bad):
        with pytest.raises(pkg.C2DError) as e:
            call()
        assert e.value.status == -1, n
    poly(S, S, None, 0, *[None] * len(d_outs))                      # n_pairs == 0: a no-op
    if q.rect:
        rect(planes, 100, planes, 100, None, 0, None)
    eng.synchronize()
    assert all((x.get().view(np.uint8) == 0).all() for x in d_outs), "a refused call wrote something"
    for z in [d_pairs, d_n, ua, x] + d_outs:
        z.free()


@each_query
def test_graph_capture_follows_the_device_count(q):
    """One capture of the query's polygon call with d_n_pairs, replayed with different counts written to the device in between
    (tests/pair_list_graph_check.py, its own process: torch has to be imported before libc2d.so)."""
    out = subprocess.run([sys.executable, os.path.join(HERE, "pair_list_graph_check.py"), q.name], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert f"{q.name} graph ok" in out.stdout
