#!/usr/bin/env python3
"""Differential fuzz of c2d_sat_rect_cross_mask / c2d_sat_rect_cross_pairs against the CPU oracle on the materialised pairs (the
reference() of tests/test_gpu_sat_cross.py, never another GPU path): set sizes on both sides of the 64-bit mask word and of the
256 x 256 tile, rectangles from random poses at densities from half a percent to more than half colliding, arbitrary quads, outliers
(scaled by 1e2 .. 1e6, shifted by 1e30, 2^60, -2^61, 1e-30), NaN / inf / 3e38 in single coordinates, duplicated rectangles, A and B
the same memory; planes shifted by 0 .. 3 floats, ld_words beyond the row's words, the upper triangle with row and column bases
drawn independently (a shifted diagonal), the mask call and the list call with no buffer, the exact capacity, a capacity below the
total and one above it.  compare() is the judge (a pure function on host arrays, tests/test_fuzz_compare_cpu.py): every mask bit,
zero tail bits, untouched padding words and guard rows, count == popcount, the list == argwhere(mask) + bases up to the capacity
with untouched guard entries around it, the total whatever the capacity, error reports.  tests/tools/poly_cross_fuzz.py shares
draw_call(), run_call() and compare().  Prints its seed; a mismatch names its configuration.
usage: cross_fuzz.py [configs] [seed]     (no seed: the commit's, tests/tools/fuzz_seed.py)"""
import importlib
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
wl = importlib.import_module("c2d_amd.workloads")
F = np.float32
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)
GUARD = 4                      # guard entries in front of and behind the list
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 511, 513]
LAST = {}                      # hits / misses of the last configuration, for the exploring leg's "not vacuous" check


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fuzz_seed = _tool("fuzz_seed")


# ---- the judge ---------------------------------------------------------------------------------------------------------------------
def expected(ref, upper, row_base, col_base):
    """bool [n_a][n_b] of the tested pairs: with C2D_CROSS_UPPER only those with (col_base + j) > (row_base + i) (include/c2d.h)"""
    if not upper:
        return ref.copy()
    n_a, n_b = ref.shape
    return ref & ((np.arange(n_b, dtype=np.int64)[None, :] + col_base) > (np.arange(n_a, dtype=np.int64)[:, None] + row_base))


def compare(mask, count, pairs, total, reported, clean, want, n_b, row_base=0, col_base=0, capacity=None, expect_report=False):
    """The judgement of one mask call and one list call -> the list of complaints (empty: all is well).
    mask u64 [1 + n_a + 1][ld_words], a guard row on each side, as the mask call left a buffer of SENTINEL words; count: what it
    added to a zeroed counter; pairs u32 [GUARD + capacity + GUARD][2] as the list call left a buffer of SENTINEL bytes, or None
    for the count-only call (capacity None); total: what the list call added to a zeroed counter; reported: how many of the two
    synchronisations raised; clean: check_async afterwards was; want bool [n_a][n_b]: expected() of the reference; expect_report:
    True: each call reports once, False: neither does, None: either (the header promises the report for the pairs a polygon with a
    bad count is in; under C2D_CROSS_UPPER such a polygon can be in no tested pair, and then the header says nothing)."""
    out = []
    n_a, words, ld = want.shape[0], (n_b + 63) // 64, mask.shape[1]
    if mask.shape[0] != n_a + 2 or ld < words:
        return [f"mask buffer of shape {mask.shape} for {n_a} rows of {words} words"]
    if not ((mask[0] == SENTINEL).all() and (mask[-1] == SENTINEL).all()):
        out.append("a guard row of the mask was written")
    body = mask[1:-1]
    if not (body[:, words:] == SENTINEL).all():
        out.append(f"{int((body[:, words:] != SENTINEL).sum())} padding words beyond ceil(n_b / 64) were written")
    bits = np.unpackbits(np.ascontiguousarray(body[:, :words]).view(np.uint8), bitorder="little", axis=-1).reshape(n_a, words * 64).astype(bool)
    if bits[:, n_b:].any():
        out.append(f"{int(bits[:, n_b:].sum())} tail bits j >= n_b are set")
    wrong = bits[:, :n_b] != want
    if wrong.any():
        i, j = np.argwhere(wrong)[0]
        out.append(f"{int(wrong.sum())} mask bits differ from the reference; first at ({i}, {j}): got {bool(bits[i, j])}")
    hits = int(want.sum())
    if count != hits:
        out.append(f"the mask call counted {count}, the reference has {hits}")
    if total != hits:
        out.append(f"the list call's total is {total}, the reference has {hits}")
    if pairs is not None:
        cap = 0 if capacity is None else capacity
        if pairs.shape != (cap + 2 * GUARD, 2):
            return out + [f"list buffer of shape {pairs.shape} for a capacity of {cap}"]
        flat = pairs.view(np.uint64).reshape(-1)
        if not (flat[:GUARD] == SENTINEL).all():
            out.append("written in front of the list")
        listed = (np.argwhere(want) + (row_base, col_base)).astype(np.uint32)
        n = min(cap, len(listed))
        got = pairs[GUARD: GUARD + n]
        if not np.array_equal(got, listed[:n]):
            bad = np.flatnonzero((got != listed[:n]).any(1))
            out.append(f"{len(bad)} of {n} list entries differ; first at {int(bad[0])}: got {got[bad[0]].tolist()}, want {listed[bad[0]].tolist()}")
        if not (flat[GUARD + n:] == SENTINEL).all():
            out.append("written behind the list (past the capacity or past the total)")
    if expect_report is not None and reported != (2 if expect_report else 0):
        out.append(f"{reported} of the two calls reported an error, {'both' if expect_report else 'none'} should")
    if not clean:
        out.append("check_async still reports an error after both synchronisations")
    return out


# ---- the call shape, shared with the polygon form ------------------------------------------------------------------------------------
def draw_sizes(rng, limit):
    sizes = SIZES + [int(rng.integers(1, 1501))]
    n_a, n_b = int(rng.choice(sizes)), int(rng.choice(sizes))
    while n_a * n_b > limit:                       # cut the larger one down
        if n_a >= n_b:
            n_a = limit // n_b
        else:
            n_b = limit // n_a
    return n_a, n_b


def draw_call(rng, n_a, n_b):
    """ld_words, upper, bases (independent: the diagonal moves), which capacity the list call gets"""
    return dict(ld=(n_b + 63) // 64 + int(rng.choice([0, 1, 3])), upper=bool(rng.random() < 0.5),
                rb=int(rng.choice([0, 7, 1 << 20, (1 << 32) - n_a])), cb=int(rng.choice([0, 7, 1 << 20, (1 << 32) - n_b])),
                cap_kind=str(rng.choice(["none", "total", "third", "more"])))


def capacity_of(kind, total):
    return {"none": None, "total": total, "third": total // 3 + 1, "more": total + 5}[kind]


def describe_call(call, n_b, total, cap):
    words = (n_b + 63) // 64
    ld = f"ld_words {call['ld']} {'>' if call['ld'] > words else '='} words {words}"
    bases = f"bases {call['rb']}, {call['cb']} ({'equal' if call['rb'] == call['cb'] else 'unequal'})"
    if cap is None:
        lst = "count-only list call (NULL, capacity 0)"
    else:
        lst = f"list capacity {cap} {'below' if cap < total else 'at' if cap == total else 'above'} the total {total}"
    return f"{ld}, upper {call['upper']}, {bases}, {lst}"


def run_call(eng, mask_fn, pairs_fn, n_a, call, cap):
    """mask_fn(d_mask_ptr, ld, d_cnt) and pairs_fn(d_pairs_ptr_or_None, capacity, d_cnt) queue the two calls with this
    configuration's sets, bases and flag -> (mask with its guard rows, count, list with its guard entries or None, total, reports,
    clean)"""
    ld = call["ld"]
    d_mask = eng.empty((n_a + 2, ld), np.uint64)
    eng.memset(d_mask, 0xA5, d_mask.nbytes)
    d_cnt = eng.zeros(2, np.uint64)
    d_pairs = None
    if cap is not None:
        d_pairs = eng.empty((cap + 2 * GUARD, 2), np.uint32)
        eng.memset(d_pairs, 0xA5, d_pairs.nbytes)
    reports = 0
    try:
        mask_fn(d_mask.ptr + 8 * ld, ld, d_cnt.ptr)
        try:
            eng.synchronize()
        except pkg.C2DError:
            reports += 1
        pairs_fn(None if d_pairs is None else d_pairs.ptr + 8 * GUARD, 0 if cap is None else cap, d_cnt.ptr + 8)
        try:
            eng.synchronize()
        except pkg.C2DError:
            reports += 1
        try:
            eng.check_async()
            clean = True
        except pkg.C2DError:
            clean = False
        count, total = (int(x) for x in d_cnt.get())
        return d_mask.get(), count, None if d_pairs is None else d_pairs.get(), total, reports, clean
    finally:
        for x in (d_mask, d_cnt, d_pairs):
            if x is not None:
                x.free()


# ---- rectangle sets ----------------------------------------------------------------------------------------------------------------
def random_rects(rng, n, oracle, quads, extent, non_finite):
    """f32 [8][n] and a few words about it"""
    if quads:        # eight free floats: not a rectangle, the parallel-axis certificate must read thin
        s = (rng.uniform(-extent, extent, (1, n)) + rng.uniform(-2, 2, (8, n))).astype(F)
    else:
        s = oracle.rects_from_poses(*wl.random_obb_pose_planes(n, seed=int(rng.integers(1 << 30)), extent=extent)[:5]).copy()
    with np.errstate(all="ignore"):
        for q in np.flatnonzero(rng.random(n) < 0.02):       # outliers
            if rng.random() < 0.5:
                s[:, q] *= F(10.0 ** rng.integers(2, 7))
            else:
                s[:, q] += F(rng.choice([1e30, 2.0 ** 60, -2.0 ** 61, 1e-30]))      # (2^61: the edge of the certificate's domain)
    if non_finite:
        for q in np.flatnonzero(rng.random(n) < 0.03) if n > 1 else [0]:
            s[int(rng.integers(0, 8)), q] = rng.choice(np.array([np.nan, np.inf, -np.inf, 3e38], F))
    if n > 3 and rng.random() < 0.5:                             # duplicated rectangles
        src, dst = rng.integers(0, n, n // 3), rng.integers(0, n, n // 3)
        s[:, dst] = s[:, src]
    return s


def upload(eng, planes, offset):
    n = planes.shape[1]
    host = np.full((8, n + 4), np.nan, F)
    host[:, offset:offset + n] = planes
    d = eng.to_device(host)
    return d, [d.row(k) + 4 * offset for k in range(8)]


def reference(oracle, a, b):
    """bool [n_a][n_b]: the oracle on the materialised pairs (A_i, B_j)"""
    n_a, n_b = a.shape[1], b.shape[1]
    res, _ = oracle.sat_rect_pairs_verts(np.concatenate([np.repeat(a, n_b, axis=1), np.tile(b, n_a)]))
    return res.reshape(n_a, n_b).astype(bool)


def one(eng, rng, idx, announce=None, oracle=None):
    """One configuration; `announce(text)` is called with its description BEFORE any GPU work.  Returns (ok, (description, results))."""
    if oracle is None:
        from oracle import cpu as oracle
    n_a, n_b = draw_sizes(rng, 1 << 20)
    same = bool(rng.random() < 1 / 3)
    quads = bool(rng.random() < 0.25)
    extent = float(rng.choice([60.0, 40.0, 20.0, 10.0, 5.0, 2.5, 1.0]))
    non_finite = bool(rng.random() < 0.4)
    if same:
        n_a = n_b = min(n_a, 1 << 10)
    a = random_rects(rng, n_a, oracle, quads, extent, non_finite)
    b = a if same else random_rects(rng, n_b, oracle, quads, extent, non_finite)
    call = draw_call(rng, n_a, n_b)
    offs = (int(rng.integers(0, 4)), int(rng.integers(0, 4)))
    ref = reference(oracle, a, b)
    want = expected(ref, call["upper"], call["rb"], call["cb"])
    total = int(want.sum())
    cap = capacity_of(call["cap_kind"], total)
    desc = (f"config {idx}: {n_a} x {n_b} {'quads' if quads else 'rectangles'}, extent {extent}, {'non-finite coordinates' if non_finite else 'finite'}, "
            f"{'A = B (the same memory)' if same else 'two sets'}, plane offsets {offs}, {describe_call(call, n_b, total, cap)}")
    if announce is not None:
        announce(desc)
    da, pa = upload(eng, a, offs[0])
    db, pb = (da, pa) if same else upload(eng, b, offs[1])
    kw = dict(row_base=call["rb"], col_base=call["cb"], upper=call["upper"])
    try:
        got = run_call(eng, lambda m, ld, c: eng.sat_rect_cross_mask(pa, n_a, pb, n_b, m, ld_words=ld, count=c, **kw),
                       lambda p, capacity, c: eng.sat_rect_cross_pairs(pa, n_a, pb, n_b, p, capacity, c, **kw), n_a, call, cap)
    finally:
        da.free()
        if not same:
            db.free()
    complaints = compare(*got, want, n_b, call["rb"], call["cb"], cap)
    LAST.update(hits=total, misses=want.size - total)
    if complaints:
        print(f"MISMATCH {desc}: " + "; ".join(complaints))
    return not complaints, (desc, n_a * n_b)


def main(name="cross_fuzz", one_fn=None):
    configs = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed, origin = (int(sys.argv[2]), "the command line") if len(sys.argv) > 2 else fuzz_seed.commit_seed()
    print(f"{name}: {configs} configurations, seed {seed} ({origin})", flush=True)
    from oracle import cpu as oracle
    oracle.set_num_threads(oracle.usable_cores())
    eng = pkg.Engine(0)
    fails = total = 0
    for i in range(configs):
        ok, info = (one_fn or one)(eng, np.random.default_rng([seed, i]), i, None, oracle)
        fails += not ok
        total += info[-1]
        if (i + 1) % 50 == 0:
            print(f"  {i + 1} / {configs} configurations, {fails} failures so far", flush=True)
    print(f"{configs} configurations, {fails} failures; {total} results compared")
    eng.close()
    sys.exit(1 if fails else 0)


if __name__ == "__main__":
    main()
