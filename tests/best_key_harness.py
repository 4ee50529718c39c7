"""The one frame of the tests of the best-key queries (the ray casts, the clearances and the shape casts, each over all of B and through
the grid), as csrc/c2d_set_best.hpp and c2d_grid_best.hpp are the two frames of their kernels: the table QUERIES of what each query
states of its own, call() between guard bands, the call run twice, the two comparisons with their messages, the strip rule, the
refusals every two-set query shares, the reference of a scene whose polygons repeat, and what the fuzz tools share (their loader,
their command line, the tail of a failing configuration).  A plain module (pytest does not collect it) on numpy, pytest and the numpy
references only: it never loads libc2d.so, so tests/best_key_graph_check.py can import it after torch.
tests/test_best_key_harness_cpu.py drives it without a device."""
import importlib
import importlib.util
import os
import sys

import numpy as np

import cast_ref
import clearance_grid_ref
import clearance_ref
import pair_list_harness as h
import ray_grid_ref
import ray_ref

HERE = os.path.dirname(os.path.abspath(__file__))
TILE_ROWS, TILE_COLS, BLOCKS_PER_CU = 256, 64, 8      # queries per block and polygons per staged tile of the three all-of-B kernels, and
                                                      # the strip rule's target of blocks per compute unit (csrc/c2d_ray_strips.hpp)


def strips_of(cus, n_rows, n_b):
    """the strip rule of csrc/c2d_ray_strips.hpp on a device of `cus` compute units: as many strips of column tiles as fill it with
    BLOCKS_PER_CU blocks each, at least one and at most one per column tile"""
    row_tiles, col_tiles = -(-n_rows // TILE_ROWS), -(-n_b // TILE_COLS)
    return min(col_tiles, max(1, BLOCKS_PER_CU * cus // row_tiles))


# ---- the table -------------------------------------------------------------------------------------------------------------------------
def _rays(method, ptr, rays, n_rays, b_set, **kw):
    method(rays.ptrs, n_rays, b_set, ptr, **kw)


def _sets(method, ptr, a_set, b_set, n_a, **kw):
    method(a_set, b_set, ptr, **kw)


def _sets_within(method, ptr, a_set, b_set, n_a, max_dist, **kw):
    method(a_set, b_set, max_dist, ptr, **kw)


def _moving_sets(method, ptr, a_set, b_set, n_a, a_motion=None, b_motion=None, **kw):
    method(a_set, b_set, a_motion, b_motion, out=ptr, **kw)


class Query:
    """What one best-key query states of its own.  ref: its numpy reference module (.same, and .reference the reference call itself);
    dt: the record; method: the Engine method (the C symbol is "c2d_" + that); lay(method, ptr, *args, **kw): how the arguments of
    call() are laid before the output, the number of records being args[n_at]; sibling: the all-of-B query a grid query is compared
    with byte for byte; stats: the Engine's reader of the last call's counters; noun: a record's word in a message.  padded: the
    default capacity is max(n, 4) and call() returns the n records (the ray calls return the capacity's)."""

    def __init__(self, name, ref, reference, dt, lay, sibling=None, stats=None, noun="", n_at=2, padded=True):
        self.name, self.ref, self.reference, self.dt, self.method, self.lay = name, ref, reference, dt, name, lay
        self.sibling, self.stats, self.noun, self.n_at, self.padded = sibling, stats, noun, n_at, padded

    def __repr__(self):
        return self.name


RAY_CASTS = Query("poly_ray_casts", ray_ref, ray_ref.ray_casts, ray_ref.RAY_HIT_DT, _rays, noun="ray ", n_at=1, padded=False)
RAY_CASTS_GRID = Query("poly_ray_casts_grid", ray_grid_ref, ray_grid_ref.ray_casts, ray_ref.RAY_HIT_DT, _rays, RAY_CASTS, "poly_ray_casts_grid_stats",
                       noun="ray ", n_at=1, padded=False)
CLEARANCES = Query("poly_set_clearances", clearance_ref, clearance_ref.clearances, clearance_ref.CLEARANCE_DT, _sets)
CLEARANCES_GRID = Query("poly_set_clearances_grid", clearance_grid_ref, clearance_grid_ref.clearances, clearance_ref.CLEARANCE_DT, _sets_within,
                        CLEARANCES, "poly_set_clearances_grid_stats")
CASTS = Query("poly_set_casts", cast_ref, cast_ref.casts, cast_ref.CAST_DT, _moving_sets)
CASTS_GRID = Query("poly_set_casts_grid", cast_ref, cast_ref.casts, cast_ref.CAST_DT, _moving_sets, CASTS, "poly_set_casts_grid_stats")
QUERIES = (RAY_CASTS, RAY_CASTS_GRID, CLEARANCES, CLEARANCES_GRID, CASTS, CASTS_GRID)


# ---- the call and its checks -----------------------------------------------------------------------------------------------------------
def call(query, eng, *args, capacity=None, expect_error=False, band=None, **kw):
    """the query's call on `args` (Query.lay) into a buffer between guard bands: the bands and every record at or beyond n must be
    untouched; under expect_error the next synchronise reports status -1, once.  band: a buffer of h.banded(eng, capacity, dt) to use
    again (many small calls: it is filled with the band's byte first and stays the caller's).  -> the n records (the ray calls: the
    capacity's)"""
    n = args[query.n_at]
    cap = capacity if capacity is not None else max(n, 4) if query.padded else None
    got = h.banded_call(eng, query.dt, n, lambda ptr: query.lay(getattr(eng, query.method), ptr, *args, **kw), cap, expect_error, band)
    return got[:n].copy() if query.padded else got


def twice(query, eng, *args, **kw):
    """twice(query, eng, *args, what, **kw): call(), run twice: the two outputs must be the same bytes"""
    *args, what = args
    got, again = call(query, eng, *args, **kw), call(query, eng, *args, **kw)
    assert got.tobytes() == again.tobytes(), f"{what}: two runs differ"
    return got


def assert_same(query, got, want, what):
    ok = query.ref.same(got, want)
    if not ok.all():
        q = int(np.flatnonzero(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {len(want)} records differ; first at {query.noun}{q}: got {got[q]}, want {want[q]}")


def check_against_sibling(got, full, what, names):
    """the records of a grid query and of its all-of-B sibling on the same arguments (names: the two calls' words) are the same bytes"""
    assert got.dtype == full.dtype and got.shape == full.shape, f"{what}: {got.shape} {names[0]} records, {full.shape} {names[1]} records"
    size = got.dtype.itemsize
    differ = (got.view(np.uint8).reshape(-1, size) != full.view(np.uint8).reshape(-1, size)).any(axis=1)
    if differ.any():
        q = int(np.flatnonzero(differ)[0])
        raise AssertionError(f"{what}: the bytes differ from {names[1]}'; first at {q}: {names[0]} {got[q]}, {names[1]} {full[q]}")


def reduce_by_query(ref, R, ia, ib, bad_a, bad_b, **kw):
    """the reference of the queries ia against the polygons ib from R, the per-pair records of the DISTINCT polygons [n_a][n_b]
    (bad_a of the distinct queries, bad_b of ib): the pick is made once per distinct query against R[:, ib] and indexed by ia, so
    that the cost does not grow with len(ia); the self pair of SKIP_SELF depends on the query's own place, and matters only where it
    is the winner: those queries are reduced one by one."""
    rb, cb, flags = kw.get("row_base", 0), kw.get("col_base", 0), kw.get("flags", 0)
    Rb = R[:, ib]
    out = ref.reduce(Rb, bad_a, bad_b, col_base=cb)[ia]
    if flags & ref.SKIP_SELF:
        j_self = rb + np.arange(len(ia), dtype=np.int64) - cb
        own = (j_self >= 0) & (j_self < len(ib)) & (out["poly"].astype(np.int64) == cb + j_self)
        for q in np.flatnonzero(own):
            out[q] = ref.reduce(Rb[ia[q]:ia[q] + 1], bad_a[ia[q]:ia[q] + 1], bad_b, row_base=rb + int(q), col_base=cb, flags=flags)[0]
    return out


# ---- the refusals every two-set query shares ------------------------------------------------------------------------------------------
def refused_set_arguments(fn, PolySet, plane, out, symbol, last_error, off=8, accepted=True):
    """Every argument error the two-set queries share, each asserted as it is tried -> the names of the cases tried.  fn(a, b, rb, cb,
    flags, o) -> status: the C call on two c2d_poly_set (or None), the bases, the flags and the output pointer, whatever else the
    query takes standing still; PolySet(rows, n, stride, vx, vy, k): the struct; plane: device floats for 16 rows of 8; out: room for
    eight records; off: a byte offset that misaligns the output.  A refusal is status -1 with a message (last_error() -> bytes) that
    names `symbol` and says the case's word; the last two cases (unless accepted is False) are accepted, status 0: the no-op at
    n_a == 0, and both bases at exactly 2^32 - n under SKIP_SELF, which writes the eight records."""
    good, top = PolySet(16, 8, 0, plane, plane, 0), (1 << 32) - 8
    refusals = [("a NULL set A", "NULL", None, good), ("a NULL set B", "NULL", good, None), ("a NULL output", "NULL", good, good, 0, 0, 0, 0)]
    for rows in (0, 17):
        bad = PolySet(rows, 8, 0, plane, plane, 0)
        refusals += [(f"rows {rows} in A", "rows", bad, good), (f"rows {rows} in B", "rows", good, bad), (f"rows {rows} in an empty B", "rows", good, PolySet(rows, 0, 0, 0, 0, 0))]
    refusals += [("a misaligned plane of A", "aligned", PolySet(16, 8, 0, plane + 2, plane, 0), good),
                 ("a misaligned plane of B", "aligned", good, PolySet(16, 8, 0, plane, plane + 1, 0)),
                 ("a NULL plane", "NULL", PolySet(16, 8, 0, 0, plane, 0), good), ("a misaligned output", "aligned", good, good, 0, 0, 0, out + off),
                 ("stride < n in A", "stride", PolySet(16, 8, 7, plane, plane, 0), good), ("stride < n in B", "stride", good, PolySet(16, 8, 7, plane, plane, 0))]
    refusals += [(f"flags {flags}", "flag", good, good, 0, 0, flags) for flags in (2, 4, 16, -1)]
    refusals += [("row_base + n_a > 2^32", "2^32", good, good, top + 1), ("col_base + n_b > 2^32", "2^32", good, good, 0, top + 1)]
    accepts = [("n_a == 0: a no-op", PolySet(16, 0, 0, 0, 0, 0), 0, 0), ("exactly 2^32", good, top, 1)][:2 * accepted]
    for name, word, a, b, *rest in refusals:
        status, said = fn(a, b, *(rest + [0, 0, 0, out][len(rest):])), last_error()
        assert status == -1 and symbol.encode() in said and word.encode() in said, f"{symbol}, {name}: status {status}, message {said!r}"
    for name, a, base, flags in accepts:
        status = fn(a, good, base, base, flags, out)
        assert status == 0, f"{symbol}, {name}: status {status}, message {last_error()!r}"
    return [r[0] for r in refusals + accepts]


# ---- what the fuzz tools share --------------------------------------------------------------------------------------------------------
def load_tool(name):
    """the module tests/tools/<name>.py, loaded afresh (the tools are no package)"""
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def mismatch(got, want, same, what):
    """the tail of a tool's one(): None where the records equal the reference's, else `what` with the count and the first difference"""
    ok = same(got, want)
    if ok.all():
        return None
    q = int(np.flatnonzero(~ok)[0])
    return what + f": {int((~ok).sum())} records differ; first at {q}: got {got[q]}, want {want[q]}"


def fuzz_main(name, one, needs_wl):
    """usage: <tool>.py [configs] [seed]     (no seed: a random one, printed); configuration i is drawn from the stream (seed, i), as
    the suite draws it; one(eng, [wl,] rng, i) -> (ok, description)"""
    sys.path.insert(0, os.path.dirname(HERE))
    from __graft_entry__ import load_package

    pkg = load_package()
    extra = (importlib.import_module("c2d_amd.workloads"),) if needs_wl else ()
    configs = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else int.from_bytes(os.urandom(4), "little")
    print(f"{name}: seed {seed}, {configs} configurations", flush=True)
    eng = pkg.Engine(0)
    bad = 0
    for idx in range(configs):
        ok, what = one(eng, *extra, np.random.default_rng([seed, idx]), idx)
        print(("ok   " if ok else "FAIL ") + what, flush=True)
        bad += not ok
    eng.close()
    sys.exit(1 if bad else 0)
