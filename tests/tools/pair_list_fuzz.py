"""What the differential fuzzers of the list-driven queries (contact_fuzz.py, manifold_fuzz.py, distance_fuzz.py, sweep_fuzz.py) do
once a configuration is drawn, stated once, as tests/pair_list_harness.py states their tests' frame: run() builds the u32 list with
its bases (an entry that wraps is judged as the call judges it), takes the bound from the device count, uploads, bands every output
between GUARD records of BAND bytes, calls, synchronises, asks check_async, frees on every way out and hands the buffers to
compare(); main() is the command line of all four.  Each tool keeps its generator, one(), and what it reports in LAST.

compare() is the judge, a pure function on host arrays (tests/test_fuzz_compare_cpu.py plants faults into it): every output record
by record under the query's own equality (pair_list_harness.QUERIES), `reserved` fields zero, the guard bands intact, every record at
or beyond min(n_pairs, *d_n_pairs) untouched, an error reported exactly when the reference has a bad entry, and check_async clean
afterwards."""
import importlib
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from __graft_entry__ import load_package  # noqa: E402
import pair_list_harness as h  # noqa: E402

pkg = load_package()
wl = importlib.import_module("c2d_amd.workloads")
GUARD, BAND = h.GUARD, h.BAND


def tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


pbf = tool("poly_broad_fuzz")      # its random sets and its upload
fuzz_seed = tool("fuzz_seed")


def compare(query, gots, reported, clean, wants, capacity):
    """gots: per output of `query` its records [GUARD + capacity + GUARD], as the call left buffers of BAND bytes; reported: the
    synchronisation raised; clean: check_async afterwards was; wants: per output the reference's records of the first
    min(n_pairs, *d_n_pairs) entries -> the list of complaints"""
    out = []
    bound = len(wants[0])
    for got, want, same, dt, noun in zip(gots, wants, query.sames, query.dts, query.nouns):
        if got.dtype != dt or got.shape != (capacity + 2 * GUARD,) or len(want) != bound or bound > capacity:
            out.append(f"{noun}: a buffer of {got.shape} {got.dtype} for a capacity of {capacity} and {len(want)} expected records")
            continue
        raw = got.view(np.uint8).reshape(-1, dt.itemsize)
        if not ((raw[:GUARD] == BAND).all() and (raw[GUARD + capacity:] == BAND).all()):
            out.append(f"{noun}: written outside the output")
        if not (raw[GUARD + bound: GUARD + capacity] == BAND).all():
            out.append(f"{noun}: written at or beyond min(n_pairs, *d_n_pairs)")
        records = got[GUARD: GUARD + bound]
        ok = same(records, want)
        for f in dt.names:
            if f.startswith("reserved"):
                ok &= records[f] == 0
        if not ok.all():
            q = int(np.flatnonzero(~ok)[0])
            out.append(f"{int((~ok).sum())} of {bound} {noun} differ; first at {q}: got {records[q]}, want {want[q]}")
    expect = bool((wants[0]["flags"] & query.bad_pair).any())
    if bool(reported) != expect:
        out.append(f"error reported: {bool(reported)}, the list {'has' if expect else 'has no'} bad entry")
    if not clean:
        out.append("check_async still reports an error after the synchronisation")
    return out


def run(eng, query, desc, a, b, pairs, cap, n_dev, rb, cb, place=None, extras=()):
    """One drawn configuration through the call of `query` and the judge.  a, b: two polygon sets, uploaded at place = [(offset,
    stride - n)] * 2 (b is a: the same memory), or, without `place`, two rectangle sets f32[8][n]; pairs: the list in local indices,
    listed behind the bases rb, cb in a buffer of `cap` entries; n_dev: the device count or None; extras: Query.extras' form.
    -> (ok, (desc, the records compared), the reference's records per output)"""
    listed = np.full((cap, 2), 0xFFFFFFFF, np.uint32)
    listed[:len(pairs)] = ((pairs + (rb, cb)) & 0xFFFFFFFF).astype(np.uint32)
    # what the call sees is the u32 list minus the bases: an entry that wrapped is judged as the call judges it
    li, lj = listed[:, 0].astype(np.int64) - rb, listed[:, 1].astype(np.int64) - cb
    bound = cap if n_dev is None else min(cap, int(n_dev))
    wants = h.outputs((query.rect_ref if place is None else query.poly_ref)(a, b, li[:bound], lj[:bound], *extras))
    keep = []
    try:
        if place is None:
            keep += [eng.to_device(a), eng.to_device(b)]
            sets = ([keep[0].row(k) for k in range(8)], a.shape[1], [keep[1].row(k) for k in range(8)], b.shape[1])
            call = getattr(eng, query.rect)
        else:
            sa, kept = pbf.upload(eng, a, place[0][0], a[0].shape[1] + place[0][1])
            keep += kept
            sb = sa
            if b is not a:
                sb, kept = pbf.upload(eng, b, place[1][0], b[0].shape[1] + place[1][1])
                keep += kept
            sets, call = (sa, sb), getattr(eng, query.poly)
        keep += [h.Extras(eng, extras), eng.to_device(listed)]
        kw, d_pairs = keep[-2].kw, keep[-1]
        d_outs = [h.banded(eng, cap, dt) for dt in query.dts]
        keep += d_outs
        if n_dev is not None:
            keep.append(eng.to_device(np.array([int(n_dev)], np.uint64)))
        call(*sets, d_pairs, cap, *[d.ptr + GUARD * dt.itemsize for d, dt in zip(d_outs, query.dts)], n_pairs_dev=None if n_dev is None else keep[-1],
             row_base=rb, col_base=cb, **kw)
        try:
            eng.synchronize()
            reported = False
        except pkg.C2DError:
            reported = True
        try:
            eng.check_async()
            clean = True
        except pkg.C2DError:
            clean = False
        gots = [d.get() for d in d_outs]
    finally:
        for x in keep:
            x.free()
    complaints = compare(query, gots, reported, clean, wants, cap)
    if complaints:
        print(f"MISMATCH {desc}: " + "; ".join(complaints))
    return not complaints, (desc, bound), wants


def hits_and_misses(wants):
    return dict(hits=int((wants[0]["hit"] != 0).sum()), misses=int((wants[0]["hit"] == 0).sum()))


def main(name, one, noun):
    """usage: <tool>.py [configs] [seed]     (no seed: the commit's, tests/tools/fuzz_seed.py); configuration i is drawn from the
    stream (seed, i), as the suite draws it"""
    configs = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed, origin = (int(sys.argv[2]), "the command line") if len(sys.argv) > 2 else fuzz_seed.commit_seed()
    print(f"{name}: {configs} configurations, seed {seed} ({origin})", flush=True)
    eng = pkg.Engine(0)
    fails = total = 0
    for i in range(configs):
        ok, info = one(eng, np.random.default_rng([seed, i]), i)
        fails += not ok
        total += info[-1]
        if (i + 1) % 50 == 0:
            print(f"  {i + 1} / {configs} configurations, {fails} failures so far", flush=True)
    print(f"{configs} configurations, {fails} failures; {total} {noun} compared")
    eng.close()
    sys.exit(1 if fails else 0)
