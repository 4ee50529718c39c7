"""The exploring leg of the grid shape-cast fuzzer (tests/tools/cast_grid_fuzz.py), after tests/test_gpu_cast_fuzz_explore.py: the
generator of the fixed-seed leg (test_gpu_casts_grid.py test_fixed_seed_fuzz), seeded from the commit under test (tests/tools/fuzz_seed.py)
and run for a time budget instead of a configuration count.  Configuration i is drawn from np.random.default_rng([leg seed, i]), so
    C2D_FUZZ_SEED=<base seed printed> C2D_FUZZ_INDEX=<i> python -m pytest tests/test_gpu_cast_grid_fuzz_explore.py -m gpu
runs exactly that one.  $C2D_FUZZ_SECONDS, default 40, is divided by eight as for the other per-configuration legs: 5 s.  The seed is
printed BEFORE the leg starts (past pytest's capture) and every configuration is named, before it runs, in
$C2D_FUZZ_TRACE_DIR/cast_grid.txt (default: build/fuzz_trace under the repository, which git ignores).  Over its run the leg must have compared a
query with a winner and one without."""
import importlib.util
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LEG, LEG_INDEX = "cast_grid", 21      # (the seed offset continues the table of tests/test_gpu_fuzz_explore.py; 20 is the grid clearances')


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cast_grid_differential_fuzz_at_this_commits_seed(eng, oracle, wl, capsys):   # (`oracle`: sizes the OpenMP team to the box's CPU share)
    base, origin = _tool("fuzz_seed").commit_seed()
    seed = (base + 0x3C6EF35F * LEG_INDEX) & 0x7FFFFFFF
    budget = float(os.environ.get("C2D_FUZZ_SECONDS", "40")) / 8
    only = os.environ.get("C2D_FUZZ_INDEX")
    fz = _tool("cast_grid_fuzz")
    trace_dir = os.environ.get("C2D_FUZZ_TRACE_DIR") or os.path.join(ROOT, "build", "fuzz_trace")
    try:
        os.makedirs(trace_dir, exist_ok=True)
        trace = open(os.path.join(trace_dir, LEG + ".txt"), "w")
    except OSError:   # a read-only checkout: the trace goes where the box lets it
        import tempfile

        trace_dir = tempfile.mkdtemp(prefix="c2d_fuzz_trace_")
        trace = open(os.path.join(trace_dir, LEG + ".txt"), "w")
    with capsys.disabled():
        print(f"\n[fuzz] {LEG}: seed {seed} = base seed {base} ({origin}) + leg offset, " + (f"{budget:.0f} s" if only is None else f"configuration {only} alone")
              + f"; reproduce with C2D_FUZZ_SEED={base} C2D_FUZZ_INDEX=<index of the configuration>; configurations named in {trace.name}", flush=True)
    trace.write(f"# {LEG}: seed {seed}, base seed {base} ({origin})\n")
    last = {"text": "(none yet)"}

    def announce(text):
        last["text"] = text
        trace.write(text + "\n")
        trace.flush()
        os.fsync(trace.fileno())

    t0, i, done = time.time(), 0 if only is None else int(only), 0
    hit = miss = False
    try:
        while time.time() - t0 < budget:
            ok, what = fz.one(eng, wl, np.random.default_rng([seed, i]), i, announce)
            hit, miss = hit or fz.LAST["hits"] > 0, miss or fz.LAST["misses"] > 0
            assert ok, f"{LEG}: differs from the reference at seed {seed} (C2D_FUZZ_SEED={base} C2D_FUZZ_INDEX={i}, {origin}), {last['text']}; {what}"
            i, done = i + 1, done + 1
            if only is not None:
                break
    finally:
        trace.write(f"# {done} configurations completed in {time.time() - t0:.1f} s\n")
        trace.close()
    with capsys.disabled():
        print(f"[fuzz] {LEG}: {done} configurations in {time.time() - t0:.1f} s, 0 differences", flush=True)
    if only is not None:
        return
    assert done >= 3, f"{LEG}: only {done} configurations fit into {budget} s"
    assert hit and miss, f"{LEG}: {done} configurations compared hits: {hit}, misses: {miss}"
