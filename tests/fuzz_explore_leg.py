"""The body of the exploring fuzz legs that came after the table of tests/test_gpu_fuzz_explore.py (test_gpu_cast_fuzz_explore.py,
test_gpu_sweep_broad_fuzz_explore.py, test_gpu_near_broad_fuzz_explore.py, test_gpu_clearance_grid_fuzz_explore.py,
test_gpu_cast_grid_fuzz_explore.py): the generator of a tool's fixed-seed leg, seeded from the commit under test
(tests/tools/fuzz_seed.py) and run for a time budget instead of a configuration count.  Configuration i is drawn from
np.random.default_rng([leg seed, i]), so
    C2D_FUZZ_SEED=<base seed printed> C2D_FUZZ_INDEX=<i> python -m pytest tests/test_gpu_<leg>_fuzz_explore.py -m gpu
runs exactly that one.  $C2D_FUZZ_SECONDS, default 40, is divided by eight as for the other per-configuration legs: 5 s.  The seed is
printed BEFORE the leg starts (past pytest's capture) and every configuration is named, before it runs, in
$C2D_FUZZ_TRACE_DIR/<leg>.txt (default: build/fuzz_trace under the repository, which git ignores).  Each file states its leg's name,
its index (the seed offset, which continues the table of tests/test_gpu_fuzz_explore.py: append only), its tool, and what the run
must have compared for it not to be vacuous."""
import os
import time

import numpy as np

from best_key_harness import load_tool as _tool

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def run(eng, wl, capsys, leg, leg_index, tool, proof, takes_wl=False):
    """proof: {wording: keys of the tool's LAST}: over the run, some configuration must have had a positive sum of those keys, for each
    entry; takes_wl: the tool's one() is one(eng, wl, rng, idx, announce), not one(eng, rng, idx, announce)"""
    base, origin = _tool("fuzz_seed").commit_seed()
    seed = (base + 0x3C6EF35F * leg_index) & 0x7FFFFFFF
    budget = float(os.environ.get("C2D_FUZZ_SECONDS", "40")) / 8
    only = os.environ.get("C2D_FUZZ_INDEX")
    fz = _tool(tool)
    trace_dir = os.environ.get("C2D_FUZZ_TRACE_DIR") or os.path.join(ROOT, "build", "fuzz_trace")
    try:
        os.makedirs(trace_dir, exist_ok=True)
        trace = open(os.path.join(trace_dir, leg + ".txt"), "w")
    except OSError:   # a read-only checkout: the trace goes where the box lets it
        import tempfile

        trace_dir = tempfile.mkdtemp(prefix="c2d_fuzz_trace_")
        trace = open(os.path.join(trace_dir, leg + ".txt"), "w")
    with capsys.disabled():
        print(f"\n[fuzz] {leg}: seed {seed} = base seed {base} ({origin}) + leg offset, " + (f"{budget:.0f} s" if only is None else f"configuration {only} alone")
              + f"; reproduce with C2D_FUZZ_SEED={base} C2D_FUZZ_INDEX=<index of the configuration>; configurations named in {trace.name}", flush=True)
    trace.write(f"# {leg}: seed {seed}, base seed {base} ({origin})\n")
    last = {"text": "(none yet)"}

    def announce(text):
        last["text"] = text
        trace.write(text + "\n")
        trace.flush()
        os.fsync(trace.fileno())

    t0, i, done = time.time(), 0 if only is None else int(only), 0
    seen = dict.fromkeys(proof, 0)
    try:
        while time.time() - t0 < budget:
            ok, what = fz.one(eng, *((wl,) if takes_wl else ()), np.random.default_rng([seed, i]), i, announce)
            for wording, keys in proof.items():
                seen[wording] += sum(int(fz.LAST[k]) for k in keys)
            assert ok, f"{leg}: differs from the reference at seed {seed} (C2D_FUZZ_SEED={base} C2D_FUZZ_INDEX={i}, {origin}), {last['text']}; {what}"
            i, done = i + 1, done + 1
            if only is not None:
                break
    finally:
        trace.write(f"# {done} configurations completed in {time.time() - t0:.1f} s\n")
        trace.close()
    compared = ", ".join(f"{wording}: {n}" for wording, n in seen.items())
    with capsys.disabled():
        print(f"[fuzz] {leg}: {done} configurations in {time.time() - t0:.1f} s, 0 differences ({compared})", flush=True)
    if only is not None:
        return
    assert done >= 3, f"{leg}: only {done} configurations fit into {budget} s"
    assert all(seen.values()), f"{leg}: {done} configurations compared {compared}"
