"""The exploring legs of the differential fuzzers: the same generators as the fixed-seed legs (test_gpu_sat.py
test_poly_differential_fuzz, test_gpu_mc.py test_mc_differential_fuzz, test_gpu_poly_binned.py test_binned_differential_fuzz,
tests/tools/pose_fuzz.py; and tests/tools/verts_fuzz.py for the headline vertex-format entry points), seeded from the commit under test (tests/tools/fuzz_seed.py) and run for a time budget instead of
a configuration count, so that every run of the suite at a new commit meets inputs no earlier run has met.  Round 5's one
defect — the binning pass's move kernel reading past its arrays on a last partial tile — passed two green runs of the
fixed-seed suite and was met by a soak outside it (profiles/notes_r05_move_kernel_overread.md).

Every leg prints its seed BEFORE it starts (past pytest's capture: a GPU fault takes the captured output down with the
process) and names every configuration, before it runs, in gpurun_out/fuzz_trace/<leg>.txt.  To reproduce a failure:
    C2D_FUZZ_SEED=<base seed printed> python -m pytest tests/test_gpu_fuzz_explore.py -m gpu -k <leg>
$C2D_FUZZ_SECONDS, default 40, is the budget of each of the first five legs (sat_rect_pose .. sat_rect_verts).  Those five thread ONE
sequential generator through their configurations: configuration i is a function of the seed and of every draw of configurations
0 .. i - 1, so a failure there reproduces only by running the leg from its start.

The twelve legs added after them (rect_cross .. clearances: the N x M, broad-phase, list-driven, ray, polygon Monte-Carlo, grid ray and
clearance entry points, tests/tools/cross_fuzz.py, poly_cross_fuzz.py, broad_fuzz.py, poly_broad_fuzz.py, contact_fuzz.py, manifold_fuzz.py,
distance_fuzz.py, ray_fuzz.py, mc_poly_fuzz.py, sweep_fuzz.py, ray_grid_fuzz.py, clearance_fuzz.py) get one eighth of that budget each, 5 s
by default (twelve eighths in all), and draw configuration i from
np.random.default_rng([leg seed, i]): there a configuration IS a function of (seed, index) alone, and
    C2D_FUZZ_SEED=<base seed> C2D_FUZZ_INDEX=<i> python -m pytest tests/test_gpu_fuzz_explore.py -m gpu -k <leg>
runs exactly that one.  Over its run each of the twelve must have compared a colliding and a non-colliding result (rays and grid rays: a
hit and a miss; clearances: a winner that is hit and one that is not; mc_poly: a scene with 0 < hits < samples)."""
import os
import time

import numpy as np
import pytest

from best_key_harness import load_tool as _tool

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OLD_LEGS = ("sat_rect_pose", "sat_poly_rows", "sat_poly_binned", "mc_scenes", "sat_rect_verts")   # one sequential generator each, the whole budget
NEW_LEGS = ("rect_cross", "poly_cross", "rect_broad", "poly_broad", "contacts", "manifolds", "distances", "rays", "mc_poly", "sweeps",
            "ray_grid", "clearances")   # a stream per configuration, an eighth
LEGS = OLD_LEGS + NEW_LEGS   # (append only: a leg's seed offset is its index)
TOOL = {"sat_rect_verts": "verts_fuzz", "sat_rect_pose": "pose_fuzz", "sat_poly_rows": "poly_fuzz", "sat_poly_binned": "binned_fuzz", "mc_scenes": "mc_fuzz",
        "rect_cross": "cross_fuzz", "poly_cross": "poly_cross_fuzz", "rect_broad": "broad_fuzz", "poly_broad": "poly_broad_fuzz", "contacts": "contact_fuzz",
        "manifolds": "manifold_fuzz", "distances": "distance_fuzz", "rays": "ray_fuzz", "mc_poly": "mc_poly_fuzz", "sweeps": "sweep_fuzz",
        "ray_grid": "ray_grid_fuzz", "clearances": "clearance_fuzz"}
TAKES_ORACLE = ("rect_cross", "poly_cross", "rect_broad", "manifolds")   # one(eng, rng, idx, announce, oracle)
TAKES_WL = ("clearances",)   # one(eng, wl, rng, idx, announce)


@pytest.mark.parametrize("leg", LEGS)
def test_differential_fuzz_at_this_commits_seed(eng, oracle, wl, capsys, leg):   # (`oracle`: sizes the OpenMP team to the box's CPU share)
    base, origin = _tool("fuzz_seed").commit_seed()
    seed = (base + 0x3C6EF35F * LEGS.index(leg)) & 0x7FFFFFFF   # one stream per leg
    new = leg in NEW_LEGS
    budget = float(os.environ.get("C2D_FUZZ_SECONDS", "40")) / (8 if new else 1)
    only = os.environ.get("C2D_FUZZ_INDEX") if new else None   # (the first five legs cannot start in the middle of their one stream)
    fz = _tool(TOOL[leg])
    trace_dir = os.path.join(ROOT, "gpurun_out", "fuzz_trace")
    try:
        os.makedirs(trace_dir, exist_ok=True)
        trace = open(os.path.join(trace_dir, leg + ".txt"), "w")
    except OSError:   # a read-only checkout: the trace goes where the box lets it
        import tempfile

        trace_dir = tempfile.mkdtemp(prefix="c2d_fuzz_trace_")
        trace = open(os.path.join(trace_dir, leg + ".txt"), "w")
    with capsys.disabled():
        print(f"\n[fuzz] {leg}: seed {seed} = base seed {base} ({origin}) + leg offset, " + (f"{budget:.0f} s" if only is None else f"configuration {only} alone")
              + f"; reproduce with C2D_FUZZ_SEED={base}" + (" C2D_FUZZ_INDEX=<index of the configuration>" if new else "")
              + f"; configurations named in {trace.name}", flush=True)
    trace.write(f"# {leg}: seed {seed}, base seed {base} ({origin})\n")
    last = {"text": "(none yet)"}

    def announce(text):
        last["text"] = text
        trace.write(text + "\n")
        trace.flush()
        os.fsync(trace.fileno())

    rng = np.random.default_rng(seed)   # the first five legs: one generator through every configuration
    t0, i, done = time.time(), 0 if only is None else int(only), 0
    hit = miss = False
    try:
        while time.time() - t0 < budget:
            if leg == "sat_poly_binned":
                ok, what, _ = fz.one(eng, rng, i, seed, announce)   # (the tool keys its polygons by seed * 100000 + index)
            elif not new:
                ok, what = fz.one(eng, rng, i, announce)
            else:   # a stream of its own per configuration: (seed, index) alone names it
                args = (eng,) + ((wl,) if leg in TAKES_WL else ()) + (np.random.default_rng([seed, i]), i, announce) + ((oracle,) if leg in TAKES_ORACLE else ())
                ok, what = fz.one(*args)
                if leg == "mc_poly":
                    hit = miss = hit or bool(((fz.LAST["hits"] > 0) & (fz.LAST["hits"] < fz.LAST["samples"])).any())
                else:
                    hit, miss = hit or fz.LAST["hits"] > 0, miss or fz.LAST["misses"] > 0
            assert ok, (f"{leg}: differs from the reference at seed {seed} (C2D_FUZZ_SEED={base}" + (f" C2D_FUZZ_INDEX={i}" if new else "")
                        + f", {origin}), {last['text']}; {what}")
            i, done = i + 1, done + 1
            if only is not None:
                break
    finally:
        trace.write(f"# {done} configurations completed in {time.time() - t0:.1f} s\n")
        trace.close()
    with capsys.disabled():
        print(f"[fuzz] {leg}: {done} configurations in {time.time() - t0:.1f} s, 0 differences", flush=True)
    if only is not None:
        return
    assert done >= 3, f"{leg}: only {done} configurations fit into {budget} s"
    assert not new or (hit and miss), f"{leg}: {done} configurations compared " + ("no scene with 0 < hits < samples" if leg == "mc_poly" else f"hits: {hit}, misses: {miss}")
