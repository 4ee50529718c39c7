"""The exploring leg of tests/tools/overlap_fuzz.py: the generator of the fixed-seed leg (test_gpu_overlaps.py), seeded from the
commit under test (tests/tools/fuzz_seed.py), configuration i drawn from np.random.default_rng([leg seed, i]), for at most
$C2D_FUZZ_SECONDS / 8 (5 s by default) or 40 configurations, whichever comes first.  The seed is printed before the leg starts, past
pytest's capture, so that
    C2D_FUZZ_SEED=<base seed printed> C2D_FUZZ_INDEX=<i> python -m pytest tests/test_gpu_overlaps_fuzz.py -m gpu
runs exactly one configuration again.  Over its run the leg must have compared hits, misses and a positive area."""
import os
import time

import numpy as np
import pytest

from best_key_harness import load_tool

pytestmark = pytest.mark.gpu

LEG, LEG_INDEX = "overlaps", 22      # (the seed offset continues the table of tests/test_gpu_fuzz_explore.py; 21 is the grid casts')
MAX_CONFIGS = 40


def test_overlap_differential_fuzz_at_this_commits_seed(eng, oracle, capsys):   # (`oracle`: sizes the OpenMP team to the box's CPU share)
    base, origin = load_tool("fuzz_seed").commit_seed()
    seed = (base + 0x3C6EF35F * LEG_INDEX) & 0x7FFFFFFF
    budget = float(os.environ.get("C2D_FUZZ_SECONDS", "40")) / 8
    only = os.environ.get("C2D_FUZZ_INDEX")
    fz = load_tool("overlap_fuzz")
    with capsys.disabled():
        print(f"\n[fuzz] {LEG}: seed {seed} = base seed {base} ({origin}) + leg offset, "
              + (f"{budget:.0f} s or {MAX_CONFIGS} configurations" if only is None else f"configuration {only} alone")
              + f"; reproduce with C2D_FUZZ_SEED={base} C2D_FUZZ_INDEX=<index of the configuration>", flush=True)
    last = {"text": "(none yet)"}
    t0, i, done = time.time(), 0 if only is None else int(only), 0
    seen = dict(hits=0, misses=0, areas=0)
    while time.time() - t0 < budget and done < MAX_CONFIGS:
        ok, what = fz.one(eng, np.random.default_rng([seed, i]), i, lambda text: last.update(text=text))
        for k in seen:
            seen[k] += int(fz.LAST[k])
        assert ok, f"{LEG}: differs from the reference at seed {seed} (C2D_FUZZ_SEED={base} C2D_FUZZ_INDEX={i}, {origin}), {last['text']}; {what}"
        i, done = i + 1, done + 1
        if only is not None:
            break
    with capsys.disabled():
        print(f"[fuzz] {LEG}: {done} configurations in {time.time() - t0:.1f} s, 0 differences ({seen})", flush=True)
    if only is not None:
        return
    assert done >= 3, f"{LEG}: only {done} configurations fit into {budget} s"
    assert all(seen.values()), f"{LEG}: {done} configurations compared {seen}"
