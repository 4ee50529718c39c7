"""The exploring leg of the swept broad phase's fuzzer (tests/tools/sweep_broad_fuzz.py), after tests/test_gpu_cast_fuzz_explore.py: the
generator of the fixed-seed leg (test_gpu_sweep_broad.py test_fuzz_at_a_fixed_seed) through tests/fuzz_explore_leg.py, which says how it
is seeded, replayed (C2D_FUZZ_SEED / C2D_FUZZ_INDEX with this file) and traced ($C2D_FUZZ_TRACE_DIR/sweep_broad.txt).  Over its run the
leg must have compared a pair that touches only in motion and a pair that never touches."""
import pytest

import fuzz_explore_leg

pytestmark = pytest.mark.gpu

LEG, LEG_INDEX = "sweep_broad", 18      # (the seed offset continues the table of tests/test_gpu_fuzz_explore.py; 17 is the casts')
TOOL = "sweep_broad_fuzz"
PROOF = {"pairs that touch only in motion": ("moving_hits",), "misses": ("misses",)}      # what the run must have compared: wording -> keys of the tool's LAST


def test_sweep_broad_differential_fuzz_at_this_commits_seed(eng, oracle, wl, capsys):   # (`oracle`: sizes the OpenMP team to the box's CPU share)
    fuzz_explore_leg.run(eng, wl, capsys, LEG, LEG_INDEX, TOOL, PROOF)
