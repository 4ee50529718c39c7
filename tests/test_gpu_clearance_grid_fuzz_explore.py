"""The exploring leg of the grid clearance query's fuzzer (tests/tools/clearance_grid_fuzz.py), after
tests/test_gpu_near_broad_fuzz_explore.py: the generator of the fixed-seed leg (test_gpu_clearances_grid.py test_fuzz_at_a_fixed_seed)
through tests/fuzz_explore_leg.py, which says how it is seeded, replayed (C2D_FUZZ_SEED / C2D_FUZZ_INDEX with this file) and traced
($C2D_FUZZ_TRACE_DIR/clearance_grid.txt).  Over its run the leg must have compared records; their mix (winners through the margin alone,
NONE records, bad queries) is asserted by the fixed-seed leg, whose configurations do not change."""
import pytest

import fuzz_explore_leg

pytestmark = pytest.mark.gpu

LEG, LEG_INDEX = "clearance_grid", 20      # (the seed offset continues the table of tests/test_gpu_fuzz_explore.py; 19 is the proximity pair search's)
TOOL = "clearance_grid_fuzz"
PROOF = {"records": ("winners", "none", "bad")}      # what the run must have compared: wording -> keys of the tool's LAST


def test_clearance_grid_differential_fuzz_at_this_commits_seed(eng, oracle, wl, capsys):   # (`oracle`: sizes the OpenMP team to the box's CPU share)
    fuzz_explore_leg.run(eng, wl, capsys, LEG, LEG_INDEX, TOOL, PROOF)
