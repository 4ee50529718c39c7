"""The exploring leg of the proximity pair search's fuzzer (tests/tools/near_broad_fuzz.py), after tests/test_gpu_cast_fuzz_explore.py:
the generator of the fixed-seed leg (test_gpu_near_broad.py test_fuzz_at_a_fixed_seed) through tests/fuzz_explore_leg.py, which says how
it is seeded, replayed (C2D_FUZZ_SEED / C2D_FUZZ_INDEX with this file) and traced ($C2D_FUZZ_TRACE_DIR/near_broad.txt).  Over its run
the leg must have compared a pair that is listed through the margin alone and a pair that is not listed."""
import pytest

import fuzz_explore_leg

pytestmark = pytest.mark.gpu

LEG, LEG_INDEX = "near_broad", 19      # (the seed offset continues the table of tests/test_gpu_fuzz_explore.py; 18 is the swept broad phase's)
TOOL = "near_broad_fuzz"
PROOF = {"pairs listed through the margin alone": ("apart",), "misses": ("misses",)}      # what the run must have compared: wording -> keys of the tool's LAST


def test_near_broad_differential_fuzz_at_this_commits_seed(eng, oracle, wl, capsys):   # (`oracle`: sizes the OpenMP team to the box's CPU share)
    fuzz_explore_leg.run(eng, wl, capsys, LEG, LEG_INDEX, TOOL, PROOF)
