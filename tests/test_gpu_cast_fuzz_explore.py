"""The exploring leg of the shape-cast fuzzer (tests/tools/cast_fuzz.py), after the legs of tests/test_gpu_fuzz_explore.py: the generator of
the fixed-seed leg (test_gpu_casts.py test_fixed_seed_fuzz) through tests/fuzz_explore_leg.py, which says how it is seeded, replayed
(C2D_FUZZ_SEED / C2D_FUZZ_INDEX with this file) and traced ($C2D_FUZZ_TRACE_DIR/casts.txt).  Over its run the leg must have compared
a query with a winner and one without."""
import pytest

import fuzz_explore_leg

pytestmark = pytest.mark.gpu

LEG, LEG_INDEX = "casts", 17      # (the seed offset continues the table of tests/test_gpu_fuzz_explore.py)
TOOL = "cast_fuzz"
PROOF = {"hits": ("hits",), "misses": ("misses",)}      # what the run must have compared: wording -> keys of the tool's LAST


def test_cast_differential_fuzz_at_this_commits_seed(eng, oracle, wl, capsys):   # (`oracle`: sizes the OpenMP team to the box's CPU share)
    fuzz_explore_leg.run(eng, wl, capsys, LEG, LEG_INDEX, TOOL, PROOF, takes_wl=True)
