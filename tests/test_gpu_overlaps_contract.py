"""What every list-driven query promises of its list (csrc/c2d_pair_list.hpp: `listed_pairs`, the host checks), for the overlap
queries: the tests of tests/test_gpu_pair_list_contract.py themselves, called with the row of tests/overlap_query.py, and the graph
check in a script of its own (tests/overlap_graph_check.py: the shared one resolves its query from pair_list_harness.QUERIES)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import test_gpu_pair_list_contract as contract  # noqa: E402
from overlap_query import OVERLAPS  # noqa: E402

pytestmark = pytest.mark.gpu


def test_device_count_bounds_the_work(eng, wl):
    contract.test_device_count_bounds_the_work(eng, wl, OVERLAPS)


def test_bad_pairs_read_nothing_and_are_reported_once(eng, wl):
    contract.test_bad_pairs_read_nothing_and_are_reported_once(eng, wl, OVERLAPS)


def test_argument_errors(eng, pkg, wl):
    contract.test_argument_errors(eng, pkg, wl, OVERLAPS)


def test_graph_capture_follows_the_device_count():
    """One capture of c2d_poly_pair_overlaps with d_n_pairs, replayed with different counts written to the device in between."""
    out = subprocess.run([sys.executable, os.path.join(HERE, "overlap_graph_check.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "overlaps graph ok" in out.stdout
