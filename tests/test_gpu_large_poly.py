"""Maximum sizes of the polygon entry points: planes and offsets past 4 GiB in every padded-layout kernel, the one-bin limit of
c2d_sat_poly_pairs_rows from both sides, more than 2^24 tiles in one launch and more than 2^25 in one binned batch, the largest
plane of a caller's bin, and c2d_poly_bins_from_padded on both sides of 16 GiB and with classes above the 4 GiB plane limit.
The work is in tests/large_poly_check.py, run in its own process because it builds its inputs with torch (which has to be
imported before libc2d.so)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def test_polygon_maximum_sizes():
    out = subprocess.run([sys.executable, os.path.join(HERE, "large_poly_check.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "large poly ok" in out.stdout
