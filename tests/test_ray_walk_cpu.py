"""The cell-range enumeration of the grid ray query (csrc/c2d_ray_walk.hpp) and its candidate predicate, checked on a CPU by
tests/cpp/test_ray_walk.cpp: on random grids (single cells, clamped edges, the 65 535-cell cap) and random segments (points,
axis-parallel, many cells long, end points on cell borders, outside the bounds), the key of every regular box that the ray meets lies
in an enumerated range, and the enumeration stays within 5 T + 9 cells of the T cells the widened segment truly crosses.  The program
is built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_walk_enumeration(tmp_path):
    exe = str(tmp_path / "test_ray_walk")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "convex-2d-gpu-collision-detection_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "test_ray_walk.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok:"), r.stdout + r.stderr
