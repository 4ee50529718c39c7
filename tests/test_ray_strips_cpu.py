"""How a ray query deals the column tiles of B to the grid (csrc/c2d_ray_strips.hpp), checked on a CPU by tests/cpp/test_ray_strips.cpp:
one strip when B fits one tile, at least two for one row tile against two or more column tiles, never more strips than column
tiles, and every column tile in exactly one strip.  The program is built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_strip_rule(tmp_path):
    exe = str(tmp_path / "test_ray_strips")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "convex-2d-gpu-collision-detection_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_ray_strips.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
