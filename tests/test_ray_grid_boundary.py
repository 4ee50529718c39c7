"""CPU tests of c2d_poly_ray_casts_grid at the C-ABI boundary, after tests/test_ray_boundary.py: the header declares the entry and states
its contract, every shipped build exports the symbol, the Python mirror types it, and argument errors come back as statuses.  No
compute entry point reaches a device here."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

PKG_DIR = os.path.join(ROOT, "convex-2d-gpu-collision-detection_amd")
SYMBOLS = ("c2d_poly_ray_casts_grid", "c2d_poly_ray_casts_grid_stats")
BUILDS = [os.path.join(PKG_DIR, "lib", n) for n in ("libc2d.so", "libc2d_fmad1.so", "libc2d_fmad2.so", "libc2d_nopretest.so",
                                                    "libc2d_movecheck.so", "libc2d_splitcheck.so")]
BUILDS.append(os.path.join(PKG_DIR, "lib-rehearsal", "libc2d.so"))


def test_header_declares_the_entry_point_and_states_the_contract():
    raw = open(os.path.join(ROOT, "include", "c2d.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bint\s+c2d_poly_ray_casts_grid\s*\(\s*c2d_ctx\s*\*\s*\w*\s*,\s*const\s+float\s*\*\s*const\s+d_rays\s*\[\s*4\s*\]\s*,\s*size_t\s+n_rays\s*,"
                     r"\s*const\s+c2d_poly_set\s*\*\s*b\s*,\s*size_t\s+col_base\s*,\s*c2d_ray_hit\s*\*\s*d_out\s*,\s*c2d_stream\s+stream\s*\)", text)
    assert re.search(r"\bint\s+c2d_poly_ray_casts_grid_stats\s*\(\s*c2d_ctx\s*\*\s*\w*\s*,\s*unsigned\s+long\s+long\s+out\s*\[\s*4\s*\]\s*\)", text)
    # the contract: the box, meets step by step, the restricted pick, the relation to the brute-force call, the scratch
    assert re.search(r"UNBOXED.*?bx = ox \+ dx.*?m  = 2\^-20 \* C.*?sx = min\(ox, bx\) > xh \+ m \|\| max\(ox, bx\) < xl - m.*?"
                     r"hx = \(0\.5 \* xh - 0\.5 \* xl\) \+ m.*?sn = \|dx \* \(cy - oy\) - dy \* \(cx - ox\)\| > hx \* \|dy\| \+ hy \* \|dx\|.*?"
                     r"meets = !\(sx \|\| sy \|\| sn\).*?restricted to \{ j : unboxed\(j\) \|\| meets\(r, j\) \}.*?NOT equal for every bit pattern.*?"
                     r"uses the ctx scratch.*?capture that would have to grow the scratch is refused", raw, flags=re.S)
    assert "c2d_version() stays 6" in raw


@pytest.mark.parametrize("path", BUILDS, ids=lambda p: os.path.relpath(p, PKG_DIR))
def test_every_build_exports_the_symbols(pkg, path):
    assert os.path.exists(path), path
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for symbol in SYMBOLS:
        assert symbol in names, f"{os.path.basename(path)} does not export {symbol}"


def test_mirror_types_the_symbols(pkg):
    from c2d_amd import binding

    lib = pkg.load_library()
    assert lib.c2d_version() == 6
    for symbol in SYMBOLS:
        assert symbol in binding.EXPORTED_SYMBOLS
        res, args = binding._SIGNATURES[symbol]
        assert res is C.c_int and getattr(lib, symbol).argtypes == args
    # the same arguments as the brute-force call
    assert binding._SIGNATURES[SYMBOLS[0]] == binding._SIGNATURES["c2d_poly_ray_casts"]
    assert binding._SIGNATURES[SYMBOLS[1]][1] == [C.c_void_p, C.POINTER(C.c_ulonglong)]


def test_null_and_bad_arguments_are_rejected_without_a_device(pkg):
    from c2d_amd import binding

    lib = pkg.load_library()
    s = binding._PolySet(16, 10, 0, 0x1000, 0x1000, 0x1000)
    planes = (C.c_void_p * 4)(*[0x1000] * 4)
    o = C.c_void_p(0x2000)
    cast = lib.c2d_poly_ray_casts_grid
    # no ctx: refused whatever else is passed
    assert cast(None, planes, 4, C.byref(s), 0, o, None) == -1
    assert cast(None, None, 0, None, 0, None, None) == -1
    assert cast(None, planes, 4, C.byref(s), 0, C.c_void_p(0x2008), None) == -1                      # (a misaligned output too)
    assert cast(None, planes, 4, C.byref(binding._PolySet(17, 10, 0, 0x1000, 0x1000, 0x1000)), 0, o, None) == -1   # (rows out of range)
    assert cast(None, planes, 4, C.byref(s), (1 << 32) - 9, o, None) == -1                           # (col_base + n_b > 2^32)
    assert cast(None, planes, (1 << 32) + 1, C.byref(s), 0, o, None) == -1                           # (n_rays > 2^32)
    assert lib.c2d_poly_ray_casts_grid_stats(None, (C.c_ulonglong * 4)()) == -1
    assert lib.c2d_poly_ray_casts_grid_stats(None, None) == -1
    # (with a ctx, every refusal is checked on the GPU, where a ctx can be made: tests/test_gpu_ray_casts_grid.py::test_argument_errors)


def test_method_checks_its_shapes_before_touching_a_device(pkg):
    eng = object.__new__(pkg.Engine)   # no ctx: the shape checks come first
    with pytest.raises(ValueError):
        pkg.Engine.poly_ray_casts_grid(eng, None, 0, None, 0)
    with pytest.raises(ValueError):
        pkg.Engine.poly_ray_casts_grid(eng, [0] * 3, 1, pkg.binding._PolySet(), 0)
    with pytest.raises(ValueError):
        pkg.Engine.poly_ray_casts_grid(eng, [0] * 4, 1, None, 0)
