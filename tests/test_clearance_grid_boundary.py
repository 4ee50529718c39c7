"""CPU tests of c2d_poly_set_clearances_grid at the C-ABI boundary, after tests/test_near_broad_boundary.py: the header declares the
entry and states its contract through the clearance and the proximity contracts, every shipped build exports the symbol, the Python
mirror types it, argument errors come back as statuses and the Python method checks its shapes first.  No compute entry point reaches
a device here."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "convex-2d-gpu-collision-detection_amd")
SYMBOL = "c2d_poly_set_clearances_grid"
STATS = "c2d_poly_set_clearances_grid_stats"
BUILDS = [os.path.join(PKG_DIR, "lib", n) for n in ("libc2d.so", "libc2d_fmad1.so", "libc2d_fmad2.so", "libc2d_nopretest.so",
                                                    "libc2d_movecheck.so", "libc2d_splitcheck.so")]
BUILDS.append(os.path.join(PKG_DIR, "lib-rehearsal", "libc2d.so"))


def test_header_declares_the_entry_point_and_its_contract():
    raw = open(os.path.join(ROOT, "include", "c2d.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bint\s+c2d_poly_set_clearances_grid\s*\(\s*c2d_ctx\s*\*\s*\w*\s*,\s*const\s+c2d_poly_set\s*\*\s*a\s*,\s*const\s+c2d_poly_set\s*\*\s*b"
                     r"\s*,\s*float\s+max_dist\s*,\s*size_t\s+row_base\s*,\s*size_t\s+col_base\s*,\s*int\s+flags\s*,\s*c2d_clearance\s*\*\s*d_out\s*,"
                     r"\s*c2d_stream\s+stream\s*\)", text)
    assert raw.index("---- proximity pair search") < raw.index("---- clearance queries through a grid") < raw.index("int c2d_poly_set_clearances_grid") \
        < raw.index("---- binned polygon batches")
    assert re.search(r"contract of c2d_poly_set_clearances.*?word for word.*?one more clause.*?considered.*?vertex count is within 1\.\.rows"
                     r".*?row_base \+ i == col_base \+ j.*?D\(i, j\)\.hit == 1 \|\| D\(i, j\)\.dist <= max_dist.*?binary32 compare of c2d_poly_near_broad_pairs"
                     r".*?every input bit pattern.*?C2D_DISTANCE_NO_CANDIDATE.*?considered only when it is hit.*?smallest key \(bits of D\(i, j\)\.dist, col_base \+ j\)"
                     r".*?smaller index.*?C2D_CLEARANCE_NONE.*?nothing within max_dist.*?C2D_DISTANCE_BAD_PAIR", raw, flags=re.S)
    # the three consequences
    assert re.search(r"poly is not 0xFFFFFFFF has hit == 1 \|\| dist <= max_dist.*?exactly when row i of the list of c2d_poly_near_broad_pairs is empty"
                     r".*?self pair removed.*?every query of a call has a winner.*?byte for byte that of c2d_poly_set_clearances", raw, flags=re.S)
    assert re.search(r"0 <= max_dist < 2\^60; -0 counts as 0.*?NaN included.*?before the sets are looked at.*?n_a == 0 is a no-op; n_b == 0 writes the NONE record"
                     r".*?n_a or n_b above 2\^32.*?C2D_ASYNC_ERR_POLY_K.*?DESIGN\.md §5\.21.*?no host synchronisation.*?workspace guard"
                     r".*?size is that of\s+\*?\s*c2d_sat_poly_broad_pairs.*?Graph capture.*?refused", raw, flags=re.S)
    assert "c2d_version() stays 6" in raw
    assert re.search(r"\bint\s+c2d_poly_set_clearances_grid_stats\s*\(\s*c2d_ctx\s*\*\s*\w*\s*,\s*unsigned\s+long\s+long\s+out\s*\[\s*5\s*\]\s*\)", text)


@pytest.mark.parametrize("path", BUILDS, ids=lambda p: os.path.relpath(p, PKG_DIR))
def test_every_build_exports_the_symbol(pkg, path):
    assert os.path.exists(path), path
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert SYMBOL in names, f"{os.path.basename(path)} does not export {SYMBOL}"
    assert STATS in names, f"{os.path.basename(path)} does not export {STATS}"


def test_mirror_types_the_symbol(pkg):
    from c2d_amd import binding

    lib = pkg.load_library()
    assert lib.c2d_version() == 6
    assert SYMBOL in binding.EXPORTED_SYMBOLS
    res, args = binding._SIGNATURES[SYMBOL]
    assert res is C.c_int and getattr(lib, SYMBOL).argtypes == args
    assert args == [C.c_void_p, C.POINTER(binding._PolySet), C.POINTER(binding._PolySet), C.c_float, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    assert list(inspect.signature(pkg.Engine.poly_set_clearances_grid).parameters)[1:] == ["a_set", "b_set", "max_dist", "d_out", "row_base", "col_base",
                                                                                            "flags", "stream"]
    sig = inspect.signature(pkg.Engine.poly_set_clearances_grid).parameters
    assert [sig[p].default for p in ("row_base", "col_base", "flags", "stream")] == [0, 0, 0, 0]
    assert STATS in binding.EXPORTED_SYMBOLS and binding._SIGNATURES[STATS] == (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong)])
    assert lib.c2d_poly_set_clearances_grid_stats(None, (C.c_ulonglong * 5)()) == -1


def test_null_and_bad_arguments_are_rejected_without_a_device(pkg):
    """Without a ctx the entry returns at its first check, whatever else is passed: a ctx needs a device, so the order of the refusals
    behind it (max_dist before the sets, then NULLs, the sets, the alignment of d_out, the flag, the bases) and their messages are
    exercised with a live ctx in tests/test_gpu_clearances_grid.py::test_argument_errors, which also checks that nothing was written."""
    from c2d_amd import binding

    lib = pkg.load_library()
    s = binding._PolySet(16, 10, 0, 0x1000, 0x1000, 0x1000)
    o = C.c_void_p(0x2000)
    fn = lib.c2d_poly_set_clearances_grid
    assert fn(None, C.byref(s), C.byref(s), 1.0, 0, 0, 0, o, None) == -1
    assert fn(None, None, None, 1.0, 0, 0, 0, None, None) == -1
    for bad in (float("nan"), float("inf"), -1.0, 2.0 ** 60):
        assert fn(None, C.byref(s), C.byref(s), bad, 0, 0, 0, o, None) == -1                                   # (a bad max_dist)
    assert fn(None, C.byref(s), C.byref(s), 1.0, 0, 0, 2, o, None) == -1                                       # (an unknown flag)
    assert fn(None, C.byref(s), C.byref(s), 1.0, 0, 0, 0, C.c_void_p(0x2008), None) == -1                      # (a misaligned output)
    assert fn(None, C.byref(s), C.byref(s), 1.0, (1 << 32) - 9, 0, 0, o, None) == -1                           # (row_base + n_a > 2^32)
    assert fn(None, C.byref(binding._PolySet(16, (1 << 32) + 1, 0, 0x1000, 0x1000, 0x1000)), C.byref(s), 1.0, 0, 0, 0, o, None) == -1   # (n_a > 2^32)


def test_method_checks_its_shapes_before_touching_a_device(pkg):
    eng = object.__new__(pkg.Engine)   # no ctx: the shape checks come first
    s = pkg.binding._PolySet(16, 10, 0, 0x1000, 0x1000, 0)
    call = pkg.Engine.poly_set_clearances_grid
    with pytest.raises(ValueError):
        call(eng, None, s, 1.0, 0x2000)
    with pytest.raises(ValueError):
        call(eng, s, [0] * 3, 1.0, 0x2000)
    with pytest.raises(ValueError):
        call(eng, s, s, 1.0, None)
    with pytest.raises(ValueError):
        call(eng, s, s, 1.0, 0x2000, flags=2)
    with pytest.raises(ValueError):
        call(eng, s, s, 1.0, 0x2000, row_base=-1)
    with pytest.raises(ValueError):
        call(eng, s, s, 1.0, 0x2000, col_base=-1)
    with pytest.raises(ValueError):
        call(eng, s, s, 1.0, pkg.DeviceArray(eng, 0x2000, (9,), pkg.CLEARANCE_DT))   # fewer than n_a records
    assert pkg.CLEARANCE_DT.itemsize == 32
    assert np.dtype(pkg.CLEARANCE_DT).names[0] == "poly"
