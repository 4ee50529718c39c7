"""CPU tests of c2d_poly_set_casts_grid at the C-ABI boundary, after tests/test_clearance_grid_boundary.py and
tests/test_cast_boundary.py: the header declares the entry and its stats call and states the contract by reference to
c2d_poly_set_casts, every shipped build exports both symbols, the Python mirror types them, argument errors come back as statuses
and the Python method checks its shapes first.  No compute entry point reaches a device here."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "convex-2d-gpu-collision-detection_amd")
SYMBOL = "c2d_poly_set_casts_grid"
STATS = "c2d_poly_set_casts_grid_stats"
BUILDS = [os.path.join(PKG_DIR, "lib", n) for n in ("libc2d.so", "libc2d_fmad1.so", "libc2d_fmad2.so", "libc2d_nopretest.so",
                                                    "libc2d_movecheck.so", "libc2d_splitcheck.so")]
BUILDS.append(os.path.join(PKG_DIR, "lib-rehearsal", "libc2d.so"))


def test_header_declares_the_entry_point_and_its_contract():
    raw = open(os.path.join(ROOT, "include", "c2d.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    ptr = r"\s*,\s*const\s+float\s*\*\s*"
    assert re.search(r"\bint\s+c2d_poly_set_casts_grid\s*\(\s*c2d_ctx\s*\*\s*\w*\s*,\s*const\s+c2d_poly_set\s*\*\s*a\s*,\s*const\s+c2d_poly_set\s*\*\s*b"
                     + ptr + "d_a_dx" + ptr + "d_a_dy" + ptr + "d_b_dx" + ptr + "d_b_dy"
                     + r"\s*,\s*size_t\s+row_base\s*,\s*size_t\s+col_base\s*,\s*int\s+flags\s*,\s*c2d_cast\s*\*\s*d_out\s*,\s*c2d_stream\s+stream\s*\)", text)
    assert re.search(r"\bint\s+c2d_poly_set_casts_grid_stats\s*\(\s*c2d_ctx\s*\*\s*\w*\s*,\s*unsigned\s+long\s+long\s+out\s*\[\s*5\s*\]\s*\)", text)
    assert raw.index("---- clearance queries through a grid") < raw.index("---- shape casts through a grid") < raw.index("int c2d_poly_set_casts_grid") \
        < raw.index("---- binned polygon batches")
    section = raw[raw.index("---- shape casts through a grid"):raw.index("---- binned polygon batches")]
    # the contract by reference, and its consequence
    assert re.search(r"contract of c2d_poly_set_casts, word for word.*?considered.*?key \(bits of S\(i, j\)\.toi, col_base \+ j\).*?miss record"
                     r".*?C2D_SWEEP_BAD_PAIR.*?C2D_CAST_SKIP_SELF.*?C2D_ASYNC_ERR_POLY_K.*?the two calls write the same bytes.*?every input bit pattern"
                     r".*?DESIGN\.md §5\.19.*?DESIGN\.md §5\.22", section, flags=re.S)
    assert re.search(r"same\s+\*?\s*memory.*?AND the same motion planes.*?different motion planes is two sets", section, flags=re.S)
    assert re.search(r"order of c2d_poly_set_casts, half a motion first.*?n_a == 0 is a no-op; n_b == 0 writes the miss\s+\*?\s*record.*?without touching the ctx scratch"
                     r".*?8-byte aligned.*?n_a or n_b above 2\^32.*?no host synchronisation.*?deterministic.*?workspace guard.*?Graph capture.*?refused",
                     section, flags=re.S)
    assert re.search(r"last grid call on the ctx was not a grid cast.*?out\[0\] = queries answered by the list kernel.*?out\[1\] = sorted grid\s+\*?\s*entries"
                     r".*?out\[2\] = candidates.*?out\[3\] = .*?axis walk", section, flags=re.S)
    assert "c2d_version() stays 6" in section


@pytest.mark.parametrize("path", BUILDS, ids=lambda p: os.path.relpath(p, PKG_DIR))
def test_every_build_exports_the_symbols(pkg, path):
    assert os.path.exists(path), path
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert SYMBOL in names, f"{os.path.basename(path)} does not export {SYMBOL}"
    assert STATS in names, f"{os.path.basename(path)} does not export {STATS}"


def test_mirror_types_the_symbols(pkg):
    from c2d_amd import binding

    lib = pkg.load_library()
    assert lib.c2d_version() == 6
    assert SYMBOL in binding.EXPORTED_SYMBOLS and STATS in binding.EXPORTED_SYMBOLS
    res, args = binding._SIGNATURES[SYMBOL]
    assert res is C.c_int and getattr(lib, SYMBOL).argtypes == args
    assert (res, args) == binding._SIGNATURES["c2d_poly_set_casts"], "the two calls take the same arguments"
    assert args == [C.c_void_p, C.POINTER(binding._PolySet), C.POINTER(binding._PolySet)] + [C.c_void_p] * 4 + [C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
    assert binding._SIGNATURES[STATS] == (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong)])
    grid, full = (inspect.signature(getattr(pkg.Engine, m)).parameters for m in ("poly_set_casts_grid", "poly_set_casts"))
    assert list(grid) == list(full) == ["self", "a_set", "b_set", "a_motion", "b_motion", "row_base", "col_base", "flags", "out", "stream"]
    assert [grid[p].default for p in list(grid)[3:]] == [full[p].default for p in list(full)[3:]] == [None, None, 0, 0, 0, None, 0]
    assert list(inspect.signature(pkg.Engine.poly_set_casts_grid_stats).parameters) == ["self"]


def test_stats_before_any_call(pkg):
    lib = pkg.load_library()
    out = (C.c_ulonglong * 5)(7, 7, 7, 7, 7)
    assert lib.c2d_poly_set_casts_grid_stats(None, out) == -1
    assert lib.c2d_poly_set_casts_grid_stats(None, None) == -1
    assert list(out) == [7] * 5, "a refused stats call wrote something"
    # (with a ctx that has run no grid call, or another grid call last: tests/test_gpu_casts_grid.py::test_the_counters)


def test_null_and_bad_arguments_are_rejected_without_a_device(pkg):
    """Without a ctx the entry returns at its first check (the motion check, which looks at the ctx first), whatever else is passed;
    the order of the refusals behind it and their messages are exercised with a live ctx in
    tests/test_gpu_casts_grid.py::test_argument_errors, which also checks that nothing was written."""
    from c2d_amd import binding

    lib = pkg.load_library()
    s = binding._PolySet(16, 10, 0, 0x1000, 0x1000, 0x1000)
    o, m = C.c_void_p(0x2000), C.c_void_p(0x3000)
    fn = lib.c2d_poly_set_casts_grid
    none = (None, None, None, None)
    assert fn(None, C.byref(s), C.byref(s), *none, 0, 0, 0, o, None) == -1
    assert fn(None, None, None, *none, 0, 0, 0, None, None) == -1                                                # (NULLs)
    assert fn(None, C.byref(s), C.byref(s), m, m, m, m, 0, 0, 0, o, None) == -1
    for half in ((m, None, None, None), (None, m, None, None), (None, None, m, None), (m, m, None, m)):
        assert fn(None, C.byref(s), C.byref(s), *half, 0, 0, 0, o, None) == -1                                   # (half a motion)
        assert fn(None, None, None, *half, 0, 0, 7, None, None) == -1                                            # (half a motion first)
    assert fn(None, C.byref(s), C.byref(s), None, None, m, C.c_void_p(0x3002), 0, 0, 0, o, None) == -1           # (a misaligned motion plane)
    assert fn(None, C.byref(s), C.byref(s), *none, 0, 0, 0, C.c_void_p(0x2004), None) == -1                      # (a misaligned output)
    for rows in (0, 17):
        assert fn(None, C.byref(binding._PolySet(rows, 10, 0, 0x1000, 0x1000, 0x1000)), C.byref(s), *none, 0, 0, 0, o, None) == -1   # (rows)
        assert fn(None, C.byref(s), C.byref(binding._PolySet(rows, 0, 0, 0, 0, 0)), *none, 0, 0, 0, o, None) == -1                    # (of an empty b too)
    assert fn(None, C.byref(binding._PolySet(16, 10, 0, 0x1002, 0x1000, 0x1000)), C.byref(s), *none, 0, 0, 0, o, None) == -1         # (a misaligned plane)
    assert fn(None, C.byref(binding._PolySet(16, 10, 9, 0x1000, 0x1000, 0x1000)), C.byref(s), *none, 0, 0, 0, o, None) == -1         # (stride < n)
    for flags in (2, 4, -1):
        assert fn(None, C.byref(s), C.byref(s), *none, 0, 0, flags, o, None) == -1                               # (an unknown flag)
    assert fn(None, C.byref(s), C.byref(s), *none, (1 << 32) - 9, 0, 0, o, None) == -1                           # (row_base + n_a > 2^32)
    assert fn(None, C.byref(s), C.byref(s), *none, 0, (1 << 32) - 9, 0, o, None) == -1                           # (col_base + n_b > 2^32)
    assert fn(None, C.byref(s), C.byref(s), *none, (1 << 32) + 1, 0, 0, o, None) == -1                           # (a base above 2^32)
    big = binding._PolySet(16, (1 << 32) + 1, 0, 0x1000, 0x1000, 0x1000)
    assert fn(None, C.byref(big), C.byref(s), *none, 0, 0, 0, o, None) == -1                                     # (n_a > 2^32)
    assert fn(None, C.byref(s), C.byref(big), *none, 0, 0, 0, o, None) == -1                                     # (n_b > 2^32)


def test_method_checks_its_shapes_before_touching_a_device(pkg):
    eng = object.__new__(pkg.Engine)   # no ctx: the shape checks come first
    s = pkg.binding._PolySet(16, 10, 0, 0x1000, 0x1000, 0)
    cast = pkg.Engine.poly_set_casts_grid
    with pytest.raises(ValueError):
        cast(eng, None, s, out=0x2000)
    with pytest.raises(ValueError):
        cast(eng, s, [0] * 3, out=0x2000)
    with pytest.raises(ValueError):
        cast(eng, s, s)                                      # no output
    with pytest.raises(ValueError):
        cast(eng, s, s, flags=2, out=0x2000)
    with pytest.raises(ValueError):
        cast(eng, s, s, row_base=-1, out=0x2000)
    with pytest.raises(ValueError):
        cast(eng, s, s, col_base=-1, out=0x2000)
    with pytest.raises(ValueError):
        cast(eng, s, s, a_motion=(0x3000,), out=0x2000)      # a motion is None or two planes
    with pytest.raises(ValueError):
        cast(eng, s, s, b_motion=(0x3000, None), out=0x2000)
    with pytest.raises(ValueError):
        cast(eng, s, s, out=pkg.DeviceArray(eng, 0x2000, (9,), pkg.CAST_DT))   # fewer than n_a records
