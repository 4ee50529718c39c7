"""CPU tests of c2d_poly_sweep_broad_pairs at the C-ABI boundary, after tests/test_cast_boundary.py: the header declares the entry and
states its contract through the sweep contract, every shipped build exports the symbol, the Python mirror types it, and argument
errors come back as statuses.  No compute entry point reaches a device here."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "convex-2d-gpu-collision-detection_amd")
SYMBOL = "c2d_poly_sweep_broad_pairs"
BUILDS = [os.path.join(PKG_DIR, "lib", n) for n in ("libc2d.so", "libc2d_fmad1.so", "libc2d_fmad2.so", "libc2d_nopretest.so",
                                                    "libc2d_movecheck.so", "libc2d_splitcheck.so")]
BUILDS.append(os.path.join(PKG_DIR, "lib-rehearsal", "libc2d.so"))


def test_header_declares_the_entry_point_and_its_contract():
    raw = open(os.path.join(ROOT, "include", "c2d.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    ptr = r"\s*,\s*const\s+float\s*\*\s*"
    assert re.search(r"\bint\s+c2d_poly_sweep_broad_pairs\s*\(\s*c2d_ctx\s*\*\s*\w*\s*,\s*const\s+c2d_poly_set\s*\*\s*a\s*,\s*const\s+c2d_poly_set\s*\*\s*b"
                     + ptr + "d_a_dx" + ptr + "d_a_dy" + ptr + "d_b_dx" + ptr + "d_b_dy"
                     + r"\s*,\s*int\s+flags\s*,\s*uint32_t\s*\*\s*d_pairs\s*,\s*size_t\s+capacity\s*,\s*unsigned\s+long\s+long\s*\*\s*d_count\s*,"
                     r"\s*c2d_stream\s+stream\s*\)", text)
    assert raw.index("---- shape casts") < raw.index("---- swept broad-phase pair search") < raw.index("int c2d_poly_sweep_broad_pairs")
    assert re.search(r"S\(i, j\) is the c2d_sweep record that c2d_poly_pair_sweeps defines.*?row_base = col_base = 0.*?S\(i, j\)\.hit == 1"
                     r".*?every input bit pattern.*?outside 1\.\.rows is in no pair.*?C2D_CROSS_UPPER.*?DESIGN\.md §5\.19.*?AND the same motion planes"
                     r".*?The chain.*?no host synchronisation.*?d_n_pairs = d_count.*?half a motion", raw, flags=re.S)
    assert "c2d_version() stays 6" in raw


@pytest.mark.parametrize("path", BUILDS, ids=lambda p: os.path.relpath(p, PKG_DIR))
def test_every_build_exports_the_symbol(pkg, path):
    assert os.path.exists(path), path
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert SYMBOL in names, f"{os.path.basename(path)} does not export {SYMBOL}"


def test_mirror_types_the_symbol(pkg):
    from c2d_amd import binding

    lib = pkg.load_library()
    assert lib.c2d_version() == 6
    assert SYMBOL in binding.EXPORTED_SYMBOLS
    res, args = binding._SIGNATURES[SYMBOL]
    assert res is C.c_int and getattr(lib, SYMBOL).argtypes == args
    assert args == [C.c_void_p, C.POINTER(binding._PolySet), C.POINTER(binding._PolySet)] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    assert list(inspect.signature(pkg.Engine.poly_sweep_broad_pairs).parameters)[1:] == ["a", "b", "pairs", "capacity", "count", "a_motion", "b_motion", "upper",
                                                                                         "stream"]
    assert list(inspect.signature(pkg.Engine.poly_sweep_broad_pairs_host).parameters)[1:] == ["vx_a", "vy_a", "k_a", "a_motion", "vx_b", "vy_b", "k_b", "b_motion",
                                                                                              "upper"]


def test_null_and_bad_arguments_are_rejected_without_a_device(pkg):
    from c2d_amd import binding

    lib = pkg.load_library()
    s = binding._PolySet(16, 10, 0, 0x1000, 0x1000, 0x1000)
    p, c, m = C.c_void_p(0x2000), C.c_void_p(0x4000), C.c_void_p(0x3000)
    fn = lib.c2d_poly_sweep_broad_pairs
    # no ctx: refused whatever else is passed
    assert fn(None, C.byref(s), C.byref(s), None, None, None, None, 0, p, 16, c, None) == -1
    assert fn(None, None, None, None, None, None, None, 0, None, 0, None, None) == -1
    assert fn(None, C.byref(s), C.byref(s), m, m, m, m, 0, p, 16, c, None) == -1
    assert fn(None, C.byref(s), C.byref(s), m, None, None, None, 0, p, 16, c, None) == -1                      # (half a motion)
    assert fn(None, C.byref(s), C.byref(s), None, None, m, C.c_void_p(0x3002), 0, p, 16, c, None) == -1        # (a misaligned motion plane)
    assert fn(None, C.byref(s), C.byref(s), None, None, None, None, 2, p, 16, c, None) == -1                   # (an unknown flag)
    # (with a ctx, every refusal is checked on the GPU, where a ctx can be made: tests/test_gpu_sweep_broad.py::test_argument_errors)


def test_methods_check_their_shapes_before_touching_a_device(pkg):
    eng = object.__new__(pkg.Engine)   # no ctx: the shape checks come first
    s = pkg.binding._PolySet(16, 10, 0, 0x1000, 0x1000, 0)
    call = pkg.Engine.poly_sweep_broad_pairs
    with pytest.raises(ValueError):
        call(eng, None, s, 0x2000, 16, 0x4000)
    with pytest.raises(ValueError):
        call(eng, s, [0] * 3, 0x2000, 16, 0x4000)
    with pytest.raises(ValueError):
        call(eng, s, s, 0x2000, 16, 0x4000, a_motion=(0x3000,))            # a motion is None or two planes
    with pytest.raises(ValueError):
        call(eng, s, s, 0x2000, 16, 0x4000, b_motion=(0x3000, None))
    host = pkg.Engine.poly_sweep_broad_pairs_host
    vx = np.zeros((4, 10), np.float32)
    with pytest.raises(ValueError):
        host(eng, vx, vx[:, :9], None)                                      # planes of two shapes
    with pytest.raises(ValueError):
        host(eng, vx, vx, None, a_motion=(np.zeros(10, np.float32),))       # a motion is two planes
    with pytest.raises(ValueError):
        host(eng, vx, vx, None, a_motion=(np.zeros(9, np.float32), np.zeros(9, np.float32)))
    with pytest.raises(ValueError):
        host(eng, vx, vx, None, b_motion=(np.zeros(10, np.float32), np.zeros(10, np.float32)))   # a motion of B without a set B
    with pytest.raises(ValueError):
        host(eng, vx, vx, None, vx_b=vx)                                    # vx_b without vy_b
    assert host(eng, vx[:, :0], vx[:, :0], None).shape == (0, 2)            # an empty set: no device needed
