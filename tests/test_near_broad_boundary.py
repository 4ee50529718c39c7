"""CPU tests of c2d_poly_near_broad_pairs at the C-ABI boundary, after tests/test_sweep_broad_boundary.py: the header declares the entry
and states its contract through the distance contract, every shipped build exports the symbol, the Python mirror types it, a NULL
ctx comes back as a status and the Python methods check their shapes first.  No compute entry point reaches a device here."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "convex-2d-gpu-collision-detection_amd")
SYMBOL = "c2d_poly_near_broad_pairs"
BUILDS = [os.path.join(PKG_DIR, "lib", n) for n in ("libc2d.so", "libc2d_fmad1.so", "libc2d_fmad2.so", "libc2d_nopretest.so",
                                                    "libc2d_movecheck.so", "libc2d_splitcheck.so")]
BUILDS.append(os.path.join(PKG_DIR, "lib-rehearsal", "libc2d.so"))


def test_header_declares_the_entry_point_and_its_contract():
    raw = open(os.path.join(ROOT, "include", "c2d.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bint\s+c2d_poly_near_broad_pairs\s*\(\s*c2d_ctx\s*\*\s*\w*\s*,\s*const\s+c2d_poly_set\s*\*\s*a\s*,\s*const\s+c2d_poly_set\s*\*\s*b"
                     r"\s*,\s*float\s+max_dist\s*,\s*int\s+flags\s*,\s*uint32_t\s*\*\s*d_pairs\s*,\s*size_t\s+capacity\s*,"
                     r"\s*unsigned\s+long\s+long\s*\*\s*d_count\s*,\s*c2d_stream\s+stream\s*\)", text)
    assert raw.index("---- swept broad-phase pair search") < raw.index("---- proximity pair search") < raw.index("int c2d_poly_near_broad_pairs")
    assert re.search(r"D\(i, j\) is the c2d_distance record that c2d_poly_pair_distances defines.*?row_base = col_base = 0"
                     r".*?D\(i, j\)\.hit == 1 \|\| D\(i, j\)\.dist <= max_dist.*?binary32 compare.*?every input bit pattern"
                     r".*?dist = \+inf\) is listed only when it is hit.*?outside 1\.\.rows is\s+\*?\s*in no pair.*?C2D_CROSS_UPPER"
                     r".*?superset.*?contains the list of c2d_sat_poly_broad_pairs.*?monotone.*?the chain.*?no host synchronisation"
                     r".*?d_n_pairs = d_count.*?DESIGN\.md §5\.20.*?0 <= max_dist < 2\^60; -0 counts as 0.*?NaN included", raw, flags=re.S)
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
    assert args == [C.c_void_p, C.POINTER(binding._PolySet), C.POINTER(binding._PolySet), C.c_float, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    assert list(inspect.signature(pkg.Engine.poly_near_broad_pairs).parameters)[1:] == ["a", "b", "max_dist", "pairs", "capacity", "count", "upper", "stream"]
    assert list(inspect.signature(pkg.Engine.poly_near_broad_pairs_host).parameters)[1:] == ["vx_a", "vy_a", "k_a", "max_dist", "vx_b", "vy_b", "k_b", "upper"]


def test_a_null_ctx_is_refused_without_a_device(pkg):
    """Without a ctx the entry returns at its first check, so this says nothing about max_dist, the flags or the sets: a ctx needs a
    device, and those refusals (a negative, NaN, infinite and >= 2^60 max_dist, an unknown flag, NULL sets) are exercised with a live
    ctx in tests/test_gpu_near_broad.py::test_argument_errors, which also checks that they are made before a kernel runs."""
    from c2d_amd import binding

    lib = pkg.load_library()
    s = binding._PolySet(16, 10, 0, 0x1000, 0x1000, 0x1000)
    fn = lib.c2d_poly_near_broad_pairs
    assert fn(None, C.byref(s), C.byref(s), 1.0, 0, C.c_void_p(0x2000), 16, C.c_void_p(0x4000), None) == -1
    assert fn(None, None, None, 1.0, 0, None, 0, None, None) == -1


def test_methods_check_their_shapes_before_touching_a_device(pkg):
    eng = object.__new__(pkg.Engine)   # no ctx: the shape checks come first
    s = pkg.binding._PolySet(16, 10, 0, 0x1000, 0x1000, 0)
    call = pkg.Engine.poly_near_broad_pairs
    with pytest.raises(ValueError):
        call(eng, None, s, 1.0, 0x2000, 16, 0x4000)
    with pytest.raises(ValueError):
        call(eng, s, [0] * 3, 1.0, 0x2000, 16, 0x4000)
    host = pkg.Engine.poly_near_broad_pairs_host
    vx = np.zeros((4, 10), np.float32)
    with pytest.raises(ValueError):
        host(eng, vx, vx[:, :9], None, 1.0)                                 # planes of two shapes
    with pytest.raises(ValueError):
        host(eng, vx, vx, None, 1.0, vx_b=vx)                               # vx_b without vy_b
    with pytest.raises(ValueError):
        host(eng, vx, vx, None, 1.0, vy_b=vx)                               # vy_b without vx_b
    assert host(eng, vx[:, :0], vx[:, :0], None, 1.0).shape == (0, 2)       # an empty set: no device needed
