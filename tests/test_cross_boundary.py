"""CPU tests of the all-pairs (N x M) rectangle entry points at the C-ABI boundary: every shipped build exports them, the
Python mirror types them and agrees with the header on the flag, and argument errors come back as statuses.  No compute
entry point reaches a device here."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "convex-2d-gpu-collision-detection_amd")
CROSS_SYMBOLS = ("c2d_sat_rect_cross_mask", "c2d_sat_rect_cross_pairs")
# every build of the library the suite makes (Makefile `all`)
BUILDS = [os.path.join(PKG_DIR, "lib", n) for n in ("libc2d.so", "libc2d_fmad1.so", "libc2d_fmad2.so", "libc2d_nopretest.so",
                                                    "libc2d_movecheck.so", "libc2d_splitcheck.so")]
BUILDS.append(os.path.join(PKG_DIR, "lib-rehearsal", "libc2d.so"))


def header_text():
    return open(os.path.join(ROOT, "include", "c2d.h")).read()


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_header_declares_both_entry_points():
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    for name in CROSS_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name


@pytest.mark.parametrize("path", BUILDS, ids=lambda p: os.path.relpath(p, PKG_DIR))
def test_every_build_exports_the_cross_symbols(pkg, path):
    assert os.path.exists(path), path
    names = exported(path)
    for name in CROSS_SYMBOLS:
        assert name in names, f"{os.path.basename(path)} does not export {name}"


def test_mirror_types_the_cross_symbols(pkg):
    from c2d_amd import binding

    lib = pkg.load_library()
    for name in CROSS_SYMBOLS:
        assert name in binding.EXPORTED_SYMBOLS
        res, args = binding._SIGNATURES[name]
        assert res is C.c_int and len(args) == 12
        assert getattr(lib, name).argtypes == args


def test_upper_flag_matches_header(pkg):
    from c2d_amd import binding

    m = re.search(r"#define\s+C2D_CROSS_UPPER\s+(\d+)", header_text())
    assert m, "include/c2d.h does not define C2D_CROSS_UPPER"
    assert binding.CROSS_UPPER == int(m.group(1)) == pkg.CROSS_UPPER


def test_null_ctx_is_rejected(pkg):
    lib = pkg.load_library()
    planes = (C.c_void_p * 8)(*([0x1000] * 8))
    assert lib.c2d_sat_rect_cross_mask(None, planes, 10, planes, 10, 0, 0, 0, C.c_void_p(0x1000), 1, None, None) == -1
    assert lib.c2d_sat_rect_cross_pairs(None, planes, 10, planes, 10, 0, 0, 0, C.c_void_p(0x1000), 16, C.c_void_p(0x1000), None) == -1
    assert lib.c2d_sat_rect_cross_mask(None, None, 0, None, 0, 0, 0, 0, None, 0, None, None) == -1
    assert lib.c2d_sat_rect_cross_pairs(None, None, 0, None, 0, 0, 0, 0, None, 0, None, None) == -1


def test_host_convenience_checks_its_planes_before_touching_a_device(pkg):
    import numpy as np

    eng = object.__new__(pkg.Engine)   # no ctx: the shape check comes first
    with pytest.raises(ValueError):
        pkg.Engine.rect_cross_pairs_host(eng, np.zeros((16, 4), np.float32), np.zeros((8, 4), np.float32))
    with pytest.raises(ValueError):
        pkg.Engine._cross_planes([0] * 8, [0] * 16)
