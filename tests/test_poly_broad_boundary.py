"""CPU tests of the broad-phase polygon pair search (c2d_sat_poly_broad_pairs) at the C-ABI boundary: the header declares it,
every shipped build exports it, the Python mirror types it, and argument errors come back as statuses before any device is
touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_cross_boundary import BUILDS, PKG_DIR, exported, header_text

SYMBOL = "c2d_sat_poly_broad_pairs"


def test_header_declares_the_entry_point():
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % SYMBOL, text)
    assert m, SYMBOL
    assert len(m.group(1).split(",")) == 8
    assert "c2d_version() stays 6" in header_text()


@pytest.mark.parametrize("path", BUILDS, ids=lambda p: os.path.relpath(p, PKG_DIR))
def test_every_build_exports_the_poly_broad_symbol(pkg, path):
    assert os.path.exists(path), path
    assert SYMBOL in exported(path), f"{os.path.basename(path)} does not export {SYMBOL}"


def test_mirror_types_the_poly_broad_symbol(pkg):
    from c2d_amd import binding

    lib = pkg.load_library()
    assert SYMBOL in binding.EXPORTED_SYMBOLS
    res, args = binding._SIGNATURES[SYMBOL]
    assert res is C.c_int and len(args) == 8
    assert args[1] == C.POINTER(binding._PolySet) and args[2] == C.POINTER(binding._PolySet)
    assert args[3] is C.c_int and args[5] is C.c_size_t
    assert getattr(lib, SYMBOL).argtypes == args
    assert callable(pkg.Engine.sat_poly_broad_pairs) and callable(pkg.Engine.poly_broad_pairs_host)


def test_null_ctx_and_bad_arguments_return_statuses(pkg):
    lib = pkg.load_library()
    f = getattr(lib, SYMBOL)
    s = pkg.Engine.poly_set(0x1000, 0x2000, 0x3000, 10, 16)
    for flags in (0, 1, 2, -1):
        assert f(None, C.byref(s), C.byref(s), flags, C.c_void_p(0x1000), 16, C.c_void_p(0x1000), None) == -1
    assert f(None, None, None, 0, None, 0, None, None) == -1
    assert f(None, C.byref(s), None, 0, None, 0, C.c_void_p(0x1000), None) == -1
    big = pkg.Engine.poly_set(0x1000, 0x2000, None, 1 << 33, 17)
    assert f(None, C.byref(big), C.byref(s), 0, None, 0, C.c_void_p(0x1000), None) == -1


def test_host_convenience_checks_its_arrays_before_touching_a_device(pkg):
    eng = object.__new__(pkg.Engine)   # no ctx: the shape checks come first
    v = np.zeros((16, 4), np.float32)
    k = np.full(4, 3, np.uint8)
    bad = [
        lambda: pkg.Engine.poly_broad_pairs_host(eng, np.zeros((17, 4), np.float32), np.zeros((17, 4), np.float32), None),   # 17 rows
        lambda: pkg.Engine.poly_broad_pairs_host(eng, v, np.zeros((16, 5), np.float32), k),                                   # vx, vy differ
        lambda: pkg.Engine.poly_broad_pairs_host(eng, v, v, np.full(5, 3, np.uint8)),                                         # counts [5] for n = 4
        lambda: pkg.Engine.poly_broad_pairs_host(eng, v, v, k, np.zeros((8,), np.float32), np.zeros((8,), np.float32), None),  # set B not 2-D
        lambda: pkg.Engine.poly_broad_pairs_host(eng, v, v, k, v, None, None),                                                # vx_b without vy_b
        lambda: pkg.Engine.poly_broad_pairs_host(eng, v, v, k, None, v, None),                                                # vy_b without vx_b
        lambda: pkg.Engine.sat_poly_broad_pairs(eng, None, None, None, 0, 0),                                                 # not poly_set()s
    ]
    for q, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert q >= 0
