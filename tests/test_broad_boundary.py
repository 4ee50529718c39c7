"""CPU tests of the broad-phase rectangle pair search (c2d_sat_rect_broad_pairs) at the C-ABI boundary: the header declares it,
every shipped build exports it, the Python mirror types it, and argument errors come back as statuses before any device is
touched."""
import ctypes as C
import os
import re

import pytest

from test_cross_boundary import BUILDS, PKG_DIR, exported, header_text

SYMBOL = "c2d_sat_rect_broad_pairs"


def test_header_declares_the_entry_point():
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % SYMBOL, text)
    assert m, SYMBOL
    assert len(m.group(1).split(",")) == 10


@pytest.mark.parametrize("path", BUILDS, ids=lambda p: os.path.relpath(p, PKG_DIR))
def test_every_build_exports_the_broad_symbol(pkg, path):
    assert os.path.exists(path), path
    assert SYMBOL in exported(path), f"{os.path.basename(path)} does not export {SYMBOL}"


def test_mirror_types_the_broad_symbol(pkg):
    from c2d_amd import binding

    lib = pkg.load_library()
    assert SYMBOL in binding.EXPORTED_SYMBOLS
    res, args = binding._SIGNATURES[SYMBOL]
    assert res is C.c_int and len(args) == 10
    assert args[5] is C.c_int and args[7] is C.c_size_t
    assert getattr(lib, SYMBOL).argtypes == args
    assert callable(pkg.Engine.sat_rect_broad_pairs) and callable(pkg.Engine.rect_broad_pairs_host)


def test_null_ctx_is_rejected(pkg):
    lib = pkg.load_library()
    planes = (C.c_void_p * 8)(*([0x1000] * 8))
    f = getattr(lib, SYMBOL)
    assert f(None, planes, 10, planes, 10, 0, C.c_void_p(0x1000), 16, C.c_void_p(0x1000), None) == -1
    assert f(None, planes, 10, planes, 10, 1, None, 0, C.c_void_p(0x1000), None) == -1
    assert f(None, None, 0, None, 0, 0, None, 0, None, None) == -1
    assert f(None, planes, 1 << 33, planes, 10, 0, None, 0, C.c_void_p(0x1000), None) == -1


def test_host_convenience_checks_its_planes_before_touching_a_device(pkg):
    import numpy as np

    eng = object.__new__(pkg.Engine)   # no ctx: the shape checks come first
    with pytest.raises(ValueError):
        pkg.Engine.rect_broad_pairs_host(eng, np.zeros((16, 4), np.float32))
    with pytest.raises(ValueError):
        pkg.Engine.rect_broad_pairs_host(eng, np.zeros((8, 4), np.float32), np.zeros((8,), np.float32))
    with pytest.raises(ValueError):
        pkg.Engine.rect_broad_pairs_host(eng, np.zeros((8, 4), np.float32), np.zeros((7, 4), np.float32), upper=True)
    with pytest.raises(ValueError):
        pkg.Engine.sat_rect_broad_pairs(eng, [0] * 8, 4, [0] * 7, 4, None, 0, 0)
