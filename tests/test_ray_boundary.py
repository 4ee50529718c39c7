"""CPU tests of c2d_poly_ray_casts at the C-ABI boundary, after tests/test_distance_boundary.py: the header declares the entry and
c2d_ray_hit, every shipped build exports the symbol, the Python mirror types it and lays the record out as a C compiler does, and
argument errors come back as statuses.  No compute entry point reaches a device here."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ray_ref  # noqa: E402

PKG_DIR = os.path.join(ROOT, "convex-2d-gpu-collision-detection_amd")
SYMBOL = "c2d_poly_ray_casts"
BUILDS = [os.path.join(PKG_DIR, "lib", n) for n in ("libc2d.so", "libc2d_fmad1.so", "libc2d_fmad2.so", "libc2d_nopretest.so",
                                                    "libc2d_movecheck.so", "libc2d_splitcheck.so")]
BUILDS.append(os.path.join(PKG_DIR, "lib-rehearsal", "libc2d.so"))
FIELDS = ["poly", "t", "u", "edge", "hit", "flags"]
OFFSETS = [0, 4, 8, 12, 14, 15]


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "c2d.h")).read(), flags=re.S)


def test_header_declares_the_entry_point_and_the_record():
    text = header_text()
    assert re.search(r"\bint\s+c2d_poly_ray_casts\s*\(\s*c2d_ctx\s*\*\s*\w*\s*,\s*const\s+float\s*\*\s*const\s+d_rays\s*\[\s*4\s*\]\s*,\s*size_t\s+n_rays\s*,"
                     r"\s*const\s+c2d_poly_set\s*\*\s*b\s*,\s*size_t\s+col_base\s*,\s*c2d_ray_hit\s*\*\s*d_out\s*,\s*c2d_stream\s+stream\s*\)", text)
    body = re.search(r"typedef\s+struct\s+c2d_ray_hit\s*\{([^}]*)\}\s*c2d_ray_hit\s*;", text).group(1)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in re.sub(r"^\s*\w+\s+", "", decl.strip()).split(",")]
    assert names == FIELDS
    assert re.search(r"#define\s+C2D_RAY_START_INSIDE\s+1\b", text)
    # the header states the rule: the usable edge without a division, the inside rule, the strict pick and its tie order
    raw = open(os.path.join(ROOT, "include", "c2d.h")).read()
    assert re.search(r"den = dx \* ey - dy \* ex.*?exactly one sign occurs.*?strict t < best.*?smallest j, then inside before edges", raw, flags=re.S)
    assert "c2d_version() stays 6" in raw


@pytest.mark.parametrize("path", BUILDS, ids=lambda p: os.path.relpath(p, PKG_DIR))
def test_every_build_exports_the_symbol(pkg, path):
    assert os.path.exists(path), path
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert SYMBOL in names, f"{os.path.basename(path)} does not export {SYMBOL}"


def test_mirror_types_the_symbol_and_the_record(pkg, tmp_path):
    from c2d_amd import binding

    lib = pkg.load_library()
    assert lib.c2d_version() == 6
    assert SYMBOL in binding.EXPORTED_SYMBOLS
    res, args = binding._SIGNATURES[SYMBOL]
    assert res is C.c_int and getattr(lib, SYMBOL).argtypes == args
    assert args == [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(binding._PolySet), C.c_size_t, C.c_void_p, C.c_void_p]
    # sizeof(c2d_ray_hit), its alignment, the field offsets and the flag value, from a C program compiled against the header
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "c2d.h"\nint main(void){ printf("%zu %zu", sizeof(c2d_ray_hit), _Alignof(c2d_ray_hit)); '
                   + "".join('printf(" %%zu", offsetof(c2d_ray_hit, %s)); ' % f for f in FIELDS)
                   + 'printf(" %d", C2D_RAY_START_INSIDE); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    nums = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert nums[0] == 16 and nums[1] == 4 and nums[2:8] == OFFSETS      # (the 16-byte alignment is asked of d_out, not of the type)
    dt = pkg.RAY_HIT_DT
    assert dt is binding.RAY_HIT_DT and dt.itemsize == 16 and list(dt.names) == FIELDS
    assert [dt.fields[f][1] for f in FIELDS] == OFFSETS
    assert [dt.fields[f][0] for f in FIELDS] == [np.dtype("<u4"), np.dtype("<f4"), np.dtype("<f4"), np.dtype("<u2"), np.dtype("u1"), np.dtype("u1")]
    assert nums[8] == pkg.RAY_START_INSIDE == binding.RAY_START_INSIDE == 1
    # the reference the GPU tests compare with speaks of the same record
    assert ray_ref.RAY_HIT_DT == dt and ray_ref.START_INSIDE == pkg.RAY_START_INSIDE


def test_null_and_bad_arguments_are_rejected_without_a_device(pkg):
    from c2d_amd import binding

    lib = pkg.load_library()
    s = binding._PolySet(16, 10, 0, 0x1000, 0x1000, 0x1000)
    planes = (C.c_void_p * 4)(*[0x1000] * 4)
    o = C.c_void_p(0x2000)
    cast = lib.c2d_poly_ray_casts
    # no ctx: refused whatever else is passed
    assert cast(None, planes, 4, C.byref(s), 0, o, None) == -1
    assert cast(None, None, 0, None, 0, None, None) == -1
    assert cast(None, planes, 4, C.byref(s), 0, C.c_void_p(0x2008), None) == -1                      # (a misaligned output too)
    assert cast(None, planes, 4, C.byref(binding._PolySet(17, 10, 0, 0x1000, 0x1000, 0x1000)), 0, o, None) == -1   # (rows out of range)
    assert cast(None, planes, 4, C.byref(s), (1 << 32) - 9, o, None) == -1                           # (col_base + n_b > 2^32)
    assert cast(None, planes, (1 << 32) + 1, C.byref(s), 0, o, None) == -1                           # (n_rays > 2^32)
    # (with a ctx, every refusal is checked on the GPU, where a ctx can be made: tests/test_gpu_ray_casts.py::test_argument_errors)


def test_method_checks_its_shapes_before_touching_a_device(pkg):
    eng = object.__new__(pkg.Engine)   # no ctx: the shape checks come first
    with pytest.raises(ValueError):
        pkg.Engine.poly_ray_casts(eng, None, 0, None, 0)
    with pytest.raises(ValueError):
        pkg.Engine.poly_ray_casts(eng, [0] * 3, 1, pkg.binding._PolySet(), 0)
    with pytest.raises(ValueError):
        pkg.Engine.poly_ray_casts(eng, [0] * 4, 1, None, 0)
