"""CPU tests of c2d_poly_pair_overlaps / c2d_rect_pair_overlaps at the C-ABI boundary, after tests/test_distance_boundary.py: the
header declares the entries and c2d_overlap, every shipped build exports the symbols, the Python mirror types them and lays the
record out as a C compiler does, and argument errors come back as statuses.  No compute entry point reaches a device here."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import overlap_ref  # noqa: E402

PKG_DIR = os.path.join(ROOT, "convex-2d-gpu-collision-detection_amd")
SYMBOLS = ("c2d_poly_pair_overlaps", "c2d_rect_pair_overlaps")
BUILDS = [os.path.join(PKG_DIR, "lib", n) for n in ("libc2d.so", "libc2d_fmad1.so", "libc2d_fmad2.so", "libc2d_nopretest.so",
                                                    "libc2d_movecheck.so", "libc2d_splitcheck.so")]
BUILDS.append(os.path.join(PKG_DIR, "lib-rehearsal", "libc2d.so"))
FIELDS = ["area", "iou", "cx", "cy", "area_a", "area_b", "hit", "flags", "pieces_a", "pieces_b", "reserved"]
OFFSETS = [0, 4, 8, 12, 16, 20, 24, 25, 26, 27, 28]
FLAGS = {"C2D_OVERLAP_DEGENERATE": 1, "C2D_OVERLAP_CLAMPED": 2, "C2D_OVERLAP_NO_CENTROID": 4, "C2D_OVERLAP_BAD_PAIR": 8}
LIST_ARGS = (r"\s*const\s+uint32_t\s*\*\s*d_pairs\s*,\s*size_t\s+n_pairs\s*,\s*const\s+unsigned\s+long\s+long\s*\*\s*d_n_pairs\s*,"
             r"\s*size_t\s+row_base\s*,\s*size_t\s+col_base\s*,\s*c2d_overlap\s*\*\s*d_out\s*,\s*c2d_stream\s+stream\s*\)")


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "c2d.h")).read(), flags=re.S)


def test_header_declares_the_entry_points_and_the_record():
    text = header_text()
    assert re.search(r"\bint\s+c2d_poly_pair_overlaps\s*\(\s*c2d_ctx\s*\*\s*\w*\s*,\s*const\s+c2d_poly_set\s*\*\s*a\s*,\s*const\s+c2d_poly_set\s*\*\s*b\s*,"
                     + LIST_ARGS, text)
    assert re.search(r"\bint\s+c2d_rect_pair_overlaps\s*\(\s*c2d_ctx\s*\*\s*\w*\s*,\s*const\s+float\s*\*\s*const\s+d_a\s*\[\s*8\s*\]\s*,\s*size_t\s+n_a\s*,"
                     r"\s*const\s+float\s*\*\s*const\s+d_b\s*\[\s*8\s*\]\s*,\s*size_t\s+n_b\s*," + LIST_ARGS, text)
    body = re.search(r"typedef\s+struct\s+c2d_overlap\s*\{([^}]*)\}\s*c2d_overlap\s*;", text).group(1)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in re.sub(r"^\s*\w+\s+", "", decl.strip()).split(",")]
    assert names == FIELDS
    for name, value in FLAGS.items():
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
    # the header states the rule under its title, and what it does not promise
    raw = open(os.path.join(ROOT, "include", "c2d.h")).read()
    assert "overlap queries: area, centroid and IoU of the intersection for listed pairs" in raw
    assert re.search(r"on side 0 only.*?non-convex or non-finite input nothing is promised.*?may differ in the last bits", raw, flags=re.S)
    assert re.search(r"#define\s+C2D_VERSION_MINOR\s+6\b", raw) or "c2d_version() stays 6" in raw


@pytest.mark.parametrize("path", BUILDS, ids=lambda p: os.path.relpath(p, PKG_DIR))
def test_every_build_exports_the_symbols(pkg, path):
    assert os.path.exists(path), path
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for symbol in SYMBOLS:
        assert symbol in names, f"{os.path.basename(path)} does not export {symbol}"


def test_mirror_types_the_symbols_and_the_record(pkg, tmp_path):
    from c2d_amd import binding

    lib = pkg.load_library()
    assert lib.c2d_version() == 6
    for symbol, contacts in zip(SYMBOLS, ("c2d_poly_pair_contacts", "c2d_rect_pair_contacts")):
        assert symbol in binding.EXPORTED_SYMBOLS
        res, args = binding._SIGNATURES[symbol]
        assert res is C.c_int and getattr(lib, symbol).argtypes == args
        assert (res, args) == binding._SIGNATURES[contacts]          # the contact call's signature, with another record behind d_out
    assert binding._SIGNATURES[SYMBOLS[0]][1][1] == C.POINTER(binding._PolySet)
    # sizeof(c2d_overlap), the field offsets and the flag values, from a C program compiled against the header
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "c2d.h"\nint main(void){ printf("%zu", sizeof(c2d_overlap)); '
                   + "".join('printf(" %%zu", offsetof(c2d_overlap, %s)); ' % f for f in FIELDS)
                   + "".join('printf(" %%d", %s); ' % f for f in FLAGS) + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    nums = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert nums[0] == 32 and nums[1:12] == OFFSETS
    dt = pkg.OVERLAP_DT
    assert dt is binding.OVERLAP_DT and dt.itemsize == 32 and list(dt.names) == FIELDS
    assert [dt.fields[f][1] for f in FIELDS] == OFFSETS
    assert [dt.fields[f][0] for f in FIELDS] == [np.dtype("<f4")] * 6 + [np.dtype("u1")] * 4 + [np.dtype("<u4")]
    assert nums[12:] == [pkg.OVERLAP_DEGENERATE, pkg.OVERLAP_CLAMPED, pkg.OVERLAP_NO_CENTROID, pkg.OVERLAP_BAD_PAIR] == list(FLAGS.values())
    # the reference the GPU tests compare with speaks of the same record
    assert overlap_ref.OVERLAP_DT == dt
    assert [overlap_ref.DEGENERATE, overlap_ref.CLAMPED, overlap_ref.NO_CENTROID, overlap_ref.BAD_PAIR] == list(FLAGS.values())


def test_null_and_bad_arguments_are_rejected_without_a_device(pkg):
    from c2d_amd import binding

    lib = pkg.load_library()
    s = binding._PolySet(16, 10, 0, 0x1000, 0x1000, 0x1000)
    p, o = C.c_void_p(0x1000), C.c_void_p(0x2000)
    planes = (C.c_void_p * 8)(*[0x1000] * 8)
    poly, rect = lib.c2d_poly_pair_overlaps, lib.c2d_rect_pair_overlaps
    # no ctx: refused whatever else is passed
    assert poly(None, C.byref(s), C.byref(s), p, 4, None, 0, 0, o, None) == -1
    assert poly(None, None, None, None, 0, None, 0, 0, None, None) == -1
    assert poly(None, C.byref(s), C.byref(s), p, 4, None, 0, 0, C.c_void_p(0x2008), None) == -1   # (a misaligned output too)
    assert rect(None, planes, 10, planes, 10, p, 4, None, 0, 0, o, None) == -1
    assert rect(None, None, 0, None, 0, None, 0, None, 0, 0, None, None) == -1
    # (with a ctx, every other refusal is checked on the GPU: tests/test_gpu_overlaps_contract.py::test_argument_errors)


def test_methods_check_their_shapes_before_touching_a_device(pkg):
    eng = object.__new__(pkg.Engine)   # no ctx: the shape checks come first
    with pytest.raises(ValueError):
        pkg.Engine.poly_pair_overlaps(eng, None, None, 0, 0, 0)
    with pytest.raises(ValueError):
        pkg.Engine.rect_pair_overlaps(eng, [0] * 7, 1, [0] * 8, 1, 0, 0, 0)
