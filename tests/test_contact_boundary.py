"""CPU tests of the contact entry points (c2d_poly_pair_contacts / c2d_rect_pair_contacts) at the C-ABI boundary: the header
declares them and c2d_contact, every shipped build exports them, the Python mirror types them and lays the record out as a C
compiler does, and argument errors come back as statuses.  No compute entry point reaches a device here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "convex-2d-gpu-collision-detection_amd")
SYMBOLS = ("c2d_poly_pair_contacts", "c2d_rect_pair_contacts")
BUILDS = [os.path.join(PKG_DIR, "lib", n) for n in ("libc2d.so", "libc2d_fmad1.so", "libc2d_fmad2.so", "libc2d_nopretest.so",
                                                    "libc2d_movecheck.so", "libc2d_splitcheck.so")]
BUILDS.append(os.path.join(PKG_DIR, "lib-rehearsal", "libc2d.so"))
FIELDS = ["depth", "nx", "ny", "axis", "hit", "flags"]


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "c2d.h")).read(), flags=re.S)


def test_header_declares_both_entry_points_and_the_record():
    text = header_text()
    assert re.search(r"\bint\s+c2d_poly_pair_contacts\s*\(\s*c2d_ctx\s*\*\s*\w*\s*,\s*const\s+c2d_poly_set\s*\*\s*a\s*,\s*const\s+c2d_poly_set\s*\*\s*b\s*,"
                     r"\s*const\s+uint32_t\s*\*\s*d_pairs\s*,\s*size_t\s+n_pairs\s*,\s*const\s+unsigned\s+long\s+long\s*\*\s*d_n_pairs\s*,", text)
    assert re.search(r"\bint\s+c2d_rect_pair_contacts\s*\(\s*c2d_ctx\s*\*\s*\w*\s*,\s*const\s+float\s*\*\s*const\s+d_a\[8\]\s*,\s*size_t\s+n_a\s*,", text)
    body = re.search(r"typedef\s+struct\s+c2d_contact\s*\{([^}]*)\}\s*c2d_contact\s*;", text).group(1)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in re.sub(r"^\s*\w+\s+", "", decl.strip()).split(",")]
    assert names == FIELDS
    assert re.search(r"#define\s+C2D_CONTACT_NO_AXIS\s+1\b", text) and re.search(r"#define\s+C2D_CONTACT_BAD_PAIR\s+2\b", text)


@pytest.mark.parametrize("path", BUILDS, ids=lambda p: os.path.relpath(p, PKG_DIR))
def test_every_build_exports_the_symbols(pkg, path):
    assert os.path.exists(path), path
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in SYMBOLS:
        assert name in names, f"{os.path.basename(path)} does not export {name}"


def test_mirror_types_the_symbols_and_the_record(pkg, tmp_path):
    from c2d_amd import binding

    lib = pkg.load_library()
    assert lib.c2d_version() == 6
    for name, n_args in zip(SYMBOLS, (10, 12)):
        assert name in binding.EXPORTED_SYMBOLS
        res, args = binding._SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args
        assert getattr(lib, name).argtypes == args
    assert binding._SIGNATURES[SYMBOLS[0]][1][1] == binding._SIGNATURES[SYMBOLS[0]][1][2] == C.POINTER(binding._PolySet)
    # sizeof(c2d_contact) and the field offsets, from a C program compiled against the header
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "c2d.h"\nint main(void){ printf("%zu", sizeof(c2d_contact)); '
                   + "".join('printf(" %%zu", offsetof(c2d_contact, %s)); ' % f for f in FIELDS)
                   + 'printf(" %d %d", C2D_CONTACT_NO_AXIS, C2D_CONTACT_BAD_PAIR); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    nums = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert nums[0] == 16 and nums[1:7] == [0, 4, 8, 12, 14, 15]
    dt = pkg.CONTACT_DT
    assert dt is binding.CONTACT_DT and dt.itemsize == 16 and list(dt.names) == FIELDS
    assert [dt.fields[f][1] for f in FIELDS] == nums[1:7]
    assert [dt.fields[f][0] for f in FIELDS] == [np.dtype("<f4")] * 3 + [np.dtype("<u2"), np.dtype("u1"), np.dtype("u1")]
    assert nums[7:] == [binding.CONTACT_NO_AXIS, binding.CONTACT_BAD_PAIR]


def test_null_and_bad_arguments_are_rejected_without_a_device(pkg):
    from c2d_amd import binding

    lib = pkg.load_library()
    s = binding._PolySet(16, 10, 0, 0x1000, 0x1000, 0x1000)
    planes = (C.c_void_p * 8)(*[0x1000] * 8)
    p, o = C.c_void_p(0x1000), C.c_void_p(0x2000)
    poly, rect = lib.c2d_poly_pair_contacts, lib.c2d_rect_pair_contacts
    # no ctx: refused whatever else is passed
    assert poly(None, C.byref(s), C.byref(s), p, 4, None, 0, 0, o, None) == -1
    assert rect(None, planes, 10, planes, 10, p, 4, None, 0, 0, o, None) == -1
    assert poly(None, None, None, None, 0, None, 0, 0, None, None) == -1
    assert rect(None, None, 0, None, 0, None, 0, None, 0, 0, None, None) == -1
    assert poly(None, C.byref(s), C.byref(s), p, 4, None, 0, 0, C.c_void_p(0x2008), None) == -1   # (a misaligned output too)
    # (with a ctx, every other refusal is checked on the GPU: tests/test_gpu_pair_list_contract.py::test_argument_errors[contacts])


def test_host_conveniences_check_their_shapes_before_touching_a_device(pkg, wl):
    eng = object.__new__(pkg.Engine)   # no ctx: the shape checks come first
    vx, vy, k = wl.random_convex_polygon_set(8, seed=1)
    for args in ((vx, vy[:, :7], k), (vx, vy, k[:7]), (vx[0], vy[0], k)):
        with pytest.raises(ValueError):
            pkg.Engine.poly_contacts_host(eng, *args)
    with pytest.raises(ValueError):
        pkg.Engine.rect_contacts_host(eng, np.zeros((7, 4), np.float32))
    pairs, contacts = pkg.Engine.poly_contacts_host(eng, vx[:, :0], vy[:, :0], k[:0])
    assert pairs.shape == (0, 2) and contacts.shape == (0,) and contacts.dtype == pkg.CONTACT_DT
    pairs, contacts = pkg.Engine.rect_contacts_host(eng, np.zeros((8, 0), np.float32))
    assert pairs.shape == (0, 2) and contacts.dtype == pkg.CONTACT_DT
