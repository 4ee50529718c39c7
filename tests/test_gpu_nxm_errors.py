"""The refusals of the six N x M entry points, word for word: the rectangle and polygon cross forms (mask and pair list) and the
two broad phases share one host front end (csrc/c2d_cross.hpp), and a caller who makes exactly one mistake must go on reading the
text each entry point has always given.  Every call here is refused on the host before anything is launched; the expected
strings are literals, copied from the sources as they stood before the front end was shared."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 100
RM, RP, RB = "c2d_sat_rect_cross_mask", "c2d_sat_rect_cross_pairs", "c2d_sat_rect_broad_pairs"
PM, PP, PB = "c2d_sat_poly_cross_mask", "c2d_sat_poly_cross_pairs", "c2d_sat_poly_broad_pairs"

FLAG = "unknown flag"
BASE = "row_base + n_a and col_base + n_b must stay below 2^62"
NO_MASK, ALIGN, LD = "NULL mask", "the mask must be 8-byte aligned", "ld_words < ceil(n_b / 64)"
NO_COUNT, NO_PAIRS = "d_count is required", "NULL pair buffer"
CROSS_LIMIT = "global indices must stay below 2^32 (the list is u32)"
BROAD_LIMIT = "n_a and n_b must stay at or below 2^32 (the list is u32)"
NO_ARG, NO_PLANE, NO_SET = "NULL argument", "NULL plane", "NULL set"
ROWS, STRIDE, PLANE_ALIGN = "rows must be 1..C2D_POLY_KMAX", "stride < n", "planes must be 4-byte aligned"
PAST_62 = (1 << 62) - 99       # + 100 objects: past 2^62
PAST_32 = (1 << 32) - 99       # + 100 objects: index 2^32


class Args:
    """100 rectangles, 100 polygons and the output buffers, on the device; the builders of every call's arguments"""

    def __init__(self, eng):
        rng = np.random.default_rng(7)
        self.eng = eng
        self.rect = eng.to_device(rng.uniform(-5, 5, (8, N)).astype(np.float32))
        self.poly = eng.to_device(rng.uniform(-5, 5, (2, 16, N)).astype(np.float32))
        self.mask = eng.zeros((N, 2), np.uint64)
        self.pairs = eng.zeros((10, 2), np.uint32)
        self.count = eng.zeros(1, np.uint64)

    def free(self):
        for x in (self.rect, self.poly, self.mask, self.pairs, self.count):
            x.free()

    def planes(self, null_at=None):
        p = [self.rect.row(k) for k in range(8)]
        if null_at is not None:
            p[null_at] = None
        return (C.c_void_p * 8)(*p)

    def set(self, **kw):
        return self.eng.poly_set(kw.get("vx", self.poly.row(0)), kw.get("vy", self.poly.row(1)), None, kw.get("n", N), kw.get("rows", 16),
                                 kw.get("stride", 0))

    # one call of each entry point; keywords replace single arguments
    def rect_mask(self, a="ok", b="ok", n_a=N, n_b=N, row_base=0, col_base=0, flags=0, mask="ok", ld=2):
        a, b = (self.planes() if x == "ok" else x for x in (a, b))
        return self.eng.lib.c2d_sat_rect_cross_mask(self.eng.h, a, n_a, b, n_b, row_base, col_base, flags, self.mask.ptr if mask == "ok" else mask, ld,
                                                    None, None)

    def rect_pairs(self, a="ok", b="ok", n_a=N, n_b=N, row_base=0, col_base=0, flags=0, pairs="ok", cap=10, count="ok"):
        a, b = (self.planes() if x == "ok" else x for x in (a, b))
        return self.eng.lib.c2d_sat_rect_cross_pairs(self.eng.h, a, n_a, b, n_b, row_base, col_base, flags, self.pairs.ptr if pairs == "ok" else pairs,
                                                     cap, self.count.ptr if count == "ok" else count, None)

    def rect_broad(self, a="ok", b="ok", n_a=N, n_b=N, flags=0, pairs="ok", cap=10, count="ok"):
        a, b = (self.planes() if x == "ok" else x for x in (a, b))
        return self.eng.lib.c2d_sat_rect_broad_pairs(self.eng.h, a, n_a, b, n_b, flags, self.pairs.ptr if pairs == "ok" else pairs, cap,
                                                     self.count.ptr if count == "ok" else count, None)

    def poly_mask(self, a="ok", b="ok", row_base=0, col_base=0, flags=0, mask="ok", ld=2):
        a, b = (C.byref(self.set()) if x == "ok" else (x if x is None else C.byref(x)) for x in (a, b))
        return self.eng.lib.c2d_sat_poly_cross_mask(self.eng.h, a, b, row_base, col_base, flags, self.mask.ptr if mask == "ok" else mask, ld, None, None)

    def poly_pairs(self, a="ok", b="ok", row_base=0, col_base=0, flags=0, pairs="ok", cap=10, count="ok"):
        a, b = (C.byref(self.set()) if x == "ok" else (x if x is None else C.byref(x)) for x in (a, b))
        return self.eng.lib.c2d_sat_poly_cross_pairs(self.eng.h, a, b, row_base, col_base, flags, self.pairs.ptr if pairs == "ok" else pairs, cap,
                                                     self.count.ptr if count == "ok" else count, None)

    def poly_broad(self, a="ok", b="ok", flags=0, pairs="ok", cap=10, count="ok"):
        a, b = (C.byref(self.set()) if x == "ok" else (x if x is None else C.byref(x)) for x in (a, b))
        return self.eng.lib.c2d_sat_poly_broad_pairs(self.eng.h, a, b, flags, self.pairs.ptr if pairs == "ok" else pairs, cap,
                                                     self.count.ptr if count == "ok" else count, None)


# (expected text, the call with its one fault)
CASES = [
    # ---- rectangle cross mask
    (RM + ": " + FLAG, lambda x: x.rect_mask(flags=2)),
    (RM + ": " + FLAG, lambda x: x.rect_mask(flags=-1)),
    (RM + ": " + BASE, lambda x: x.rect_mask(row_base=PAST_62)),
    (RM + ": " + BASE, lambda x: x.rect_mask(col_base=PAST_62)),
    (RM + ": " + NO_MASK, lambda x: x.rect_mask(mask=None)),
    (RM + ": " + ALIGN, lambda x: x.rect_mask(mask=x.mask.ptr + 4)),
    (RM + ": " + LD, lambda x: x.rect_mask(ld=1)),
    (RM + ": " + NO_ARG, lambda x: x.rect_mask(a=None)),
    (RM + ": " + NO_PLANE, lambda x: x.rect_mask(a=x.planes(null_at=3))),
    (RM + ": " + NO_PLANE, lambda x: x.rect_mask(b=x.planes(null_at=7))),
    # ---- rectangle cross pair list
    (RP + ": " + FLAG, lambda x: x.rect_pairs(flags=4)),
    (RP + ": " + BASE, lambda x: x.rect_pairs(row_base=PAST_62)),
    (RP + ": " + BASE, lambda x: x.rect_pairs(col_base=PAST_62)),
    (RP + ": " + NO_COUNT, lambda x: x.rect_pairs(count=None)),
    (RP + ": " + NO_PAIRS, lambda x: x.rect_pairs(pairs=None)),
    (RP + ": " + CROSS_LIMIT, lambda x: x.rect_pairs(row_base=PAST_32)),
    (RP + ": " + CROSS_LIMIT, lambda x: x.rect_pairs(col_base=PAST_32)),
    (RP + ": " + NO_ARG, lambda x: x.rect_pairs(b=None)),
    (RP + ": " + NO_PLANE, lambda x: x.rect_pairs(a=x.planes(null_at=0))),
    # ---- rectangle broad phase
    (RB + ": " + FLAG, lambda x: x.rect_broad(flags=2)),
    (RB + ": " + NO_COUNT, lambda x: x.rect_broad(count=None)),
    (RB + ": " + NO_PAIRS, lambda x: x.rect_broad(pairs=None)),
    (RB + ": " + BROAD_LIMIT, lambda x: x.rect_broad(n_a=(1 << 32) + 1)),
    (RB + ": " + BROAD_LIMIT, lambda x: x.rect_broad(n_b=(1 << 32) + 1)),
    (RB + ": " + NO_ARG, lambda x: x.rect_broad(a=None)),
    (RB + ": " + NO_PLANE, lambda x: x.rect_broad(b=x.planes(null_at=5))),
    # ---- polygon cross mask
    (PM + ": " + FLAG, lambda x: x.poly_mask(flags=2)),
    (PM + ": " + FLAG, lambda x: x.poly_mask(flags=-1)),
    (PM + ": " + BASE, lambda x: x.poly_mask(row_base=PAST_62)),
    (PM + ": " + BASE, lambda x: x.poly_mask(col_base=PAST_62)),
    (PM + ": " + NO_MASK, lambda x: x.poly_mask(mask=None)),
    (PM + ": " + ALIGN, lambda x: x.poly_mask(mask=x.mask.ptr + 4)),
    (PM + ": " + LD, lambda x: x.poly_mask(ld=1)),
    (PM + ": " + NO_SET, lambda x: x.poly_mask(a=None)),
    (PM + ": " + NO_SET, lambda x: x.poly_mask(b=None)),
    (PM + ": set a: " + NO_PLANE, lambda x: x.poly_mask(a=x.set(vx=0))),
    (PM + ": set b: " + NO_PLANE, lambda x: x.poly_mask(b=x.set(vy=0))),
    (PM + ": set a: " + PLANE_ALIGN, lambda x: x.poly_mask(a=x.set(vx=x.poly.row(0) + 2))),
    (PM + ": set b: " + STRIDE, lambda x: x.poly_mask(b=x.set(stride=N - 1))),
    (PM + ": set a: " + ROWS, lambda x: x.poly_mask(a=x.set(rows=0))),
    (PM + ": set b: " + ROWS, lambda x: x.poly_mask(b=x.set(rows=17))),
    # ---- polygon cross pair list
    (PP + ": " + FLAG, lambda x: x.poly_pairs(flags=2)),
    (PP + ": " + BASE, lambda x: x.poly_pairs(row_base=PAST_62)),
    (PP + ": " + BASE, lambda x: x.poly_pairs(col_base=PAST_62)),
    (PP + ": " + NO_COUNT, lambda x: x.poly_pairs(count=None)),
    (PP + ": " + NO_PAIRS, lambda x: x.poly_pairs(pairs=None)),
    (PP + ": " + CROSS_LIMIT, lambda x: x.poly_pairs(row_base=PAST_32)),
    (PP + ": " + CROSS_LIMIT, lambda x: x.poly_pairs(col_base=PAST_32)),
    (PP + ": " + NO_SET, lambda x: x.poly_pairs(a=None)),
    (PP + ": set b: " + NO_PLANE, lambda x: x.poly_pairs(b=x.set(vx=0))),
    (PP + ": set a: " + STRIDE, lambda x: x.poly_pairs(a=x.set(stride=N - 1))),
    (PP + ": set a: " + ROWS, lambda x: x.poly_pairs(a=x.set(rows=17))),
    (PP + ": set b: " + ROWS, lambda x: x.poly_pairs(b=x.set(rows=0))),
    # ---- polygon broad phase
    (PB + ": " + FLAG, lambda x: x.poly_broad(flags=2)),
    (PB + ": " + NO_COUNT, lambda x: x.poly_broad(count=None)),
    (PB + ": " + NO_PAIRS, lambda x: x.poly_broad(pairs=None)),
    (PB + ": " + BROAD_LIMIT, lambda x: x.poly_broad(a=x.set(n=(1 << 32) + 1))),
    (PB + ": " + BROAD_LIMIT, lambda x: x.poly_broad(b=x.set(n=(1 << 32) + 1))),
    (PB + ": " + NO_SET, lambda x: x.poly_broad(b=None)),
    (PB + ": set a: " + NO_PLANE, lambda x: x.poly_broad(a=x.set(vy=0))),
    (PB + ": set b: " + STRIDE, lambda x: x.poly_broad(b=x.set(stride=N - 1))),
    (PB + ": set a: " + ROWS, lambda x: x.poly_broad(a=x.set(rows=0))),
    (PB + ": set b: " + ROWS, lambda x: x.poly_broad(b=x.set(rows=17))),
]


def test_single_fault_texts(eng):
    x = Args(eng)
    try:
        wrong = []
        for q, (text, call) in enumerate(CASES):
            status = call(x)
            got = eng.lib.c2d_last_error(eng.h).decode()
            if status != -1 or got != text:
                wrong.append((q, status, got, text))
        assert not wrong, wrong
        # nothing was launched and nothing written: the buffers are as they were made, and the ctx has no deferred error
        eng.synchronize()
        eng.check_async()
        assert not x.mask.get().any() and not x.pairs.get().any() and int(x.count.get()[0]) == 0
        # and the same arguments without a fault are accepted by every entry point
        for ok in (x.rect_mask, x.rect_pairs, x.rect_broad, x.poly_mask, x.poly_pairs, x.poly_broad):
            assert ok() == 0
        eng.synchronize()
        eng.check_async()
    finally:
        x.free()
